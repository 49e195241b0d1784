"""The SpMV instantiations of the device solvers and the cases that run them cannot drift apart (no GPU needed).

pyiga_amd/csrc/solve.hip picks the group width of k_spmv / k_csr_spmv with spmv_gw(maxlen) and maps it to one instantiation
per width in the dispatch table of each family (with_spmv_kernel, with_csr_spmv_kernel), through which both the launch and the
occupancy query go; the SpMV and vector kernels loop over their rows with grids of at most NB_SPMV_MAX and NB_VEC blocks.  tests/_solver_cases.py restates all of it, and tests/test_solver_kernels_gpu.py runs
its cases.  A new width, a changed threshold, a dropped case line or a larger grid constant fails here: the table must then
be extended so that every instantiation, and the second pass of every grid-stride loop, still runs under a test."""
import numpy as np
import pytest

import _solver_cases as sc


@pytest.fixture(scope='module')
def src():
    return sc.read_source()


def test_constants(src):
    assert sc.parse_constants(src) == {'BLOCK': sc.BLOCK, 'NB_VEC': sc.NB_VEC, 'NB_SPMV_MAX': sc.NB_SPMV_MAX}


def test_spmv_gw_thresholds(src):
    pairs, default = sc.parse_gw_thresholds(src)
    assert pairs == sc.GW_THRESHOLDS and default == 4
    assert tuple(sorted({g for _, g in pairs} | {default})) == sc.GWS
    # the restatement at and around every threshold
    for t, g in pairs:
        assert sc.spmv_gw(t) == g and sc.spmv_gw(t - 1) < g
    assert sc.spmv_gw(1) == 4 and sc.spmv_gw(10 ** 6) == 64


def test_dispatch_table_case_lines(src):
    """Every width has a case line in the dispatch table of each kernel family; the label is the width it names (the default:
    GW 4)."""
    d = sc.parse_dispatch(src)
    for name, inst in (('k_spmv', sc.SPMV_INSTANCES), ('k_csr_spmv', sc.CSR_SPMV_INSTANCES)):
        lines = d[name]
        assert len(lines) == len(sc.GWS), (name, sorted(lines, key=str))
        assert {(gw, u) for _, gw, u in lines} == inst, (name, sorted(lines, key=str))
        for label, gw, _ in lines:
            assert label == gw or (label is None and gw == 4), (name, label, gw)


def test_no_instance_outside_the_dispatch_tables(src):
    """No instantiation is named outside the tables: the launch and the occupancy query take their kernel from the same table,
    so the query asks about the kernel that is launched."""
    assert sc.instances_outside_tables(src) == []


def test_spmv_pass_bounds():
    assert [sc.spmv_pass_rows(g) for g in sc.GWS] == [524288, 262144, 131072, 65536, 32768]
    assert sc.vec_pass_rows() == 262144


def test_axis_ranges_of_single_and_repeated_knots():
    from pyiga_amd import bspline
    for p in range(1, 7):
        jlo, jhi = sc.axis_ranges(bspline.make_knots(p, 0.0, 1.0, 3 * p + 2))
        assert (jhi - jlo).max() == 2 * p + 1 and (jhi - jlo).min() == p + 1
    # double knots: C^(p-2) joints, the supports of fewer functions overlap
    jlo, jhi = sc.axis_ranges(bspline.make_knots(2, 0.0, 1.0, 6, mult=2))
    assert (jhi - jlo).max() == 5
    jlo, jhi = sc.axis_ranges(bspline.make_knots(1, 0.0, 1.0, 6, mult=2))
    assert (jhi - jlo).max() == 2


def test_patch_cases_reach_every_width_past_one_grid():
    ids = [c.id for c in sc.PATCH_CASES]
    assert len(set(ids)) == len(ids)
    past = set()
    for c in sc.PATCH_CASES:
        kvs = c.kvs()
        rows = int(np.prod([kv.numdofs for kv in kvs]))
        maxlen = sc.patch_maxlen(kvs)
        assert sc.spmv_gw(maxlen) == c.gw, (c.id, maxlen, c.gw)
        if rows > sc.spmv_pass_rows(c.gw):
            past.add(c.gw)
    assert {c.gw for c in sc.PATCH_CASES} == set(sc.GWS)
    assert past == set(sc.GWS), sorted(past)
    # C4's degree, mixed degrees and repeated knots
    assert any(c.dim == 3 and all(a[0] == 4 for a in c.axes) for c in sc.PATCH_CASES)
    assert any(len({a[0] for a in c.axes}) > 1 for c in sc.PATCH_CASES)
    assert any(any(a[2] > 1 for a in c.axes) for c in sc.PATCH_CASES)


def test_multipatch_cases_reach_every_width_past_one_grid():
    ids = [c.id for c in sc.MULTIPATCH_CASES]
    assert len(set(ids)) == len(ids)
    past = set()
    for c in sc.MULTIPATCH_CASES:
        MP = c.build()
        S = sc.multipatch_pattern(MP)
        assert sc.spmv_gw(sc.max_row(S)) == c.gw, (c.id, sc.max_row(S), c.gw)
        if MP.numdofs > sc.spmv_pass_rows(c.gw):
            past.add(c.gw)
    assert {c.gw for c in sc.MULTIPATCH_CASES} == set(sc.GWS)
    assert past == set(sc.GWS), sorted(past)


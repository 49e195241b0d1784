"""Diagonal outer pairs of the 3D stiffness chain k_geoA -> k_bf3 (sumfact.hip: plan_diag_skip): k_geoA does not write the K1
slices that repeat another array's, k_bf3 reads the written one for both slots and builds the lines of the role of last-axis
type 2 from the window of the role of type 1.  `IGX_NO_DIAG_SKIP=1` (read when a patch is created) keeps every slice written and
read as before.  The matrix must be the same BITS either way; needs a real MI355X:  pytest -m gpu.

Shapes: the smallest at which the change can go wrong -- axis 0 with one span (every pair in one window), p + 1 and 2p + 3 spans;
the last axis one row longer than a tile of k_bf3 (two tiles) and the mid axis 4 (p + 1) rows (two chunks of the mid axis: with so
few blocks bf2_choose_chunks cuts wherever a chunk keeps 2 (p + 1) rows).
"""
import numpy as np
import pytest
import scipy.sparse

from conftest import rel_maxdiff
import _bf3_cases as bc

pytestmark = pytest.mark.gpu

RTOL = 1e-12            # sum-factorised against entry-wise: the bound of tests/test_gpu_parity.py
KNOB = 'IGX_NO_DIAG_SKIP'


@pytest.fixture(scope='module')
def iga():
    import pyiga_amd
    pyiga_amd._lib.context()          # raises if no GPU / library: there is no fallback
    return pyiga_amd


def _geo(iga, name):
    g = iga.geometry
    return {'twisted_box': g.twisted_box,
            'cylinder': lambda: g.tensor_product(g.line_segment(0.0, 1.0), g.quarter_annulus())}[name]()


def kv_mults(iga, p, mults):
    n = len(mults) + 1
    inner = np.repeat(np.arange(1, n) / n, mults)
    return iga.bspline.KnotVector(np.concatenate([np.zeros(p + 1), inner, np.ones(p + 1)]), p)


def two_tiles_two_chunks(iga, p1, p2, q, n0=None):
    """Knot vectors of the mid and the last axis (single knots): 4 (p1 + 1) rows on the mid axis, RMAX + 1 rows on the last."""
    mk = iga.bspline.make_knots
    rmax = bc.bf3_rmax(p1 + 1, p2 + 1, q, 'stiffness')
    return mk(p1, 0., 1., 4 * (p1 + 1) - p1), mk(p2, 0., 1., rmax + 1 - p2)


def both_ways(monkeypatch, make, run):
    """run(make()) with the skip on (default) and off; -> [(result, last_path)] in that order."""
    out = []
    for off in (False, True):
        if off:
            monkeypatch.setenv(KNOB, '1')
        else:
            monkeypatch.delenv(KNOB, raising=False)
        obj = make()
        patch = getattr(obj, 'patch', obj)
        A = run(obj)
        out.append((A, patch.last_path()))
        patch.close()
    monkeypatch.delenv(KNOB, raising=False)
    return out


def check_stiffness(iga, monkeypatch, kvs, geo, path=None, entrywise=True):
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')
    (A, pa), (B, pb) = both_ways(monkeypatch, lambda: iga.assemblers.DevicePatch(kvs, geo), lambda pt: pt.csr('stiffness', algo='sumfact'))
    tag = ([kv.p for kv in kvs], [kv.numdofs for kv in kvs], sorted(pa))
    assert pa == pb, tag
    if path is not None:
        assert pa == path, tag
    assert not np.isnan(A.data).any(), tag
    assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices), tag
    assert np.array_equal(A.data, B.data), (tag, int((A.data != B.data).sum()))
    assert abs(A - A.T).max() == 0.0, tag
    if entrywise:
        patch = iga.assemblers.DevicePatch(kvs, geo)
        E = patch.csr('stiffness', algo='entrywise')
        patch.close()
        assert np.array_equal(A.indptr, E.indptr) and np.array_equal(A.indices, E.indices), tag
        assert rel_maxdiff(A, E) <= RTOL, (tag, rel_maxdiff(A, E))
    return A


BF3 = {'geoA', 'fused', 'both', 'bf3'}


@pytest.mark.parametrize('spans0', ['one', 'p+1', '2p+3'])
@pytest.mark.parametrize('gname', ['cylinder', 'twisted_box'])
@pytest.mark.parametrize('p', [2, 3, 4])
def test_equal_degrees(iga, monkeypatch, p, gname, spans0):
    """Degrees 2 - 4 on a NURBS and a B-spline map: same bits with and without the skip, exactly symmetric, the entry-wise kernel's
    matrix to rounding."""
    n0 = {'one': 1, 'p+1': p + 1, '2p+3': 2 * p + 3}[spans0]
    kv1, kv2 = two_tiles_two_chunks(iga, p, p, p + 1)
    check_stiffness(iga, monkeypatch, (iga.bspline.make_knots(p, 0., 1., n0), kv1, kv2), _geo(iga, gname), BF3)


def test_repeated_knot_on_the_mid_axis(iga, monkeypatch):
    """MULT: the window of the swept axis moves by the multiplicity of a knot."""
    mk = iga.bspline.make_knots
    _, kv2 = two_tiles_two_chunks(iga, 3, 3, 4)
    kv1 = kv_mults(iga, 3, [1, 2, 1, 1, 3, 1, 1, 2, 1])
    check_stiffness(iga, monkeypatch, (mk(3, 0., 1., 4), kv1, kv2), _geo(iga, 'cylinder'), BF3)


def test_repeated_knots_on_the_last_axis(iga, monkeypatch):
    """TR: the chain runs on the twin patch (mid and last axis exchanged) and stores into this patch's layout."""
    mk = iga.bspline.make_knots
    kv1, _ = two_tiles_two_chunks(iga, 3, 3, 4)
    kv2 = kv_mults(iga, 3, [2, 1, 3, 1, 2, 1, 1, 2])
    # (the twin's last axis is this patch's mid axis: RMAX + 1 rows there)
    kvm = mk(3, 0., 1., bc.bf3_rmax(4, 4, 4, 'stiffness') + 1 - 3)
    check_stiffness(iga, monkeypatch, (mk(3, 0., 1., 5), kvm, kv2), _geo(iga, 'twisted_box'), BF3 | {'twin'})
    check_stiffness(iga, monkeypatch, (mk(3, 0., 1., 1), kv1, kv2), _geo(iga, 'cylinder'), BF3 | {'twin'})


def test_unequal_degrees(iga, monkeypatch):
    """Degrees 4 x 2 x 4: k_bf3<3, 5, 5>."""
    mk = iga.bspline.make_knots
    kv1, kv2 = two_tiles_two_chunks(iga, 2, 4, 5)
    check_stiffness(iga, monkeypatch, (mk(4, 0., 1., 5), kv1, kv2), _geo(iga, 'cylinder'), BF3)


def test_repeated_knot_on_axis_0(iga, monkeypatch):
    """Several dofs leave the axis-0 window at one span end: the flush steps behind the first come from the step table."""
    kv1, kv2 = two_tiles_two_chunks(iga, 3, 3, 4)
    check_stiffness(iga, monkeypatch, (kv_mults(iga, 3, [1, 2, 1, 3, 1]), kv1, kv2), _geo(iga, 'twisted_box'), BF3)


@pytest.mark.parametrize('cuts', [(0, 4, 9), (0, 1, 5, 9)])
def test_row_slabs(iga, monkeypatch, cuts):
    """Slabs of axis-0 rows: every slab begins and ends with a diagonal pair it owns; stacked, they are the whole patch bit for bit
    (which in turn is the matrix without the skip)."""
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')
    p = 3
    kv1, kv2 = two_tiles_two_chunks(iga, p, p, p + 1)
    kvs = (iga.bspline.make_knots(p, 0., 1., 6), kv1, kv2)
    assert kvs[0].numdofs == cuts[-1]
    geo = _geo(iga, 'cylinder')
    A = check_stiffness(iga, monkeypatch, kvs, geo, BF3, entrywise=False)
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        patch = iga.assemblers.DevicePatch(kvs, geo, row0=(lo, hi))
        parts.append(patch.csr('stiffness', algo='sumfact'))
        assert patch.last_path() == BF3
        patch.close()
    V = scipy.sparse.vstack(parts).tocsr()
    assert np.array_equal(V.indptr, A.indptr) and np.array_equal(V.indices, A.indices) and np.array_equal(V.data, A.data)


def test_chains_that_keep_every_slice(iga, monkeypatch):
    """Patches whose K1 has another reader, or another writer: the skip is off for them -- same bits, same path either way.  Degree
    6 and repeated knots on both the mid and the last axis leave the fused chain; IGX_BF=2 is k_bf2 + the mirror pass; degree 5 stays
    on k_geoA -> k_bf3 but its axis-0 sweep does not form one product per pair (geoA_diag_types_commute)."""
    mk = iga.bspline.make_knots
    geo = _geo(iga, 'cylinder')
    both = (mk(3, 0., 1., 4), kv_mults(iga, 3, [1, 2, 1]), kv_mults(iga, 3, [2, 1, 1, 2]))
    for kvs in ((mk(6, 0., 1., 2), mk(6, 0., 1., 3), mk(6, 0., 1., 2)), both):
        check_stiffness(iga, monkeypatch, kvs, geo)                    # (same path with and without the knob: checked there)
        patch = iga.assemblers.DevicePatch(kvs, geo)
        patch.csr('stiffness', algo='sumfact')
        assert 'bf3' not in patch.last_path() and 'fused' not in patch.last_path(), patch.last_path()
        patch.close()
    check_stiffness(iga, monkeypatch, (mk(5, 0., 1., 3), mk(5, 0., 1., 4), mk(5, 0., 1., 5)), geo, BF3)
    monkeypatch.setenv('IGX_BF', '2')
    kvs = (mk(3, 0., 1., 5), mk(3, 0., 1., 9), mk(3, 0., 1., 30))
    B2 = check_stiffness(iga, monkeypatch, kvs, geo, {'geoA', 'fused', 'mirror'})
    monkeypatch.delenv('IGX_BF')
    B3 = check_stiffness(iga, monkeypatch, kvs, geo, BF3, entrywise=False)
    assert np.array_equal(B2.data, B3.data)               # (test_both_triangles_from_the_fused_stage: the two chains agree bit for bit)


def test_other_forms(iga, monkeypatch):
    """Mass, the convection-diffusion form and a symmetric coefficient table: nothing of theirs is skipped."""
    mk = iga.bspline.make_knots
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')
    geo = _geo(iga, 'cylinder')
    kv1, kv2 = two_tiles_two_chunks(iga, 3, 3, 4)
    kvs = (mk(3, 0., 1., 4), kv1, kv2)
    runs = [('mass', lambda: iga.assemblers.DevicePatch(kvs, geo), lambda pt: pt.csr('mass', algo='sumfact'), {'geoA', 'fused', 'both', 'bf3'}),
            ('convdiff', lambda: iga.assemblers.ConvDiffAssembler3D(kvs, geo, iga.assemblers.AffineCoefficient(1.5, 0.2, -0.1, 0.3)),
             lambda asm: asm.assemble_csr(algo='sumfact'), {'geoA', 'fused', 'bf3'}),
            ('table', lambda: iga.assemblers.GeneralFormAssembler3D(kvs, geo, '(2 * inner(grad(u), grad(v)) + 3 * u * v) * dx'),
             lambda asm: asm.assemble_csr(algo='sumfact'), {'geoA', 'fused', 'both', 'bf3'})]
    for name, make, run, path in runs:
        (A, pa), (B, pb) = both_ways(monkeypatch, make, run)
        assert pa == pb == path, (name, pa, pb)
        assert not np.isnan(A.data).any(), name
        assert np.array_equal(A.indices, B.indices) and np.array_equal(A.data, B.data), name

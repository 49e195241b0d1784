"""The multigrid and DIRK kernels and the cases that run them cannot drift apart (no GPU needed).

pyiga_amd/csrc/multigrid.hip maps the group width of the sweep kernels to one instantiation of k_csr_gs / k_csr_gs_block per width
in with_gs_kernel, loops over the rows of a colour with a grid of at most NB_GS_MAX blocks, and k_mg_transfer carries a dof count
and a band width per axis; solve_step.hip's k_dirk_rhs holds at most COMB_MAX vectors.  tests/_mg_cases.py restates all of it, and
tests/test_mg_kernels_gpu.py and tests/test_parabolic_gpu.py run its cases.  A new width, a changed batch, a dropped case line, a
larger grid constant, more DIRK stages or a transfer case that became isotropic fails here: the tables must then be extended so that
every instantiation and every loop still runs under a test that would notice a mistake in it."""
import numpy as np
import pytest

from pyiga_amd import solvers

import _mg_cases as mc
import _mg_model as G
import _solver_cases as sc


@pytest.fixture(scope='module')
def src():
    return mc.read_source()


def test_constants(src):
    assert mc.parse_constants(src) == {'BLOCK': mc.BLOCK, 'NB_GS_MAX': mc.NB_GS_MAX, 'BLOCK_ONE': mc.BLOCK_ONE}
    assert [mc.gs_pass_rows(g) for g in sc.GWS] == [524288, 262144, 131072, 65536, 32768]
    assert all(mc.BLOCK_ONE % g == 0 and mc.BLOCK % g == 0 for g in sc.GWS)


def test_gs_dispatch_case_lines(src):
    """Every width has a case line in with_gs_kernel that names both kernels at that width and one batch; the label is the width
    (the default: GW 4); the instantiations are those of the CSR SpMV, as the header comment of the table says."""
    d = mc.parse_gs_dispatch(src)
    assert d['k_csr_gs'] == d['k_csr_gs_block'], d
    lines = d['k_csr_gs']
    assert len(lines) == len(sc.GWS), sorted(lines, key=str)
    assert {(gw, u) for _, gw, u in lines} == mc.GS_INSTANCES, sorted(lines, key=str)
    for label, gw, _ in lines:
        assert label == gw or (label is None and gw == 4), (label, gw)
    assert mc.GS_INSTANCES == sc.CSR_SPMV_INSTANCES
    assert {(gw, u) for _, gw, u in sc.parse_dispatch(sc.read_source())['k_csr_spmv']} == mc.GS_INSTANCES


def test_no_gs_instance_outside_the_table(src):
    assert mc.gs_instances_outside_table(src) == []


def _colouring(MP, sides):
    S = sc.multipatch_pattern(MP)
    free = np.ones(MP.numdofs, dtype=bool)
    free[mc.fixed_dofs(MP, sides)] = False
    colour, nc = solvers.first_fit_colouring(S.indptr, S.indices, free)
    return S, colour, nc


def test_gs_cases_reach_every_width():
    ids = [c.id for c in mc.GS_CASES]
    assert len(set(ids)) == len(ids)
    strided = set()
    for c in mc.GS_CASES:
        assert c.n % 2 == 0                                   # coarsened once
        MP = c.build()
        S, colour, nc = _colouring(MP, c.sides)
        assert sc.spmv_gw(sc.max_row(S)) == c.gw, (c.id, sc.max_row(S), c.gw)
        assert nc == c.colours, (c.id, nc)
        assert np.array_equal(colour, G.first_fit(S.indptr, S.indices, colour >= 0)), c.id
        if max(len(r) for r in mc.colour_lists(colour)) > mc.BLOCK_ONE // c.gw:
            strided.add(c.gw)
        assert c.distance <= mc.RELAX_BOUND / 4
    assert {c.gw for c in mc.GS_CASES} == set(sc.GWS)
    # at every width the one-block sweep strides over a colour of more rows than it has row groups
    assert strided == set(sc.GWS), sorted(strided)
    # GW 64 by both routes: 3D p = 3 and 2D p = 7
    assert {len(c.build().patches[0][0]) for c in mc.GS_CASES if c.gw == 64} == {2, 3}


def test_big_case_takes_a_second_pass_of_the_colour_grid():
    c = mc.GS_BIG_CASE
    MP = c.build()
    S, colour, nc = _colouring(MP, c.sides)
    assert sc.spmv_gw(sc.max_row(S)) == c.gw == 4
    largest = max(len(r) for r in mc.colour_lists(colour))
    print(c.id, 'dofs', MP.numdofs, 'nonzeros', S.nnz, 'colours', nc, 'largest colour', largest, 'one pass', mc.gs_pass_rows(c.gw))
    assert nc == c.colours
    assert largest > mc.gs_pass_rows(c.gw), (largest, mc.gs_pass_rows(c.gw))
    assert c.distance <= mc.RELAX_BOUND / 4


def _level_pairs(case):
    MPs = case.hierarchy()
    assert len(MPs) == case.levels
    return list(zip(MPs[:-1], MPs[1:]))


@pytest.mark.parametrize('case', mc.TRANSFER_CASES, ids=[c.id for c in mc.TRANSFER_CASES])
def test_transfer_cases_are_anisotropic(case):
    """Per patch and level pair: pairwise distinct dof counts per axis on both levels, pairwise distinct band widths per axis in
    both directions (a 2D patch counts its one-dof outer axis of width 1), and each of the three swaps changes what the
    restatement of k_mg_transfer returns while the restatement itself is the Kronecker product."""
    rng = np.random.default_rng(3)
    for F, Cs in _level_pairs(case):
        assert F.injective and Cs.injective and not F.bare_joins
        for (kf, _), (kc, _) in zip(F.patches, Cs.patches):
            Ps = mc.axis_prolongations(kc, kf)
            pad = [1] * (3 - len(kf))
            for kvs in (kf, kc):
                N = pad + [kv.numdofs for kv in kvs]
                assert len(set(N)) == 3, (case.id, N)
            for transposed in (False, True):
                w = pad + [mc.make_band(P, transposed)[2] for P in Ps]
                assert len(set(w)) == 3, (case.id, transposed, w)
                Pk = G.patch_prolongation(kc, kf)
                Pk = Pk.T if transposed else Pk
                x = rng.standard_normal(Pk.shape[1])
                ref = Pk @ x
                y = mc.transfer_restated(Ps, x, transposed)
                assert abs(y - ref).max() <= 1e-14 * abs(ref).max(), (case.id, transposed)
                for swap in ('No', 'Ni', 'w'):
                    z = mc.transfer_restated(Ps, x, transposed, swap=swap)
                    assert abs(z - ref).max() > 1e-3 * abs(ref).max(), (case.id, transposed, swap)
    assert case.distance <= mc.TRANSFER_BOUND / 4


def test_transfer_cases_cover_what_they_name():
    tags = set().union(*[c.tags for c in mc.TRANSFER_CASES])
    assert tags >= {'3d', 'repeated', 'graded', 'flipped', 'three_level'}
    for c in mc.TRANSFER_CASES:
        MP = c.make()
        kvs = [kv for ks, _ in MP.patches for kv in ks]
        assert ('3d' in c.tags) == (len(MP.patches[0][0]) == 3), c.id
        repeated = any((np.unique(kv.kv[kv.p + 1:-kv.p - 1], return_counts=True)[1] > 1).any() for kv in kvs)
        assert ('repeated' in c.tags) == repeated, c.id
        graded = any(np.ptp(np.diff(kv.mesh)) > 1e-3 for kv in kvs)
        assert ('graded' in c.tags) == graded, c.id
        flipped = any(j[4] is not None and any(j[4]) for j in MP.boundary_joins)
        assert ('flipped' in c.tags) == flipped, c.id
        assert ('three_level' in c.tags) == (c.levels >= 3), c.id
        # the fixed sides are whole sides, found again as such on every level
        for L in c.hierarchy():
            fixed = mc.fixed_dofs(L, c.sides)
            maps = [L.patch_to_global_idx(q) for q in range(L.numpatches)]
            assert np.array_equal(G.side_dofs(L, solvers.fixed_sides([k for k, _ in L.patches], maps, fixed)), fixed), c.id
    # the band widths of the graded case vary along an axis: make_band clamps the first column and pads with zeros
    c = next(c for c in mc.TRANSFER_CASES if 'graded' in c.tags)
    F, Cs = _level_pairs(c)[0]
    varied = False
    for P in mc.axis_prolongations(Cs.patches[0][0], F.patches[0][0]):
        lo, v, w = mc.make_band(P)
        inner = [np.flatnonzero(row) for row in P[1:-1]]
        varied |= len({int(nz[-1] - nz[0]) for nz in inner}) > 1 and (v[1:-1] == 0).any()
    assert varied


def test_dense_cases_sizes():
    for c in mc.DENSE_CASES:
        MP = c.build()
        m = MP.numdofs - mc.fixed_dofs(MP, c.sides).size
        assert c.lo < m <= c.hi and m % mc.BLOCK != 0, (c.id, m)
    ranges = [(c.lo, c.hi) for c in mc.DENSE_CASES]
    assert ranges == [(0, 255), (256, 511), (1500, 8192)]


def test_dirk_bound_and_full_tableaux():
    solve_src = sc.read_source()
    with open(mc.IGX_H) as f:
        header = f.read()
    from pyiga_amd import _lib
    k = mc.parse_dirk_constants(solve_src, header)
    assert k == {'COMB_MAX': mc.COMB_MAX, 'AXPBY_U': mc.AXPBY_U, 'IGX_DIRK_MAX_STAGES': mc.DIRK_MAX_STAGES}
    assert _lib.IGX_DIRK_MAX_STAGES == mc.DIRK_MAX_STAGES
    # M x, one F_j per earlier stage, f: a stage combines at most stages + 1 vectors
    assert k['IGX_DIRK_MAX_STAGES'] + 1 <= k['COMB_MAX']
    tabs = mc.dirk6_tableaux()
    assert set(tabs) == {'sdirk6', 'esdirk6'}
    for name, A in tabs.items():
        B, gamma = solvers.check_tableau(A)
        s = mc.DIRK_MAX_STAGES
        assert B.shape == (s + 1, s) and gamma > 0
        assert np.count_nonzero(B[s - 1, :s - 1]) == s - 1 == 5
        assert (B[:s][np.tril_indices(s, -1)] != 0).all()
        assert (B[0, 0] == 0) == (name == 'esdirk6')
        assert 1 + np.count_nonzero(B[s - 1, :s - 1]) + 1 == 7 <= mc.COMB_MAX
    with pytest.raises(ValueError):
        solvers.check_tableau(np.zeros((s + 2, s + 1)))

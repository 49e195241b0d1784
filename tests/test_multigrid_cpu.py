"""Geometric multigrid for multipatch systems, the parts that need no GPU: the host spline pieces against the reference
(tests/golden/golden_multigrid.npz, made by tests/golden/make_golden_multigrid.py), knot coarsening, the first-fit colouring of
the library against its Python restatement, the recorded joins, the whole-side check, and the numpy model of the method
(tests/_mg_model.py) on the oracle's matrices: a symmetric V-cycle, a prolongation that is a partition of unity and single-valued
on shared dofs, and PCG iteration counts that do not grow with the refinement."""
import numpy as np
import pytest
import scipy.sparse

from pyiga_amd import assemble, bspline, solvers

import _mg_model as G
import _mpsolve_model as M

LSHAPE_SIDES = [(0, 'left'), (0, 'bottom'), (1, 'bottom'), (1, 'right'), (2, 'top')]


def _spline_cases(g):
    return [str(s) for s in g['spline_cases']]


def test_refine_knot_insertion_prolongation_match_reference(golden):
    g = golden('multigrid')
    names = _spline_cases(g)
    assert len(names) == 9 and {n[:5] for n in names} == {'kv_p%d' % p for p in range(1, 6)}
    for name in names:
        p = int(name[4])
        kv = bspline.KnotVector(g[name + '_kv'], p)
        fine = kv.refine()
        assert np.array_equal(fine.kv, g[name + '_refined']), name
        assert np.array_equal(kv.refine([0.1, 0.55, 0.55]).kv, g[name + '_refined_at']), name
        for k, u in enumerate(g[name + '_ins_u']):
            T = bspline.knot_insertion(kv, float(u))
            assert scipy.sparse.isspmatrix_csr(T) and T.shape == (kv.numdofs + 1, kv.numdofs)
            assert abs(T.toarray() - g[name + '_ins%d' % k]).max() <= 1e-13, (name, u)
        P = bspline.prolongation(kv, fine)
        assert scipy.sparse.isspmatrix_csr(P)
        assert abs(P.toarray() - g[name + '_P']).max() <= 1e-13, name
        assert abs(bspline.prolongation(kv, fine.refine()).toarray() - g[name + '_P2']).max() <= 1e-13, name
        assert (abs(P.data) >= 1e-15).all()


def test_prolongation_reproduces_a_spline(oracle):
    rng = np.random.default_rng(5)
    x = np.linspace(0.0, 1.0, 50)
    for p in range(1, 6):
        for mult in (1, 2):
            if mult > p:
                continue
            kc = bspline.make_knots(p, 0.0, 1.0, 6, mult=mult)
            kf = kc.refine()
            c = rng.standard_normal(kc.numdofs)
            Bc = np.asarray(oracle.collocation_derivs_dense(oracle.KnotVector(kc.kv, p), x, 0))[0]
            Bf = np.asarray(oracle.collocation_derivs_dense(oracle.KnotVector(kf.kv, p), x, 0))[0]
            assert abs(Bf @ (bspline.prolongation(kc, kf) @ c) - Bc @ c).max() <= 1e-13, (p, mult)


def test_coarsen_knots():
    for p in range(1, 5):
        for mult in (1, 2):
            if mult > p:
                continue
            kv = bspline.make_knots(p, 0.0, 1.0, 6, mult=mult)
            assert solvers.coarsen_knots(kv.refine()) == kv
            assert np.array_equal(solvers.coarsen_knots(kv.refine()).kv, kv.kv)
    kv = bspline.make_knots(3, 0.0, 1.0, 8)
    assert solvers.coarsen_knots(kv).numspans == 4 and solvers.coarsen_knots(solvers.coarsen_knots(kv)).numspans == 2
    # the coarse space is nested in the fine one: the prolongation exists and is a partition of unity
    P = bspline.prolongation(solvers.coarsen_knots(kv), kv)
    assert abs(P @ np.ones(P.shape[1]) - 1).max() <= 1e-14
    for n in (1, 3, 7):
        with pytest.raises(ValueError):
            solvers.coarsen_knots(bspline.make_knots(2, 0.0, 1.0, n))


def test_prolongation_refusals():
    kv = bspline.make_knots(2, 0.0, 1.0, 4)
    with pytest.raises(ValueError):
        bspline.prolongation(kv, bspline.make_knots(3, 0.0, 1.0, 8))        # another degree
    with pytest.raises(ValueError):
        bspline.prolongation(kv.refine(), kv)                                # not nested
    with pytest.raises(ValueError):
        bspline.prolongation(kv, bspline.make_knots(2, 0.0, 1.0, 5))         # other knots
    with pytest.raises(ValueError):
        bspline.knot_insertion(kv, 1.5)


def test_joins_are_recorded_and_replayed():
    MP = M.notebook(p=3, n=8)
    assert MP.boundary_joins == [(0, (0, 1), 1, (1, 1), (False,)), (1, (1, 0), 2, (0, 1), (True,)), (1, (0, 0), 3, (0, 1), (False,))]
    assert not MP.bare_joins
    MPc = G.coarsen(MP)
    ref = M.notebook(p=3, n=4)
    assert MPc.numdofs == ref.numdofs
    for p in range(4):
        assert np.array_equal(MPc.patch_to_global_idx(p), ref.patch_to_global_idx(p))
    kvs = 2 * (bspline.make_knots(2, 0.0, 1.0, 4),)
    from pyiga_amd import geometry
    MPb = assemble.Multipatch([(kvs, geometry.unit_square()), (kvs, geometry.unit_square().translate((1, 0)))])
    MPb.join_dofs(0, assemble.boundary_dofs(kvs, 'right', ravel=True), 1, assemble.boundary_dofs(kvs, 'left', ravel=True))
    MPb.finalize()
    assert MPb.bare_joins
    with pytest.raises(ValueError):
        MPb.replay_joins(MPb.patches)


def test_fixed_sides():
    MP = M.notebook(p=3, n=8)
    shapes, maps = M.shapes_maps(MP)
    kvs = [k for k, _ in MP.patches]
    fixed = M.fixed_dofs(MP, M.NOTEBOOK_DIRICHLET)
    sides = solvers.fixed_sides(kvs, maps, fixed)
    assert np.array_equal(G.side_dofs(MP, sides), fixed)
    # the same sides on the coarse space are the coarse domain's Dirichlet dofs
    MPc = G.coarsen(MP)
    assert np.array_equal(G.side_dofs(MPc, sides), M.fixed_dofs(MPc, M.NOTEBOOK_DIRICHLET))
    with pytest.raises(ValueError) as e:
        solvers.fixed_sides(kvs, maps, fixed[:-1])
    assert 'dof' in str(e.value)
    part = MP.patch_to_global_idx(1)[assemble.boundary_dofs(kvs[1], 'top', ravel=True)[:4]]
    with pytest.raises(ValueError) as e:
        solvers.fixed_sides(kvs, maps, part)
    assert 'dof %d' % part.min() in str(e.value)


def _pattern(MP):
    """The global pattern from the patches' tensor-product patterns (host)."""
    S = None
    for p in range(MP.numpatches):
        kvs = MP.patches[p][0]
        B = None
        for kv in kvs:
            ms = kv.mesh_support_idx_all()
            b = scipy.sparse.csr_matrix(((ms[:, None, 0] < ms[None, :, 1]) & (ms[None, :, 0] < ms[:, None, 1])).astype(float))
            B = b if B is None else scipy.sparse.kron(B, b, format='csr')
        X = MP.patch_to_global(p)
        T = X @ B @ X.T
        S = T if S is None else S + T
    S = scipy.sparse.csr_matrix(S)
    S.sort_indices()
    return S


@pytest.mark.parametrize('case', ['notebook_p3', 'lshape_p2', 'lshape_p3_all_free'])
def test_library_colouring_equals_restatement_and_is_valid(case):
    if case == 'notebook_p3':
        MP = M.notebook(p=3, n=8)
        fixed = M.fixed_dofs(MP, M.NOTEBOOK_DIRICHLET)
    elif case == 'lshape_p2':
        MP = M.lshape(p=2, n=8)
        fixed = M.fixed_dofs(MP, LSHAPE_SIDES)
    else:
        MP = M.lshape(p=3, n=4)
        fixed = np.zeros(0, dtype=np.int64)
    S = _pattern(MP)
    free = np.ones(MP.numdofs, dtype=bool)
    free[fixed] = False
    colour, nc = solvers.first_fit_colouring(S.indptr, S.indices, free if fixed.size else None)
    assert np.array_equal(colour, G.first_fit(S.indptr, S.indices, free))
    assert (colour[free] >= 0).all() and (colour[~free] == -1).all()
    assert nc == colour.max() + 1 <= np.diff(S.indptr).max()
    # valid: no free row has a free neighbour of its own colour
    C = S.tocoo()
    off = (C.row != C.col) & free[C.row] & free[C.col]
    assert not (colour[C.row[off]] == colour[C.col[off]]).any()


def test_golden_colour_order_is_the_restatement(golden):
    g = golden('multigrid')
    for name in [str(s) for s in g['domain_cases']]:
        n = g[name + '_indptr'].size - 1
        free = np.ones(n, dtype=bool)
        free[g[name + '_bc_idx']] = False
        colour, _ = solvers.first_fit_colouring(g[name + '_indptr'], g[name + '_indices'], free)
        assert np.array_equal(G.colour_order(colour), g[name + '_order']), name
        # and the model's sweep is the reference's
        A = scipy.sparse.csr_matrix((g[name + '_data'], g[name + '_indices'], g[name + '_indptr']), shape=(n, n))
        for sweep in ('forward', 'backward', 'symmetric'):
            x = G.gauss_seidel(A, g[name + '_x0'], g[name + '_b'], g[name + '_order'], sweep)
            ref = g[name + '_gs_' + sweep]
            assert abs(x - ref).max() <= 1e-13 * abs(ref).max(), (name, sweep)


def _geos(oracle, which):
    if which == 'notebook':
        return [oracle.geo_quarter_annulus(), oracle.geo_unit_cube(2), oracle.geo_quarter_annulus(), oracle.geo_quarter_annulus()]
    return 3 * [oracle.geo_unit_cube(2)]


@pytest.mark.parametrize('which', ['notebook', 'lshape'])
def test_global_prolongation_is_a_partition_of_unity_and_single_valued(which):
    MPf, MPc = (M.notebook(p=3, n=8), M.notebook(p=3, n=4)) if which == 'notebook' else (M.lshape(p=2, n=8), M.lshape(p=2, n=4))
    assert any(j[4] is not None and any(j[4]) for j in MPf.boundary_joins)            # a flipped join
    P, terms, mult = G.global_prolongation(MPf, MPc)
    assert abs(P @ np.ones(MPc.numdofs) - 1).max() <= 1e-13
    xc = np.random.default_rng(1).standard_normal(MPc.numdofs)
    for p in range(MPf.numpatches):
        Xf, Xc = MPf.patch_to_global(p), MPc.patch_to_global(p)
        own = G.patch_prolongation(MPc.patches[p][0], MPf.patches[p][0]) @ (Xc.T @ xc)
        assert abs(own - Xf.T @ (P @ xc)).max() <= 1e-13, p


@pytest.mark.parametrize('which,p', [('notebook', 3), ('lshape', 2)])
def test_model_vcycle_is_symmetric(which, p, oracle):
    make, sides = (M.notebook, M.NOTEBOOK_DIRICHLET) if which == 'notebook' else (M.lshape, LSHAPE_SIDES)
    model = G.Model(*G.oracle_levels(oracle, make, _geos(oracle, which), p, 16, 3, sides))
    n = model.levels[0]['fr'].size
    rng = np.random.default_rng(2)
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    a, b = model.vcycle(x) @ y, x @ model.vcycle(y)
    assert abs(a - b) <= 1e-12 * abs(a), (a, b)
    assert x @ model.vcycle(x) > 0


@pytest.mark.parametrize('which,p', [('notebook', 3), ('lshape', 2)])
def test_model_iterations_do_not_grow_with_refinement(which, p, oracle):
    """PCG with V(1,1) on a random right-hand side (seed 0, tol 1e-8, as test_schwarz_halves_jacobi_iterations_in_the_model), the
    coarsest level of 4 spans per patch: the counts at n = 16 and 32 are within 2 of each other and at n = 32 at most half of
    Jacobi's."""
    make, sides = (M.notebook, M.NOTEBOOK_DIRICHLET) if which == 'notebook' else (M.lshape, LSHAPE_SIDES)
    its = {}
    for n, nlev in ((16, 3), (32, 4)):
        model = G.Model(*G.oracle_levels(oracle, make, _geos(oracle, which), p, n, nlev, sides))
        A = model.levels[0]['Af']
        b = np.random.default_rng(0).standard_normal(A.shape[0])
        x, its[n] = G.pcg(A, b, model.vcycle, 1e-8)
        assert np.linalg.norm(A @ x - b) <= 1e-7 * np.linalg.norm(b)
    d = A.diagonal()
    _, it_j = G.pcg(A, b, lambda r: r / d, 1e-8)
    print('model iterations', which, p, its, 'jacobi at n = 32:', it_j)
    assert abs(its[16] - its[32]) <= 2, its
    assert 2 * its[32] <= it_j, (its, it_j)


def test_new_abi_names_and_preconditioner_table():
    from pyiga_amd import _lib
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for name in ('igx_csr_colouring', 'igx_solver_set_mg_smoother', 'igx_solver_set_mg_coarse', 'igx_solver_set_mg_inverse',
                 'igx_solver_mg_info', 'igx_solver_mg_colours', 'igx_solver_mg_relax_d', 'igx_solver_mg_prolong_d',
                 'igx_solver_mg_restrict_d'):
        assert name in bound, name
    assert _lib.IGX_PRECOND_MG == 4 and _lib.MP_PRECONDS['mg'] == 4 and 'mg' not in _lib.PRECONDS
    assert 'mg' in solvers.MultipatchSystem.PRECONDS and 'mg' not in solvers.PatchSystem.PRECONDS

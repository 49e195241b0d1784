"""Geometric multigrid for multipatch systems on the device (MultipatchSystem.solve(precond='mg'), igx_solver_set_mg_*,
pyiga_amd/csrc/multigrid.hip): the coloured Gauss-Seidel sweeps against the reference's gauss_seidel (golden_multigrid.npz), the
transfers against the model's sparse prolongation, the V-cycle against the numpy model on the downloaded matrices of every level,
solutions against the reference's direct solution, iteration counts against the model and against Jacobi and Schwarz, a size past
one SpMV grid, determinism and the refusals.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

from pyiga_amd import _lib, assemble, bspline, geometry, solvers

import _mg_model as G
import _mpsolve_model as M

pytestmark = pytest.mark.gpu

STIFF = 'inner(grad(u),grad(v))*dx'
LSHAPE_DIRICHLET = [(0, 'left'), (0, 'bottom'), (2, 'top')]


def f2(x, y):
    return np.exp(-5 * ((x - 0.3) ** 2 + (y - 1) ** 2))


def g2(x, y):
    return 1e-1 * np.sin(8 * x)


def f3(x, y, z):
    return 1.0 + x * y - z


def g3(x, y, z):
    return x + 0.5 * y * z


def _domain(name):
    """(MP, f, bcs) of a golden case name such as 'lshape_p2_n8', or of 'cubes_p2_n4'."""
    which, p, n = name.split('_')
    p, n = int(p[1:]), int(n[1:])
    if which == 'cubes':
        MP = M.three_cubes(p=p, n=n)
        return MP, f3, MP.compute_dirichlet_bcs([(0, (0, 0), g3), (2, (2, 1), g3)])
    MP, sides = (M.notebook(p=p, n=n), M.NOTEBOOK_DIRICHLET) if which == 'notebook' else (M.lshape(p=p, n=n), LSHAPE_DIRICHLET)
    return MP, f2, MP.compute_dirichlet_bcs([(q, bd, g2) for q, bd in sides])


def _system(name, **mg):
    MP, f, bcs = _domain(name)
    S = solvers.MultipatchSystem(MP, STIFF, 'f*v*dx', bcs=bcs, f=f)
    if mg:
        S.set_multigrid(**mg)
    return S, bcs


def _model(S):
    """The numpy model on the downloaded device matrices of every level of S's hierarchy."""
    levels = [S.mg_level(l) for l in range(len(S.mg_info()))]
    return G.Model([L.matrix() for L in levels], [L.MP for L in levels], [L.bc_indices for L in levels],
                   smooth_steps=S._mg['smooth_steps'])


def _relmax(a, b):
    return abs(a - b).max() / abs(b).max()


GOLDEN_CASES = ['lshape_p2_n8', 'lshape_p3_n8', 'notebook_p3_n8']
PATHS = {'per_colour': 0, 'one_block': 1 << 30}


@pytest.mark.parametrize('path', sorted(PATHS))
@pytest.mark.parametrize('name', GOLDEN_CASES)
def test_relax_matches_the_reference(name, path, golden):
    """One sweep of each kind from the golden start vector against the reference's gauss_seidel(A, x, b, indices=order, sweep=)
    on the reference's matrix, through the per-colour kernel and through the one-block kernel."""
    g = golden('multigrid')
    S, bcs = _system(name, levels=2, block_rows=PATHS[path])
    try:
        assert np.array_equal(bcs[0], g[name + '_bc_idx'])
        info = S.mg_info()
        assert info[0]['one_block'] == (path == 'one_block')
        assert np.array_equal(S.mg_colour_order(0), g[name + '_order'])
        for sweep in ('forward', 'backward', 'symmetric'):
            x = S.relax(g[name + '_x0'], g[name + '_b'], sweep=sweep)
            ref = g[name + '_gs_' + sweep]
            print('relax', name, path, sweep, 'rel. difference %.2e' % _relmax(x, ref), 'colours', info[0]['colours'])
            assert _relmax(x, ref) <= 1e-12, (name, path, sweep)
            assert not x[bcs[0]].any()
        # the coarse level's sweeps and two iterations, against the model on the downloaded matrix
        L1 = S.mg_level(1)
        A1 = L1.matrix()
        rng = np.random.default_rng(11)
        x0, b1 = rng.standard_normal(L1.n), rng.standard_normal(L1.n)
        x0[L1.bc_indices] = 0
        order = S.mg_colour_order(1)
        ref = G.gauss_seidel(A1, G.gauss_seidel(A1, x0, b1, order, 'symmetric'), b1, order, 'symmetric')
        x = S.relax(x0, b1, sweep='symmetric', iterations=2, level=1)
        print('relax level 1', name, path, 'rel. difference %.2e' % _relmax(x, ref))
        assert _relmax(x, ref) <= 1e-12
    finally:
        S.close()


@pytest.mark.parametrize('name', ['notebook_p3_n8', 'lshape_p2_n8', 'cubes_p2_n4'])
def test_transfers_match_the_model(name):
    S, bcs = _system(name, levels=2)
    try:
        F, Cs = S.mg_level(0), S.mg_level(1)
        if name.startswith('notebook'):
            assert any(j[4] is not None and any(j[4]) for j in F.MP.boundary_joins)        # a flipped join
        Pfull, _, _ = G.global_prolongation(F.MP, Cs.MP)
        ff = np.ones(F.n)
        ff[F.bc_indices] = 0
        fc = np.ones(Cs.n)
        fc[Cs.bc_indices] = 0
        rng = np.random.default_rng(12)
        xc, rf = rng.standard_normal(Cs.n), rng.standard_normal(F.n)
        ref = ff * (Pfull @ (fc * xc))
        y = S.prolong(xc, 0)
        print('prolong', name, 'rel. difference %.2e' % _relmax(y, ref))
        assert _relmax(y, ref) <= 1e-13
        ref = fc * (Pfull.T @ (ff * rf))
        y = S.restrict(rf, 0)
        print('restrict', name, 'rel. difference %.2e' % _relmax(y, ref))
        assert _relmax(y, ref) <= 1e-13
        assert not y[Cs.bc_indices].any()
    finally:
        S.close()


@pytest.mark.parametrize('path', sorted(PATHS))
@pytest.mark.parametrize('name,levels,steps', [('notebook_p3_n16', 3, 1), ('lshape_p2_n16', 3, 2), ('cubes_p2_n8', 2, 1)])
def test_vcycle_matches_the_model_and_is_symmetric(name, levels, steps, path):
    S, bcs = _system(name, levels=levels, smooth_steps=steps, block_rows=PATHS[path])
    try:
        assert len(S.mg_info()) == levels
        model = _model(S)
        rng = np.random.default_rng(13)
        x, y = rng.standard_normal(S.n), rng.standard_normal(S.n)
        Bx, By = S.apply_precond(x, 'mg'), S.apply_precond(y)
        ref = model.apply_full(x)
        print('V-cycle', name, path, 'rel. difference to the model %.2e' % _relmax(Bx, ref))
        assert _relmax(Bx, ref) <= 1e-10
        assert not Bx[bcs[0]].any()
        free = np.ones(S.n, dtype=bool)
        free[bcs[0]] = False
        a, b = Bx[free] @ y[free], x[free] @ By[free]
        print('V-cycle', name, path, 'symmetry %.2e' % (abs(a - b) / abs(a)))
        assert abs(a - b) <= 1e-11 * abs(a)
    finally:
        S.close()


@pytest.mark.parametrize('name', GOLDEN_CASES)
def test_solution_matches_the_reference_and_iterations_the_model(name, golden):
    g = golden('multigrid')
    S, bcs = _system(name, levels=2)
    try:
        u = S.solve(tol=1e-12, precond='mg')
        assert S.info['converged'] and S.info['precond'] == 'mg' and S.info['smooth_steps'] == 1 and S.info['levels'] == 2
        err = np.linalg.norm(u - g[name + '_u']) / np.linalg.norm(g[name + '_u'])
        print('solve', name, 'iterations to 1e-12:', S.info['iterations'], 'rel. error %.2e' % err)
        assert err <= 1e-8
        assert np.array_equal(u[bcs[0]], bcs[1])
        # iterations against the model on the same matrices; two solves are bit-identical
        u1 = S.solve(tol=1e-8, precond='mg')
        it = S.info['iterations']
        assert S.info['converged']
        u2 = S.solve(tol=1e-8, precond='mg')
        assert np.array_equal(u1, u2)
        RS = assemble.RestrictedLinearSystem(S.matrix(), S.rhs(), bcs)
        _, it_model = G.pcg(RS.A.tocsr(), RS.b, _model(S).vcycle, 1e-8)
        print('solve', name, 'iterations to 1e-8:', it, 'model', it_model)
        assert abs(it - it_model) <= 2
    finally:
        S.close()
    # the default hierarchy of so small a system is its dense inverse alone
    S, bcs = _system(name)
    try:
        u = S.solve(tol=1e-12, precond='mg')
        assert S.info['converged'] and S.info['levels'] == 1 and S.info['iterations'] <= 2
        assert np.linalg.norm(u - g[name + '_u']) <= 1e-8 * np.linalg.norm(g[name + '_u'])
    finally:
        S.close()


def test_iterations_do_not_grow_with_refinement_on_the_notebook_domain():
    """p = 3, the right-hand side and Dirichlet data of test_schwarz_halves_jacobi_on_notebook_n64_and_matches_model: the device's
    counts follow the model's at n = 16, 32, 64; at n = 64 at most a quarter of Jacobi's and half of Schwarz's."""
    its = {}
    for n in (16, 32, 64):
        S, bcs = _system('notebook_p3_n%d' % n, coarse_max=200)      # (down to 4 spans per patch: 3, 4 and 5 levels)
        try:
            assert S.mg_info()[-1]['spans'][0] == (4, 4) and len(S.mg_info()) == {16: 3, 32: 4, 64: 5}[n]
            S.solve(tol=1e-8, precond='mg')
            assert S.info['converged']
            it = S.info['iterations']
            RS = assemble.RestrictedLinearSystem(S.matrix(), S.rhs(), bcs)
            _, it_model = G.pcg(RS.A.tocsr(), RS.b, _model(S).vcycle, 1e-8)
            its[n] = (it, it_model)
            print('notebook p = 3, n = %d: levels %d, colours %s, iterations %d, model %d'
                  % (n, S.info['levels'], [d['colours'] for d in S.mg_info()], it, it_model))
            assert abs(it - it_model) <= 2, (n, it, it_model)
            if n == 64:
                S.solve(tol=1e-8, precond='jacobi')
                it_j = S.info['iterations']
                S.solve(tol=1e-8, precond='schwarz')
                it_s = S.info['iterations']
                print('notebook p = 3, n = 64: jacobi %d, schwarz %d, mg %d' % (it_j, it_s, it))
                assert 4 * it <= it_j and 2 * it <= it_s, (it, it_j, it_s)
                S.solve(tol=1e-8, precond='mg')                     # and back: the hierarchy is kept
                assert S.info['iterations'] == it
        finally:
            S.close()


@pytest.mark.parametrize('name', ['cubes_p2_n32', 'notebook_p3_n256'])
def test_sizes_past_one_block_per_colour_and_one_spmv_grid(name):
    """3D with several blocks per colour, and a 2D system of more rows than one pass of the CSR SpMV's grid (131 072 at the
    group width 16 of p = 3): converged, and the residual recomputed on the host from the downloaded system."""
    S, bcs = _system(name)
    try:
        u = S.solve(tol=1e-10, precond='mg')
        info = S.mg_info()
        assert S.info['converged'] and not info[0]['one_block'] and info[-1]['dense_inverse']
        if name.startswith('notebook'):
            assert S.n > 131072
        rows_per_colour = info[0]['free'] / info[0]['colours']
        assert rows_per_colour > 256
        RS = assemble.RestrictedLinearSystem(S.matrix(), S.rhs(), bcs)
        free = np.ones(S.n, dtype=bool)
        free[bcs[0]] = False
        res = np.linalg.norm(RS.A @ u[free] - RS.b) / np.linalg.norm(RS.b)
        print(name, 'dofs', S.n, 'levels', [(d['free'], d['colours'], d['one_block']) for d in info], 'iterations', S.info['iterations'],
              'host residual %.2e' % res)
        assert res <= 1e-8
    finally:
        S.close()


def test_refusals():
    MP, f, bcs = _domain('lshape_p2_n8')
    # fixed dofs that are not whole sides
    S = solvers.MultipatchSystem(MP, STIFF, 'f*v*dx', bcs=(bcs[0][:-1], bcs[1][:-1]), f=f)
    with pytest.raises(ValueError) as e:
        S.solve(precond='mg')
    assert 'whole patch sides' in str(e.value)
    S.close()
    # BiCGStab
    S = solvers.MultipatchSystem(MP, STIFF, 'f*v*dx', bcs=bcs, f=f, method='bicgstab')
    with pytest.raises(ValueError):
        S.solve(precond='mg')
    with pytest.raises(ValueError):
        S.set_multigrid()
    S.close()
    S = solvers.MultipatchSystem(MP, STIFF, 'f*v*dx', bcs=bcs, f=f)
    S.set_multigrid(levels=2)
    S.solve(precond='mg')
    assert S.info['levels'] == 2
    with pytest.raises(ValueError):
        S.set_method('bicgstab')
    assert _lib.load().igx_solver_set_method(S.handle, _lib.IGX_METHOD_BICGSTAB) == _lib.IGX_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        S.relax(np.zeros(S.n), level=7)
    with pytest.raises(ValueError):
        S.set_multigrid(levels=2, coarse_max=10)                    # the coarsest level would be too large
    assert S.solve(precond='mg').shape == (S.n,) and S.info['converged']       # (set up again with the defaults)
    S.set_multigrid(levels=2)
    # a solve after MP.assemble_system restarted the sums
    MP.assemble_system('u*v*dx', 'f*v*dx', f=f)
    with pytest.raises(_lib.IgxError) as e:
        S.solve(precond='mg')
    assert e.value.code == _lib.IGX_ERR_ARG and 'restarted' in str(e.value)
    # use after close()
    coarse = S.mg_level(1)
    S.close()
    assert coarse.handle is None and coarse.MP._handle is None
    with pytest.raises(_lib.IgxError):
        S.solve(precond='mg')
    with pytest.raises(_lib.IgxError):
        S.relax(np.zeros(MP.numdofs))
    # a coarse level whose sums were restarted
    S = solvers.MultipatchSystem(MP, STIFF, 'f*v*dx', bcs=bcs, f=f)
    S.set_multigrid(levels=2)
    S.mg_level(1).MP.assemble_system('u*v*dx', 'f*v*dx', f=f)
    with pytest.raises(_lib.IgxError) as e:
        S.solve(precond='mg')
    assert e.value.code == _lib.IGX_ERR_ARG
    S.close()


def test_profile_covers_every_level():
    S, bcs = _system('notebook_p3_n32', coarse_max=200)
    try:
        info = S.mg_info()
        pf = S.mg_profile(reps=2)
        print('profile', pf)
        assert pf['levels'] == len(info) == 4
        sweeps = sum(2 * (1 if d['one_block'] else d['colours']) for d in info[:-1])
        assert pf['launches'] == sweeps + (len(info) - 1) * (2 + 2 * 4) + 1
        assert all(t > 0 for t in pf['smooth_ms'][:-1]) and pf['coarse_ms'] > 0 and pf['total_ms'] > 0
    finally:
        S.close()


def test_bare_joins_need_explicit_coarse_multipatches():
    def joined(n, bare):
        kvs = 2 * (bspline.make_knots(2, 0.0, 1.0, n),)
        MP = assemble.Multipatch([(kvs, geometry.unit_square()), (kvs, geometry.unit_square().translate((1, 0)))])
        if bare:
            MP.join_dofs(0, assemble.boundary_dofs(kvs, 'right', ravel=True), 1, assemble.boundary_dofs(kvs, 'left', ravel=True))
        else:
            MP.join_boundaries(0, 'right', 1, 'left')
        MP.finalize()
        return MP
    MP = joined(8, True)
    bcs = MP.compute_dirichlet_bcs([(0, 'left', g2), (1, 'right', g2)])
    S = solvers.MultipatchSystem(MP, STIFF, 'f*v*dx', bcs=bcs, f=f2)
    try:
        with pytest.raises(ValueError) as e:
            S.set_multigrid(levels=2)
        assert 'join_dofs' in str(e.value)
        S.set_multigrid(coarse=[joined(4, True)])
        u = S.solve(tol=1e-10, precond='mg')
        assert S.info['converged'] and S.info['levels'] == 2
        S2 = solvers.MultipatchSystem(joined(8, False), STIFF, 'f*v*dx', bcs=bcs, f=f2)
        u2 = S2.solve(tol=1e-10, precond='mg')
        S2.close()
        assert np.linalg.norm(u - u2) <= 1e-8 * np.linalg.norm(u2)
    finally:
        S.close()


def test_non_injective_maps_are_refused():
    kvs = 2 * (bspline.make_knots(2, 0.0, 1.0, 4),)
    MP = assemble.Multipatch([(kvs, geometry.unit_square()), (kvs, geometry.unit_square().translate((1, 0)))])
    MP.join_dofs(0, [5], 1, [12])
    MP.join_dofs(1, [12], 0, [23])
    MP.finalize()
    assert not MP.injective
    bcs = MP.compute_dirichlet_bcs([(0, 'left', g2), (1, 'right', g2)])
    S = solvers.MultipatchSystem(MP, STIFF, 'f*v*dx', bcs=bcs, f=f2)
    try:
        with pytest.raises(ValueError):
            S.solve(precond='mg')
        assert S.solve(tol=1e-10, precond='jacobi').shape == (MP.numdofs,) and S.info['converged']
    finally:
        S.close()

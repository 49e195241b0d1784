"""MultipatchEigenSystem on the device: parity with the reference's multipatch matrices and dense eigh
(tests/golden/golden_mp_eig.npz), the L-shaped membrane, agreement with the host model of the controller and the V-cycle,
iteration growth, determinism and lifecycle."""
import numpy as np
import pytest
import scipy.sparse.linalg

import _eig_model as EM
import _mg_model as G
import _mp_eig_cases as MC
import _mpsolve_model as M

pytestmark = pytest.mark.gpu

STIFF, MASS = 'inner(grad(u), grad(v)) * dx', 'u * v * dx'


def host_matrices(MP):
    """(K, M) as ``MP.assemble_system`` returns them (before a system is made over MP: it restarts the sums)."""
    return MP.assemble_system(STIFF, None)[0].tocsr(), MP.assemble_system(MASS, None)[0].tocsr()


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name, k', [('lshape', 6), ('lshape', 12), ('notebook', 6), ('cubes2', 6)])
def test_golden_parity(golden, name, k):
    from pyiga_amd import solvers
    g = golden('mp_eig')
    MP, domain = MC.golden_domain(name)
    fixed = MC.outer_dofs(MP, domain)
    assert np.array_equal(fixed, g[name + '_fixed'])
    ref, V = g[name + '_lam'], g[name + '_V']
    K, Mm = host_matrices(MP)
    free = np.setdiff1d(np.arange(K.shape[0]), fixed)
    Kf, Mf = K[free][:, free], Mm[free][:, free].tocsc()
    tol = 1e-9
    try:
        S = solvers.MultipatchEigenSystem(MP, fixed)
        lam, U = S.solve(k=k, tol=tol)
        info = S.info
    finally:
        MP.close()
    assert info['converged'].all() and lam.shape == (k,) and info['block'] == min(16, k + max(2, k // 2))
    Uf = U[free]
    assert U.shape == (MP.numdofs, k) and np.all(U[fixed] == 0.0)
    orth = np.abs(Uf.T @ (Mf @ Uf) - np.eye(k)).max()
    solve_M = scipy.sparse.linalg.factorized(Mf)
    for i in range(k):
        x = Uf[:, i]
        r = Kf @ x - lam[i] * (Mf @ x)
        bound = np.sqrt(r @ solve_M(r)) / np.sqrt(x @ (Mf @ x))
        err = abs(lam[i] - ref[i])
        print(name, k, i, 'lam', lam[i], 'err', err, 'bound', bound, 'res', np.linalg.norm(r) / np.linalg.norm(Kf @ x))
        assert err <= max(bound, 1e-12 * ref[i])
        assert np.linalg.norm(r) <= 2.0 * tol * np.linalg.norm(Kf @ x)           # the stopping rule, recomputed (slack 2)
        assert info['residuals'][i] <= tol
        gaps = np.abs(np.delete(ref, i) - ref[i])
        if gaps.min() > 1e-6 * ref[i]:                                           # a non-degenerate pair: the same vector
            assert abs(U[:, i] @ (Mm @ V[:, i])) >= 1.0 - 1e-8
    assert orth <= 1e-10


# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lshape_runs():
    """n -> dict of the runs on the L-shape at p = 3 (k = 6, block 9, tol 1e-9, the same start block, a hierarchy down to 4 spans
    per patch): the device solve with 'mg', the host model on the matrices downloaded from the device, and at n = 64 the device
    solve with 'jacobi'.  Each solved once."""
    from pyiga_amd import solvers
    out = {}
    for n, nlev in ((16, 3), (64, 5)):
        MP = M.lshape(p=3, n=n)
        fixed = MC.outer_dofs(MP, 'lshape')
        Mm = MP.assemble_system(MASS, None)[0].tocsr()
        X0 = EM.start_block(MP.numdofs, 9, 0)
        try:
            S = solvers.MultipatchEigenSystem(MP, fixed)
            S.set_multigrid(levels=nlev)
            lam, U = S.solve(k=6, tol=1e-9, block=9, X0=X0, precond='mg')
            run = dict(lam=lam, U=U, info=S.info, fixed=fixed)
            run['lam2'], run['U2'] = S.solve(k=6, tol=1e-9, block=9, X0=X0, precond='mg')
            levels = [S.mg_level(l) for l in range(nlev)]
            As, MPs, fx = [L.matrix() for L in levels], [L.MP for L in levels], [L.bc_indices for L in levels]
            if n == 64:
                S.solve(k=6, tol=1e-9, block=9, X0=X0, precond='jacobi', maxiter=600)
                run['jacobi'] = S.info
                run['auto'] = S.set_precond('auto')
            model = G.Model(As, MPs, fx)
        finally:
            MP.close()
        ops = EM.NumpyOps(As[0], Mm, fixed, X0, lambda R: np.stack([model.apply_full(R[:, j]) for j in range(R.shape[1])], axis=1))
        mlam, run['minfo'] = solvers.lobpcg_loop(ops, 9, 6, 1e-9, 200)
        run['mlam'] = mlam[:6]
        out[n] = run
    return out


def test_lshaped_membrane(lshape_runs):
    lam = lshape_runs[16]['lam']
    print('lam_1 / 9.6397238440219 - 1 =', lam[0] / 9.6397238440219 - 1.0, ' lam_3 / (2 pi^2) - 1 =', lam[2] / (2 * np.pi ** 2) - 1.0)
    assert lshape_runs[16]['info']['converged'].all() and lshape_runs[16]['info']['precond'] == 'mg'
    assert 0.0 < lam[0] / 9.6397238440219 - 1.0 <= 6.4e-4
    assert -1e-10 <= lam[2] / (2 * np.pi ** 2) - 1.0 <= 4e-9


@pytest.mark.parametrize('n', [16, 64])
def test_device_solve_agrees_with_the_host_model(lshape_runs, n):
    run = lshape_runs[n]
    dev, minfo = run['info'], run['minfo']
    print(n, 'device', dev['iterations'], 'model', minfo['iterations'])
    assert dev['converged'].all() and minfo['converged'].all()
    assert abs(dev['iterations'] - minfo['iterations']) <= 2
    assert (np.abs(run['lam'] - run['mlam']) <= 1e-11 * np.abs(run['mlam'])).all()
    assert dev['block_products'] == dev['iterations'] + 1 and dev['restarts'] == 0
    assert np.array_equal(run['lam'], run['lam2']) and np.array_equal(run['U'], run['U2'])     # the same bits (injective maps)


def test_iterations_do_not_grow_with_the_mesh(lshape_runs):
    mg16, mg64, jac64 = lshape_runs[16]['info'], lshape_runs[64]['info'], lshape_runs[64]['jacobi']
    print('mg', mg16['iterations'], mg64['iterations'], 'jacobi', jac64['iterations'])
    assert abs(mg64['iterations'] - mg16['iterations']) <= 5
    assert jac64['converged'].all() and jac64['iterations'] >= 2 * mg64['iterations']
    assert lshape_runs[64]['auto'] == 'mg'


# ---------------------------------------------------------------------------------------------
def test_determinism_and_lifecycle():
    from pyiga_amd import _lib, solvers
    MP = M.lshape(p=2, n=8)
    fixed = MC.outer_dofs(MP, 'lshape')
    S = solvers.MultipatchEigenSystem(MP, (fixed, np.zeros(fixed.size)))
    assert S in MP._solvers
    lam, U = S.solve(k=4, tol=1e-9, timed=True, precond='jacobi')
    assert S.info['converged'].all() and S.info['precond'] == 'jacobi'
    assert all(S.info[key] > 0.0 for key in ('products_ms', 'gram_ms', 'combine_ms', 'residual_ms', 'precond_ms'))
    lam2, U2 = S.solve(k=4, tol=1e-9, precond='jacobi')
    assert np.array_equal(lam, lam2) and np.array_equal(U, U2)                    # the same bits
    lam3, U3 = S.solve(k=2, block=5, tol=1e-9, seed=3, precond='jacobi')          # another k, block and seed
    assert S.info['converged'].all() and S.info['block'] == 5 and U3.shape == (S.n, 2)
    assert (np.abs(lam3 - lam[:2]) <= 1e-10 * lam[:2]).all()
    for kw in (dict(k=0), dict(k=5, block=4), dict(k=2, block=17), dict(precond='schwarz'), dict(precond='kron')):
        with pytest.raises(ValueError):
            S.solve(**kw)
    # the C ABI's refusals: Kronecker / Schwarz on a multipatch solver, a mass matrix for a patch solver
    lib = _lib.load()
    for pc in (_lib.IGX_PRECOND_KRON, _lib.IGX_PRECOND_SCHWARZ):
        assert lib.igx_solver_eig_set_precond(S.handle, pc, None, None, None, None, 0) == _lib.IGX_ERR_UNSUPPORTED
    S.close()
    S.close()                                                                     # idempotent
    assert S not in MP._solvers
    with pytest.raises(_lib.IgxError):
        S.solve(k=4)
    # one scattered dof fixed: no union of whole sides, so 'auto' is Jacobi
    S = solvers.MultipatchEigenSystem(MP, np.append(fixed, np.setdiff1d(np.arange(MP.numdofs), fixed)[7]))
    lam4, _ = S.solve(k=2, tol=1e-9)
    assert S.info['precond'] == 'jacobi' and S.info['converged'].all()
    with pytest.raises(ValueError):
        S.solve(k=2, precond='mg')
    # a later assembly restarts the sums the solver reads
    MP.assemble_system(MASS, None)
    with pytest.raises(_lib.IgxError):
        S.solve(k=2)
    MP.close()                                                                    # destroys the solver
    assert S.handle is None
    with pytest.raises(_lib.IgxError):
        S.block_products(np.zeros((S.n, 2)))


def test_patch_solver_refuses_a_mass_matrix_and_multipatch_needs_one():
    from pyiga_amd import _lib, bspline, geometry, solvers
    from pyiga_amd.operators import DeviceArray
    lib = _lib.load()
    kv = bspline.make_knots(2, 0.0, 1.0, 4)
    P = solvers.PatchSystem((kv, kv), geometry.unit_square(), np.zeros(kv.numdofs ** 2))
    d = DeviceArray(P._ctx, 8)
    try:
        assert lib.igx_solver_set_mass_d(P.handle, d.ptr) == _lib.IGX_ERR_UNSUPPORTED
    finally:
        P.close()
    MP = M.lshape(p=2, n=4)
    fixed = MC.outer_dofs(MP, 'lshape')
    S = solvers.MultipatchSystem(MP, STIFF, None, (fixed, np.zeros(fixed.size)))
    try:
        assert lib.igx_solver_eig_set_precond(S.handle, _lib.IGX_PRECOND_NONE, None, None, None, None, 0) == _lib.IGX_ERR_ARG
        assert 'igx_solver_set_mass_d' in _lib.last_error()
    finally:
        MP.close()

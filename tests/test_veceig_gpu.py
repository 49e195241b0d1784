"""VectorEigenSystem on the device: parity with the reference's elasticity matrices and dense eigh
(tests/golden/golden_veceig.npz), the exact spectrum of two decoupled Laplacians with different boundary conditions, agreement
with the host model of the controller, a density-weighted mass, determinism, lifecycle and refusals."""
import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.linalg

import _eig_model as EM
import _veceig_model as VM
import _vecsolve_model as V

pytestmark = pytest.mark.gpu

MU_LAM = dict(mu=1.0, lam=2.0)
LAPLACE = 'inner(grad(u), grad(v)) * dx'


def patch(name):
    """kvs, geo, nc and the fixed dofs of the golden cases: `annulus2` clamped on every side, `cylinder3` a cantilever."""
    from pyiga_amd import bspline, geometry
    if name == 'annulus2':
        kvs, geo, nc, sides = VM.annulus2_kvs(), geometry.quarter_annulus(), 2, [(0, 0), (0, 1), (1, 0), (1, 1)]
    else:
        kvs = (bspline.make_knots(2, 0.0, 1.0, 4),) * 3
        geo, nc, sides = geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.quarter_annulus()), 3, [(0, 0)]
    return kvs, geo, nc, np.sort(V.side_dofs(kvs, sides, nc))


def elasticity(name, **kw):
    from pyiga_amd import solvers
    kvs, geo, nc, fixed = patch(name)
    return solvers.VectorEigenSystem(V.ELASTICITY, kvs, fixed, bfuns=V.bfuns(nc), geo=geo, **MU_LAM, **kw)


def host_matrices(name):
    from pyiga_amd import assemble
    kvs, geo, nc, _ = patch(name)
    K = assemble.assemble(V.ELASTICITY, kvs, geo=geo, bfuns=V.bfuns(nc), layout='blocked', **MU_LAM).tocsr()
    return K, VM.block_mass(assemble.mass(kvs, geo).tocsr(), nc)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name, k', [(name, k) for name in ('annulus2', 'cylinder3') for k in (4, 6, 10)])
def test_golden_parity(golden, name, k):
    g = golden('veceig')
    assert k in g[name + '_ks']                    # (every k of the table qualified on the reference's numbers)
    kvs, geo, nc, fixed = patch(name)
    assert np.array_equal(fixed, g[name + '_fixed'])
    ref, Vg = g[name + '_lam'], g[name + '_V']
    K, M = host_matrices(name)
    free = np.setdiff1d(np.arange(K.shape[0]), fixed)
    Kf, Mf = K[free][:, free], M[free][:, free].tocsc()
    tol = 1e-9
    S = elasticity(name)
    try:
        lam, U = S.solve(k=k, tol=tol)
        info = S.info
    finally:
        S.close()
    assert info['converged'].all() and lam.shape == (k,) and info['block'] == min(16, k + max(2, k // 2))
    assert U.shape == (K.shape[0], k) and np.all(U[fixed] == 0.0)
    Uf = U[free]
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
            assert abs(U[:, i] @ (M @ Vg[:, i])) >= 1.0 - 1e-8
    assert orth <= 1e-10


# ---------------------------------------------------------------------------------------------
def test_exact_spectrum_of_two_decoupled_components():
    """The vector Laplacian on the unit square: component 0 fixed on every side, component 1 on the two sides of axis 0 only.
    The eigenvalues are the sorted union of the two Kronecker-sum spectra (solvers.fastdiag_factors on each box): the masks and
    the boxes are per component.  tol = 1e-9: the eigenvalue error is quadratic in the residual."""
    from pyiga_amd import bspline, geometry, solvers
    kv = bspline.make_knots(3, 0.0, 1.0, 12)
    kvs, nd, k = (kv, kv), kv.numdofs, 8
    N = nd * nd
    idx = np.arange(N).reshape(nd, nd)
    fixed = np.sort(np.concatenate([EM.boundary_dofs((nd, nd)), np.concatenate([idx[0], idx[-1]]) + N]))
    parts = []
    for lo, hi in (((1, 1), (nd - 1, nd - 1)), ((1, 0), (nd - 1, nd))):
        lam1 = solvers.fastdiag_factors(kvs, lo, hi, True)[1]
        parts.append(np.add.outer(lam1[0], lam1[1]).ravel())
    exact = np.sort(np.concatenate(parts))
    assert exact[k] - exact[k - 1] > 1e-3 * exact[k]          # the cut is between clusters
    S = solvers.VectorEigenSystem(LAPLACE, kvs, fixed, bfuns=V.bfuns(2), geo=geometry.unit_square())
    try:
        assert S.boxes == [((1, 1), (nd - 1, nd - 1)), ((1, 0), (nd - 1, nd))] and S.present == [[True, False], [False, True]]
        lam, U = S.solve(k=k, tol=1e-9)
        print('iterations', S.info['iterations'], 'rel err', np.abs(lam - exact[:k]) / exact[:k])
        assert S.info['converged'].all() and S.info['precond'] == 'kron'
        assert np.all(np.diff(lam) >= 0.0)
        assert (np.abs(lam - exact[:k]) <= 1e-10 * exact[:k]).all()
        assert U.shape == (2 * N, k) and np.all(U[fixed] == 0.0)
        assert U.reshape((2, nd, nd, k)).shape == (2,) + S.ndofs + (k,)
    finally:
        S.close()


# ---------------------------------------------------------------------------------------------
def test_device_solve_agrees_with_the_host_model(golden):
    g = golden('veceig')
    X0 = EM.start_block(g['annulus2_V'].shape[0], 8, 4)
    S = elasticity('annulus2')
    try:
        lam, _ = S.solve(k=6, tol=1e-9, block=8, X0=X0, precond='kron')
        dev = S.info
        factors = S.kron_factors()
    finally:
        S.close()
    mlam, minfo, mX0 = VM.run_model(g, 6, 8, 4, factors)
    assert np.array_equal(X0, mX0)
    print('device', dev['iterations'], 'model', minfo['iterations'], 'rel diff', np.abs(lam - mlam[:6]) / mlam[:6])
    assert dev['converged'].all() and minfo['converged'].all()
    assert abs(dev['iterations'] - minfo['iterations']) <= 2
    assert (np.abs(lam - mlam[:6]) <= 1e-11 * np.abs(mlam[:6])).all()
    assert dev['block_products'] == dev['iterations'] + 1 and dev['restarts'] == 0


def test_density_weighted_mass_scales_the_spectrum():
    S = elasticity('annulus2')
    F = elasticity('annulus2', mass='2.5*u*v*dx')
    try:
        lam, _ = S.solve(k=6, tol=1e-9)
        flam, _ = F.solve(k=6, tol=1e-9)
        assert S.info['converged'].all() and F.info['converged'].all()
        assert (np.abs(flam * 2.5 - lam) <= 1e-10 * lam).all(), (flam * 2.5 - lam) / lam
    finally:
        S.close()
        F.close()


# ---------------------------------------------------------------------------------------------
def test_c_abi_refusals():
    """igx_solver_take_mass and the eigen entries on block solvers they do not serve: IGX_ERR_ARG and a message, no crash."""
    from pyiga_amd import _lib, solvers
    lib = _lib.load()
    kvs, geo, nc, fixed = patch('annulus2')
    bcs = (fixed, np.zeros(fixed.size))
    X0 = np.zeros((nc * 169, 4))
    S = elasticity('annulus2')
    P = solvers.VectorFormSystem(V.ELASTICITY, kvs, 0.0, bcs, bfuns=V.bfuns(nc), geo=geo, **MU_LAM)     # symmetric, no mass taken
    Q = solvers.VectorFormSystem(V.NONSYM, kvs, 0.0, bcs, bfuns=V.bfuns(nc), geo=geo)                   # not symmetric
    R = solvers.PatchSystem(kvs, geo, np.zeros(169), (fixed[fixed < 169], np.zeros((fixed < 169).sum())))
    try:
        assert lib.igx_solver_take_mass(S.handle) == _lib.IGX_ERR_ARG                   # a second call
        assert lib.igx_solver_take_mass(R.handle) == _lib.IGX_ERR_ARG                   # not a block solver
        assert lib.igx_solver_take_mass(P.handle) == _lib.IGX_ERR_ARG                   # the patch holds no values (all handed over)
        # Kronecker before the factors of the components are set, and with box arguments
        assert lib.igx_solver_eig_set_precond(S.handle, _lib.IGX_PRECOND_KRON, None, None, None, None, 0) == _lib.IGX_ERR_ARG
        for T in (P, Q):                                                                # no mass / not symmetric
            assert lib.igx_solver_eig_begin(T.handle, 4, _lib.dptr(X0), 0) == _lib.IGX_ERR_ARG
            assert lib.igx_solver_eig_set_precond(T.handle, _lib.IGX_PRECOND_NONE, None, None, None, None, 0) == _lib.IGX_ERR_ARG
        with pytest.raises(_lib.IgxError, match='igx_solver_take_mass'):
            _lib.check(lib.igx_solver_eig_begin(P.handle, 4, _lib.dptr(X0), 0), 'igx_solver_eig_begin')
        lam, _ = S.solve(k=4, tol=1e-9)                                                 # the refused calls left S as it was
        assert S.info['converged'].all()
    finally:
        for T in (S, P, Q, R):
            T.close()


def test_determinism_lifecycle_refusals():
    from pyiga_amd import _lib, solvers
    kvs, geo, nc, fixed = patch('cylinder3')
    S = elasticity('cylinder3')
    try:
        lam, U = S.solve(k=4, tol=1e-9, timed=True)
        assert S.info['converged'].all() and S.info['products_ms'] > 0.0 and S.info['gram_ms'] > 0.0
        assert S.info['precond'] == 'kron' and S.info['n_free'] == S.n - fixed.size
        lam2, U2 = S.solve(k=4, tol=1e-9)
        assert np.array_equal(lam, lam2) and np.array_equal(U, U2)                # the same bits
        lam3, U3 = S.solve(k=2, block=5, tol=1e-9, seed=3, precond='jacobi', maxiter=2000)   # another k, block, seed, preconditioner
        assert S.info['converged'].all() and S.info['block'] == 5 and U3.shape == (S.n, 2) and S.info['precond'] == 'jacobi'
        assert (np.abs(lam3 - lam[:2]) <= 1e-10 * lam[:2]).all()
        for bad in (np.zeros((S.n, 5)), np.zeros((S.n - 1, 6)), np.zeros(S.n)):
            with pytest.raises(ValueError):
                S.solve(k=4, block=6, X0=bad)
        for kw in (dict(k=0), dict(k=5, block=4), dict(k=2, block=17), dict(k=1, block=S.n_free // 3 + 1), dict(precond='schwarz')):
            with pytest.raises(ValueError):
                S.solve(**kw)
        with pytest.raises(NotImplementedError):
            S.spmv(np.zeros(S.n))
    finally:
        S.close()
    with pytest.raises(_lib.IgxError):
        S.solve(k=4)
    with pytest.raises(_lib.IgxError):
        S.block_products(np.zeros((S.n, 2)))
    # scattered fixed dofs: no box, so 'auto' is Jacobi and 'kron' is refused
    S = solvers.VectorEigenSystem(V.ELASTICITY, kvs, fixed[::2], bfuns=V.bfuns(nc), geo=geo, **MU_LAM)
    try:
        assert S.boxes[0] is None and S.default_precond == 'jacobi'
        with pytest.raises(ValueError):
            S.solve(k=2, precond='kron')
    finally:
        S.close()

"""EigenSystem on the device: exact spectra of the unit square and cube, parity with the reference's
matrices and dense eigh (tests/golden/golden_eig.npz), agreement with the host model of the controller, determinism, lifecycle
and refusals."""
import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.linalg

import _eig_model as EM

pytestmark = pytest.mark.gpu


def patch(name, p, n):
    from pyiga_amd import bspline, geometry
    kv = bspline.make_knots(p, 0.0, 1.0, n)
    geo = {'annulus': geometry.quarter_annulus, 'square': geometry.unit_square, 'cube': geometry.unit_cube,
           'cylinder': lambda: geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.quarter_annulus())}[name]()
    kvs = (kv,) * geo.dim
    return kvs, geo, EM.boundary_dofs(tuple(k.numdofs for k in kvs))


def host_matrices(kvs, geo):
    from pyiga_amd import assemble
    return assemble.stiffness(kvs, geo).tocsr(), assemble.mass(kvs, geo).tocsr()


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name, p, n, k', [('square', 3, 16, 6), ('cube', 2, 6, 7)])
def test_exact_spectrum_of_the_identity_map(name, p, n, k):
    """On the identity map K and M are Kronecker sums and products of the 1D matrices: the discrete eigenvalues are the sorted
    sums of the 1D generalized eigenvalues (solvers.fastdiag_factors), degenerate pairs (square) and triples (cube) included;
    k does not split a cluster.  tol = 1e-9: the eigenvalue error is quadratic in the residual."""
    from pyiga_amd import solvers
    kvs, geo, fixed = patch(name, p, n)
    lam1 = solvers.fastdiag_factors(kvs, (1,) * len(kvs), tuple(kv.numdofs - 1 for kv in kvs), True)[1]
    sums = lam1[0]
    for l in lam1[1:]:
        sums = np.add.outer(sums, l)
    exact = np.sort(sums.ravel())
    assert exact[k] - exact[k - 1] > 1e-3 * exact[k]          # the cut is between clusters
    S = solvers.EigenSystem(kvs, geo, (fixed, np.zeros(fixed.size)))
    try:
        lam, U = S.solve(k=k, tol=1e-9)
        print(name, 'iterations', S.info['iterations'], 'rel err', np.abs(lam - exact[:k]) / exact[:k])
        assert S.info['converged'].all() and S.info['precond'] == 'kron'
        assert np.all(np.diff(lam) >= 0.0)
        assert (np.abs(lam - exact[:k]) <= 1e-10 * exact[:k]).all()
        assert U.shape == (S.n, k) and np.all(U[fixed] == 0.0)
    finally:
        S.close()


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name, p, n', [('annulus', 3, 16), ('cylinder', 2, 6)])
@pytest.mark.parametrize('k', [6, 12])
def test_golden_parity(golden, name, p, n, k):
    from pyiga_amd import solvers
    g = golden('eig')
    kvs, geo, fixed = patch(name, p, n)
    assert np.array_equal(fixed, g[name + '_fixed'])
    ref, V = g[name + '_lam'], g[name + '_V']
    K, M = host_matrices(kvs, geo)
    free = np.setdiff1d(np.arange(K.shape[0]), fixed)
    Kf, Mf = K[free][:, free], M[free][:, free].tocsc()
    tol = 1e-9
    S = solvers.EigenSystem(kvs, geo, fixed)
    try:
        lam, U = S.solve(k=k, tol=tol)
        info = S.info
    finally:
        S.close()
    assert info['converged'].all() and lam.shape == (k,) and info['block'] == min(16, k + max(2, k // 2))
    Uf = U[free]
    assert np.all(U[fixed] == 0.0)
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
            assert abs(U[:, i] @ (M @ V[:, i])) >= 1.0 - 1e-8
    assert orth <= 1e-10


# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def annulus_runs():
    """n -> (device info with 'kron', device lam, model info, model lam, device info with None): each solved once."""
    from pyiga_amd import solvers
    out = {}
    for n in (16, 64):
        kvs, geo, fixed = patch('annulus', 3, n)
        ndofs = tuple(kv.numdofs for kv in kvs)
        X0 = EM.start_block(int(np.prod(ndofs)), 8, 4)
        S = solvers.EigenSystem(kvs, geo, fixed)
        try:
            lam, _ = S.solve(k=6, tol=1e-9, block=8, X0=X0, precond='kron')
            dev = S.info
            plain = None
            if n == 64:
                S.solve(k=6, tol=1e-9, block=8, X0=X0, precond=None, maxiter=600)
                plain = S.info
            U1, lam1, _ = S._kron_factors()
        finally:
            S.close()
        K, M = host_matrices(kvs, geo)
        ops = EM.NumpyOps(K, M, fixed, X0, EM.kron_precond(U1, lam1, S.box, ndofs))
        mlam, minfo = solvers.lobpcg_loop(ops, 8, 6, 1e-9, 200)
        out[n] = (dev, lam, minfo, mlam[:6], plain)
    return out


@pytest.mark.parametrize('n', [16, 64])
def test_device_solve_agrees_with_the_host_model(annulus_runs, n):
    dev, lam, minfo, mlam, _ = annulus_runs[n]
    print(n, 'device', dev['iterations'], 'model', minfo['iterations'])
    assert dev['converged'].all() and minfo['converged'].all()
    assert abs(dev['iterations'] - minfo['iterations']) <= 2
    assert (np.abs(lam - mlam) <= 1e-11 * np.abs(mlam)).all()
    assert dev['block_products'] == dev['iterations'] + 1 and dev['restarts'] == 0


def test_kron_iterations_do_not_grow_with_the_mesh(annulus_runs):
    kron16, kron64, plain64 = annulus_runs[16][0], annulus_runs[64][0], annulus_runs[64][4]
    print('kron', kron16['iterations'], kron64['iterations'], 'none', plain64['iterations'])
    assert abs(kron64['iterations'] - kron16['iterations']) <= 15
    assert plain64['converged'].all() and plain64['iterations'] >= 2 * kron64['iterations']


# ---------------------------------------------------------------------------------------------
def test_determinism_lifecycle_refusals():
    from pyiga_amd import _lib, solvers
    kvs, geo, fixed = patch('cylinder', 2, 6)
    S = solvers.EigenSystem(kvs, geo, (fixed, np.zeros(fixed.size)))
    try:
        lam, U = S.solve(k=4, tol=1e-9, timed=True)
        assert S.info['converged'].all() and S.info['products_ms'] > 0.0 and S.info['gram_ms'] > 0.0
        lam2, U2 = S.solve(k=4, tol=1e-9)
        assert np.array_equal(lam, lam2) and np.array_equal(U, U2)                # the same bits
        lam3, U3 = S.solve(k=2, block=5, tol=1e-9, seed=3, precond='jacobi')      # another k, block, seed and preconditioner
        assert S.info['converged'].all() and S.info['block'] == 5 and U3.shape == (S.n, 2)
        assert (np.abs(lam3 - lam[:2]) <= 1e-10 * lam[:2]).all()
        for bad in (np.zeros((S.n, 5)), np.zeros((S.n - 1, 6)), np.zeros(S.n)):
            with pytest.raises(ValueError):
                S.solve(k=4, block=6, X0=bad)
        for kw in (dict(k=0), dict(k=5, block=4), dict(k=2, block=17), dict(k=1, block=S.n_free // 3 + 1), dict(precond='schwarz')):
            with pytest.raises(ValueError):
                S.solve(**kw)
    finally:
        S.close()
    with pytest.raises(_lib.IgxError):
        S.solve(k=4)
    with pytest.raises(_lib.IgxError):
        S.block_products(np.zeros((S.n, 2)))
    # scattered fixed dofs: no box, so 'auto' is Jacobi and 'kron' is refused
    S = solvers.EigenSystem(kvs, geo, fixed[::2])
    try:
        assert S.box is None and S.default_precond == 'jacobi'
        with pytest.raises(ValueError):
            S.solve(k=2, precond='kron')
    finally:
        S.close()


def test_symmetric_form_string_shifts_the_spectrum():
    """A reaction-diffusion string (a traced table that is symmetric) is K + 2.5 M: the stiffness spectrum plus 2.5."""
    from pyiga_amd import solvers
    kvs, geo, fixed = patch('annulus', 3, 16)
    S = solvers.EigenSystem(kvs, geo, fixed)
    F = solvers.EigenSystem(kvs, geo, fixed, problem='(inner(grad(u), grad(v)) + 2.5 * u * v) * dx')
    try:
        lam, _ = S.solve(k=5, tol=1e-9)
        flam, _ = F.solve(k=5, tol=1e-9)
        assert S.info['converged'].all() and F.info['converged'].all() and F.kind == 'form'
        assert (np.abs(flam - 2.5 - lam) <= 1e-10 * lam).all(), (flam - 2.5 - lam) / lam
    finally:
        S.close()
        F.close()

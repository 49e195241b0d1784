"""solvers.SaddlePointSystem on the device: the cells of the reference's solve-stokes notebook with spsolve replaced by the
device MINRES, against the golden solutions and the host model's recorded counts (tests/_saddle_cases.py); determinism; the
product against the host bmat; the pressure normalisations; the Schur scale; the refusals."""
import ctypes as C
import warnings

import numpy as np
import pytest
import scipy.sparse

from pyiga_amd import _lib, assemble, bspline, geometry, solvers

import _saddle_cases as sc
from _saddle_systems import problem as _problem, system as _system

pytestmark = pytest.mark.gpu

ITER_SLACK = 3             # iterations the device may differ from the model by (rounding order)


@pytest.fixture(scope='module')
def stokes_unpinned():
    S, nv = _system('stokes', 'unpinned')
    yield S, nv
    S.close()


def test_incompatible_data_in_3d(golden):
    """The 3D cavity unpinned: its lid data is not discretely compatible, so solve() warns, projects the mean off and solves the
    projected system -- the model's solution of that system (computed here on the golden matrices), not the golden, pinned one
    (0.97 away, the model's recorded error).  At tol = 1e-10: at 1e-12 MINRES's estimate sits on a plateau of 1.36e-12 phi_0 for 70
    iterations in the model, and rounding decides where a solve leaves it (model 248 iterations, device 178, the same solution to
    1.2e-8).  Accepted: the model's iteration count +- 3, 10 x its true residual, and 1e-6 of max |u| between the two solutions
    (both stop at 1e-10 of the same right-hand side; the golden amplification of the system is 19)."""
    from oracle import iga_oracle as orc
    its, err, res = sc.MODEL[('stokes3', 'unpinned', 1e-10)]
    M = sc.system(golden, 'stokes3')
    um, minfo = sc.model_solve(M, 'unpinned', 1e-10, orc)
    S, nv = _system('stokes3', 'unpinned')
    try:
        with pytest.warns(UserWarning, match='not compatible'):
            u = S.solve(tol=1e-10, maxiter=600)
        e = abs(u - M.u).max() / abs(M.u).max()
        d = abs(u - um).max() / abs(um).max()
        print('stokes3 unpinned: %d iterations (model %d), err against the pinned golden solution %.3f (model %.3f), against the '
              'model %.2e, relres %.3e (model %.3e), rhs mean / norm %.2e'
              % (S.info['iterations'], minfo['iterations'], e, err, d, S.info['relres'], res, abs(S.info['rhs_mean']) / S.info['rhs_norm']))
        assert S.info['converged'] and abs(S.info['iterations'] - its) <= ITER_SLACK and e <= 10 * err
        assert S.info['relres'] <= 10 * res <= 1e3 * 1e-10 and d <= 1e-6
    finally:
        S.close()


@pytest.mark.parametrize('name,which', [('stokes', 'unpinned'), ('stokes', 'pinned'), ('stokes3', 'pinned')])
def test_notebook_on_the_device(name, which, golden):
    """solve(tol=1e-12) against the golden solution: the error at most 10 x the model's, the iteration count within 3 of the
    model's, the true relative residual at most 10 x the model's (and below 1e3 tol)."""
    its, err, res = sc.MODEL[(name, which, 1e-12)]
    ref = sc.system(golden, name).u
    S, nv = _system(name, which)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('error')                 # (compatible data: no warning about the pressure mean)
            u = S.solve(tol=1e-12, maxiter=400)
        info = S.info
        e = abs(u - ref).max() / abs(ref).max()
        print('%s %s: %d iterations (model %d), err %.3e (model %.3e), relres %.3e (model %.3e), precond %s, spmv widths %s'
              % (name, which, info['iterations'], its, e, err, info['relres'], res, info['precond'],
                 sc.widths(*sc.system(golden, name).spaces)))
        assert info['converged'] and info['breakdown'] is None and info['precond'] == 'kron' and info['method'] == 'minres'
        assert u.shape == ref.shape and e <= 10 * err
        assert abs(info['iterations'] - its) <= ITER_SLACK
        assert info['relres'] <= 10 * res <= 1e3 * 1e-12
        U, P = S.split(u)
        d = len(S.kvs)
        assert U.shape == S.ndofs + (d,) and P.shape == S.ndofs_p and P.ravel()[0] == 0.0
        velocity, pressure = bspline.BSplineFunc(S.kvs, U), bspline.BSplineFunc(S.kvs_p, P)
        grid = (np.linspace(0, 1, 5),) * d
        assert velocity.grid_eval(grid).shape == (5,) * d + (d,) and pressure.grid_eval(grid).shape == (5,) * d
    finally:
        S.close()


def test_determinism_and_check_every(stokes_unpinned):
    S, _ = stokes_unpinned
    u1 = S.solve(tol=1e-10)
    it1 = S.info['iterations']
    u2 = S.solve(tol=1e-10)
    u5 = S.solve(tol=1e-10, check_every=5)
    assert np.array_equal(u1, u2) and np.array_equal(u1, u5) and S.info['iterations'] == it1 and S.info['converged']
    u7 = S.solve(tol=1e-10, check_every=7, timed=True)
    assert np.array_equal(u1, u7) and S.info['spmv_ms'] > 0.0


def test_spmv_against_the_host_bmat(stokes_unpinned):
    """spmv(x) on full random x against R K R^T x of the host bmat of the matrices assemble.assemble returns for a and b, row by
    row within (len + C) 2^-53 sum |v x|, len the entries of the row of K and C = 10 the additions of the kernels' reduction trees
    (at most 6 shuffle steps, the batch sums of a lane).  The velocity form is integrated with the Gauss rule of the pair here
    (q = 4 points per span; p + 1 = 4 for the velocity space alone: the same rule)."""
    S, nv = stokes_unpinned
    kvs = (S.kvs, S.kvs_p)
    geo = geometry.quarter_annulus()
    A = assemble.assemble('inner(grad(u), grad(v)) * dx', kvs[0], bfuns=[('u', 2), ('v', 2)], geo=geo)
    B = assemble.assemble('div(u) * p * dx', kvs, bfuns=[('u', 2, 0), ('p', 1, 1)], geo=geo)
    K = scipy.sparse.bmat([[A, B.T], [B, None]], format='csr')
    free = np.ones(S.n, dtype=bool)
    free[S.bc_indices] = False
    x = np.random.default_rng(5).standard_normal(S.n)
    y = S.spmv(x)
    xm = np.where(free, x, 0.0)
    LD = np.longdouble
    Kl = K.tocsr()
    ref = np.zeros(S.n, dtype=LD)
    mag = np.zeros(S.n)
    for i in range(S.n):
        sl = slice(Kl.indptr[i], Kl.indptr[i + 1])
        t = Kl.data[sl].astype(LD) * xm[Kl.indices[sl]].astype(LD)
        ref[i], mag[i] = t.sum(), float(abs(t).sum())
    lens = np.diff(Kl.indptr)
    bound = (lens + 10) * 2.0 ** -53 * mag
    assert np.array_equal(y[~free], np.zeros((~free).sum()))
    ratio = (abs(y.astype(LD) - ref)[free] / bound[free]).max()
    print('SaddlePointSystem.spmv: largest |dev - ref| / bound = %.3f' % float(ratio))
    assert ratio <= 1.0


def test_pressure_mean(stokes_unpinned):
    """pressure='mean': zero coefficient mean, and the velocity of 'auto' (the model's two normalisations differ by
    MODEL_VELOCITY_DIFF = 0 in the velocity: they shift the pressure of one solve)."""
    S, nv = stokes_unpinned
    ua = S.solve(tol=1e-10)
    um = S.solve(tol=1e-10, pressure='mean')
    p = um[nv:]
    assert abs(um[:nv] - ua[:nv]).max() <= 10 * sc.MODEL_VELOCITY_DIFF
    assert abs(p.mean()) <= p.size * 2.0 ** -52 * abs(p).max() and ua[nv] == 0.0
    assert abs((um[nv:] - um[nv]) - ua[nv:]).max() <= 4 * 2.0 ** -52 * abs(ua[nv:]).max()
    assert abs(S.info['rhs_mean']) <= 1e-10 * S.info['rhs_norm']


def test_viscosity_scales_the_schur_complement(stokes_unpinned):
    S1, _ = stokes_unpinned
    S1.solve(tol=1e-8)
    it1 = S1.info['iterations']
    S, nv = _system('stokes', 'unpinned', viscosity=0.01)
    try:
        u = S.solve(tol=1e-8)
        it = S.info['iterations']
        print('viscosity 0.01: %d iterations, viscosity 1: %d; the model without the Schur scale: %d'
              % (it, it1, sc.MODEL_VISCOSITY['unscaled']))
        assert S.info['converged'] and it <= 1.5 * it1 + 5 and it < sc.MODEL_VISCOSITY['unscaled']
        assert abs(it1 - sc.MODEL[('stokes', 'unpinned', 1e-8)][0]) <= ITER_SLACK
        # the velocity does not depend on the viscosity (right-hand side 0); the pressure scales with it
        u1 = S1.solve(tol=1e-10)
        u = S.solve(tol=1e-10)
        assert abs(u[:nv] - u1[:nv]).max() <= 1e-6 * abs(u1[:nv]).max()
        assert abs(u[nv:] - 0.01 * u1[nv:]).max() <= 1e-6 * abs(0.01 * u1[nv:]).max()
    finally:
        S.close()


def test_jacobi_and_no_preconditioner(stokes_unpinned):
    S, nv = stokes_unpinned
    uk = S.solve(tol=1e-10)
    itk = S.info['iterations']
    uj = S.solve(tol=1e-10, precond='jacobi', maxiter=2000)
    itj = S.info['iterations']
    assert S.info['converged'] and S.info['precond'] == 'jacobi' and itj > itk
    assert abs(uj - uk).max() <= 1e-6 * abs(uk).max()
    un = S.solve(tol=1e-10, precond=None, maxiter=3000)
    assert S.info['converged'] and S.info['iterations'] > itj and abs(un - uk).max() <= 1e-6 * abs(uk).max()
    print('MINRES iterations at tol 1e-10: kron %d, jacobi %d, none %d' % (itk, itj, S.info['iterations']))


def test_refusals_on_the_device(stokes_unpinned):
    S, nv = stokes_unpinned
    lib = _lib.load()
    UNSUPPORTED, ARG = 3, 1
    with pytest.raises(_lib.IgxError):
        S.set_method('cg')
    assert lib.igx_solver_set_method(S.handle, _lib.IGX_METHOD_BICGSTAB) == UNSUPPORTED
    assert S.method == 'minres' and lib.igx_solver_set_method(S.handle, _lib.IGX_METHOD_MINRES) == 0
    # MINRES on a PatchSystem
    kv = bspline.make_knots(2, 0.0, 1.0, 4)
    geo = geometry.quarter_annulus()
    bc = assemble.compute_dirichlet_bcs((kv, kv), geo, [('left', lambda x, y: 0.0)])
    PS = solvers.PatchSystem((kv, kv), geo, np.ones(kv.numdofs ** 2), bcs=bc)
    try:
        assert lib.igx_solver_set_method(PS.handle, _lib.IGX_METHOD_MINRES) == UNSUPPORTED
        assert lib.igx_solver_take_pair_block(PS.handle, S.pair.handle, 0) == ARG
        assert lib.igx_solver_saddle_projection(PS.handle, 1, None, None) == ARG
    finally:
        PS.close()
    # eigen and parabolic calls on a saddle solver
    assert lib.igx_solver_take_mass(S.handle) == UNSUPPORTED
    assert lib.igx_solver_eig_begin(S.handle, 4, None, 0) == UNSUPPORTED
    assert lib.igx_solver_take_values(S.handle, _lib.IGX_ROLE_MASS) == UNSUPPORTED
    assert lib.igx_solver_set_dirk(S.handle, 1, (C.c_double * 2)(1.0, 1.0), 0.1) == UNSUPPORTED
    assert 'saddle-point solver' in _lib.last_error()
    # a block taken twice, q out of range
    assert lib.igx_solver_take_pair_block(S.handle, S.pair.handle, 0) == ARG
    assert lib.igx_solver_take_pair_block(S.handle, S.pair.handle, 2) == ARG
    # the projection with a pinned pressure dof
    kvs_u, kvs_p, geo, bcs, nv = _problem('stokes')
    from pyiga_amd.assemblers import DevicePair, DevicePatch
    patch = DevicePatch(kvs_u, geo, nqp=4)
    other = DevicePatch(kvs_u, geo, nqp=4)
    pair, pair_other = DevicePair(patch, kvs_p), DevicePair(other, kvs_p)
    idx = np.ascontiguousarray(np.unique(bcs[0]), dtype=np.int64)
    ip = idx.ctypes.data_as(C.POINTER(C.c_int64))
    h = C.c_void_p()
    try:
        # a pair made over another patch
        assert lib.igx_solver_create_saddle(patch.handle, pair_other.handle, 2, ip, idx.size, C.byref(h)) == ARG and not h.value
        assert lib.igx_solver_create_saddle(patch.handle, pair.handle, 4, ip, idx.size, C.byref(h)) == ARG
        assert lib.igx_solver_create_saddle(patch.handle, pair.handle, 2, ip, idx.size, C.byref(h)) == 0
        assert lib.igx_solver_saddle_projection(h, 1, None, None) == ARG          # (a pinned pressure dof)
        assert lib.igx_solver_take_pair_block(h, pair.handle, 0) == ARG            # (a pair without values)
        # a solve with a B block missing: both diagonal blocks of A and B_0 only
        patch.set_form([[1.0, None, None, None]] + [[None] * 4] * 3)
        for c in range(2):
            patch.assemble('form', to_host=False)
            assert lib.igx_solver_take_block(h, c, c) == 0
        pair.assemble('form', to_host=False)
        assert lib.igx_solver_take_pair_block(h, pair.handle, 0) == 0
        assert not lib.igx_pair_d_data(pair.handle)                                # (the buffer was moved)
        b = np.zeros(nv + pair.shape[0])
        vals = np.ascontiguousarray(np.zeros(idx.size))
        u = np.zeros_like(b)
        assert lib.igx_solver_solve(h, _lib.dptr(b), _lib.dptr(vals), None, 1e-8, 10, 1, 0, _lib.dptr(u), None) == ARG
        assert 'B_1 missing' in _lib.last_error()
        assert lib.igx_solver_set_precond(h, _lib.IGX_PRECOND_KRON, None, None, None, None, 0) == ARG      # (no Schur part yet)
    finally:
        if h.value:
            lib.igx_solver_destroy(h)
        pair.close(); pair_other.close(); patch.close(); other.close()

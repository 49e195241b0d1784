"""solvers.OseenSystem on the device: the linear systems of the reference's solve-navier-stokes notebook with the wind given as
data and spsolve replaced by the device GMRES, against the golden solutions of golden_oseen.npz and the host model's recorded
counts (tests/_oseen_cases.py); restarts, determinism, the refusals, the Stokes systems by GMRES, three Arnoldi steps against the
model, and a right-hand side that is not finite."""
import ctypes as C
import warnings

import numpy as np
import pytest
import scipy.sparse

from pyiga_amd import _lib, assemble, bspline, geometry, solvers

import _gmres_model as gm
import _oseen_cases as oc
import _saddle_cases as sc
from _oseen_systems import system as _system, wind2
from _saddle_systems import system as _stokes_system

pytestmark = pytest.mark.gpu

LONG = 128                 # the longest cycle the device holds: what the comparisons with the goldens solve with
UNSUPPORTED, ARG = 3, 1


def _err(u, ref):
    return abs(u - ref).max() / abs(ref).max()


@pytest.fixture(scope='module')
def oseen2(golden):
    S, nv = _system('oseen2', oc.system(golden, 'oseen2').nu)
    yield S, nv
    S.close()


@pytest.fixture(scope='module')
def stokes_pinned():
    S, nv = _system('stokes')
    yield S, nv
    S.close()


@pytest.mark.parametrize('name,tri', [('oseen2', True), ('oseen2', False), ('oseen3', True), ('oseen3', False)])
def test_goldens(name, tri, golden):
    """solve(tol=1e-12, precond='kron') against the golden solution: converged, the error at most 10 x the model's, the true
    relative residual at most 10 x the model's, at most 1.5 x the model's steps + 5."""
    its, restarts, err, res = oc.MODEL[(name, tri, LONG, 1e-12)]
    M = oc.system(golden, name)
    S, nv = _system(name, M.nu)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('error')
            u = S.solve(tol=1e-12, maxiter=3000, precond='kron', triangular=tri, restart=LONG)
        info = S.info
        e = _err(u, M.u)
        print('%s %s: %d steps, %d restarts (model %d, %d), err %.3e (model %.3e), relres %.3e (model %.3e)'
              % (name, 'triangular' if tri else 'diagonal', info['iterations'], info['restarts'], its, restarts, e, err, info['relres'], res))
        assert info['converged'] and info['breakdown'] is None and info['precond'] == 'kron' and info['method'] == 'gmres'
        assert info['triangular'] == tri and info['restart'] == LONG
        assert u.shape == M.u.shape and e <= 10 * err
        assert info['relres'] <= 10 * res
        assert info['iterations'] <= 1.5 * its + 5
        U, P = S.split(u)
        assert U.shape == S.ndofs + (S.ncomp,) and P.shape == S.ndofs_p and P.ravel()[0] == 0.0
    finally:
        S.close()


def test_triangular_takes_fewer_steps(oseen2):
    S, _ = oseen2
    S.solve(tol=1e-10, restart=LONG, triangular=True)
    it_t = S.info['iterations']
    S.solve(tol=1e-10, restart=LONG, triangular=False)
    print('oseen2 at tol 1e-10: %d steps triangular, %d diagonal' % (it_t, S.info['iterations']))
    assert S.info['converged'] and it_t < S.info['iterations']


def test_restarts(stokes_pinned, golden):
    """restart = 20 against one long cycle on `stokes` (pinned, triangular, tol 1e-12): the same solution within 1e-8 max |u|, with
    restarts.  restart = 5 stagnates on every system tried, in the model as on the device (_oseen_cases.py): its iterate after 60
    steps, 11 restarts, is compared with the model's, within the same 1e-8 max |u|."""
    from oracle import iga_oracle as orc
    S, nv = stokes_pinned
    u0 = S.solve(tol=1e-12, restart=LONG, maxiter=3000)
    i0 = S.info
    u20 = S.solve(tol=1e-12, restart=20, maxiter=3000)
    i20 = S.info
    d = abs(u20 - u0).max() / abs(u0).max()
    print('restart 20: %d steps, %d restarts (model %s); one cycle: %d steps (model %d); difference %.2e'
          % (i20['iterations'], i20['restarts'], oc.MODEL_RESTART20, i0['iterations'], oc.MODEL_LONG[0], d))
    assert i0['converged'] and i0['restarts'] == 0 and i0['iterations'] <= 1.5 * oc.MODEL_LONG[0] + 5
    assert i20['converged'] and i20['restarts'] > 0 and i20['iterations'] <= 1.5 * oc.MODEL_RESTART20[0] + 5
    assert d <= 1e-8
    u5 = S.solve(tol=1e-12, restart=5, maxiter=oc.RESTART5_STEPS)
    i5 = S.info
    um, im = oc.model_stokes(golden, orc, 'stokes', 'pinned', 1e-12, maxiter=oc.RESTART5_STEPS, restart=5, triangular=True)
    d5 = abs(u5 - um).max() / abs(um).max()
    print('restart 5: %d steps, %d restarts, relres %.3e (model %.3e), |dev - model| %.2e' % (i5['iterations'], i5['restarts'], i5['relres'],
                                                                                            im['relres'], d5))
    assert not i5['converged'] and i5['iterations'] == oc.RESTART5_STEPS == im['iterations']
    assert i5['restarts'] == im['restarts'] == oc.RESTART5_STEPS // 5 - 1 > 0
    assert d5 <= 1e-8 and i5['relres'] < 1.0


def test_determinism_and_check_every(oseen2):
    S, _ = oseen2
    u1 = S.solve(tol=1e-10, restart=LONG)
    it1 = S.info['iterations']
    assert S.info['converged']
    u2 = S.solve(tol=1e-10, restart=LONG)
    assert np.array_equal(u1, u2) and S.info['iterations'] == it1
    for ce in (5, 7):
        u = S.solve(tol=1e-10, restart=LONG, check_every=ce, timed=(ce == 7))
        assert np.array_equal(u1, u) and S.info['iterations'] == it1 and S.info['converged']
    assert S.info['spmv_ms'] > 0.0 and S.info['precond_ms'] > 0.0 and S.info['vector_ms'] > 0.0
    # with restarts, stopped by maxiter in the middle of a cycle
    v1 = S.solve(tol=1e-10, restart=7, maxiter=31)
    r1 = S.info['restarts']
    for ce in (5, 7):
        v = S.solve(tol=1e-10, restart=7, maxiter=31, check_every=ce)
        assert np.array_equal(v1, v) and S.info['iterations'] == 31 and S.info['restarts'] == r1 == 4


def test_maxiter_returns_the_last_iterate(oseen2, golden):
    S, nv = oseen2
    M = oc.system(golden, 'oseen2')
    u = S.solve(tol=1e-12, restart=LONG, maxiter=30)
    i30 = dict(S.info)
    assert not i30['converged'] and i30['iterations'] == 30 and i30['restarts'] == 0 and i30['breakdown'] is None
    assert np.isfinite(u).all() and np.array_equal(u[M.bcs[0]], M.bcs[1])
    S.solve(tol=1e-12, restart=LONG, maxiter=60)
    assert S.info['relres'] < i30['relres'] < 1.0               # (GMRES's residual falls monotonely within a cycle)


def test_refusals_on_the_device(oseen2):
    S, nv = oseen2
    lib = _lib.load()
    assert lib.igx_solver_set_gmres(S.handle, 129, 0) == ARG
    assert lib.igx_solver_set_gmres(S.handle, -1, 0) == ARG
    assert lib.igx_solver_set_gmres(S.handle, 0, 1) == ARG and 'MINRES' in _lib.last_error()
    assert lib.igx_solver_set_gmres(S.handle, 40, 1) == 0
    assert lib.igx_solver_gmres_orth_d(S.handle, None, 1, None, None, None) == ARG
    # the solver family is still guarded by igx_solver_set_method
    assert lib.igx_solver_set_method(S.handle, _lib.IGX_METHOD_BICGSTAB) == UNSUPPORTED
    assert lib.igx_solver_set_method(S.handle, _lib.IGX_METHOD_MINRES) == 0
    with pytest.raises(ValueError, match='method'):
        S.set_method('minres')
    kv = bspline.make_knots(2, 0.0, 1.0, 4)
    geo = geometry.quarter_annulus()
    bc = assemble.compute_dirichlet_bcs((kv, kv), geo, [('left', lambda x, y: 0.0)])
    PS = solvers.PatchSystem((kv, kv), geo, np.ones(kv.numdofs ** 2), bcs=bc)
    try:
        assert lib.igx_solver_set_gmres(PS.handle, 40, 0) == UNSUPPORTED
        assert lib.igx_solver_gmres_restarts(PS.handle) == 0
    finally:
        PS.close()


def test_minres_bits_survive_gmres():
    """After igx_solver_set_gmres(h, 0, 0) a MINRES solve of a symmetric system gives the bits it gave before GMRES was selected."""
    S, nv = _stokes_system('stokes', 'unpinned')
    lib = _lib.load()
    try:
        u1 = S.solve(tol=1e-10)
        it1 = S.info['iterations']
        assert lib.igx_solver_set_gmres(S.handle, 100, 1) == 0
        ug = S.solve(tol=1e-8, maxiter=300)                  # (a GMRES solve of the same handle, triangular preconditioner)
        assert S.info['converged'] and abs(ug - u1).max() <= 1e-5 * abs(u1).max()
        assert lib.igx_solver_set_gmres(S.handle, 0, 0) == 0
        u2 = S.solve(tol=1e-10)
        assert np.array_equal(u1, u2) and S.info['iterations'] == it1
    finally:
        S.close()


@pytest.mark.parametrize('base,which', sorted(oc.MODEL_STOKES))
def test_stokes_by_gmres(base, which, golden):
    """convection=None: the Stokes systems of test_saddle_gpu.py solved by GMRES (block-diagonal preconditioner, tol 1e-12)
    against stokes_u / stokes3_u with that file's margins: the error at most 10 x the model's, the true residual at most 10 x the
    model's (and below 1e3 tol), the steps within 1.5 x the model's + 5."""
    its, err, res = oc.MODEL_STOKES[(base, which)]
    ref = sc.system(golden, base).u
    S, nv = _system(base, which=which)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('error')
            u = S.solve(tol=1e-12, maxiter=1000, triangular=False, restart=LONG)
        info = S.info
        e = _err(u, ref)
        print('%s %s by GMRES: %d steps, %d restarts (model %d), err %.3e (model %.3e), relres %.3e (model %.3e)'
              % (base, which, info['iterations'], info['restarts'], its, e, err, info['relres'], res))
        assert info['converged'] and info['breakdown'] is None and info['precond'] == 'kron'
        assert e <= 10 * err and info['relres'] <= 10 * res <= 1e3 * 1e-12
        assert info['iterations'] <= 1.5 * its + 5
        assert u[nv] == 0.0
    finally:
        S.close()


def _host_system(S, nu):
    """K of the system S on the host from the matrices assemble.assemble returns for its three forms."""
    geo = geometry.quarter_annulus()
    kvs = (S.kvs, S.kvs_p)
    bf = [('u', 2), ('v', 2)]
    A = assemble.assemble('inner(grad(u), grad(v)) * dx', kvs[0], bfuns=bf, geo=geo)
    N = assemble.assemble('grad(u).dot(w).dot(v) * dx', kvs[0], bfuns=bf, geo=geo, w=wind2)
    B = assemble.assemble('div(u) * p * dx', kvs, bfuns=[('u', 2, 0), ('p', 1, 1)], geo=geo)
    return scipy.sparse.csr_matrix(nu * A + N), scipy.sparse.csr_matrix(B)


def test_three_arnoldi_steps_against_the_model(oseen2, golden):
    """Three steps without a preconditioner from Dirichlet data g != 0 and b != 0 -- the lifting, the products, the two
    Gram-Schmidt passes, the rotations, the back substitution and the update in the solver's own sequence -- against the host
    model on the host copies of the matrices.  Accepted: 50 (len + 10) 2^-53 of max |u|, len the longest row of K, the bound
    the MINRES kernels meet in the same comparison."""
    S, nv = oseen2
    lib = _lib.load()
    A, B = _host_system(S, oc.system(golden, 'oseen2').nu)
    K = scipy.sparse.bmat([[A, B.T], [B, None]], format='csr')
    rng = np.random.default_rng(17)
    fixed = S.bc_indices
    b, g = rng.standard_normal(S.n), rng.standard_normal(fixed.size)
    u = np.empty(S.n)
    info = _lib.SolveInfo()
    S.set_precond(None)
    _lib.check(lib.igx_solver_set_gmres(S.handle, 40, 0), 'igx_solver_set_gmres')
    _lib.check(lib.igx_solver_saddle_projection(S.handle, 0, None, None), 'igx_solver_saddle_projection')
    _lib.check(lib.igx_solver_solve(S.handle, _lib.dptr(b), _lib.dptr(g), None, 1e-30, 3, 1, 0, _lib.dptr(u), C.byref(info)),
               'igx_solver_solve')
    um, minfo = gm.solve(A, B, 2, (fixed, g), b=b, tol=1e-30, maxiter=3, restart=40)
    assert info.iterations == 3 == minfo['iterations'] and lib.igx_solver_last_breakdown(S.handle) == 0
    tol = 50 * (int(np.diff(K.indptr).max()) + 10) * 2.0 ** -53
    err = abs(u - um).max() / abs(um).max()
    print('three Arnoldi steps: |dev - model| / max |model| = %.2e (allowed %.2e), relres %.3e (model %.3e)'
          % (err, tol, info.relres, minfo['relres']))
    assert err <= tol and abs(info.relres - minfo['relres']) <= tol * minfo['relres']
    assert np.array_equal(u[fixed], g)


def test_nan_right_hand_side(oseen2):
    """A right-hand side that is not finite: the solve stops before its first step as IGX_BREAKDOWN_NONFINITE and returns the
    start vector (0 on the free dofs, g on the fixed ones)."""
    S, nv = oseen2
    lib = _lib.load()
    fixed = S.bc_indices
    g = np.random.default_rng(3).standard_normal(fixed.size)
    u, info = np.empty(S.n), _lib.SolveInfo()
    S.set_precond(None)
    _lib.check(lib.igx_solver_set_gmres(S.handle, 40, 0), 'igx_solver_set_gmres')
    b = np.full(S.n, np.nan)
    _lib.check(lib.igx_solver_solve(S.handle, _lib.dptr(b), _lib.dptr(g), None, 1e-8, 5, 1, 0, _lib.dptr(u), C.byref(info)), 'igx_solver_solve')
    free = np.ones(S.n, dtype=bool)
    free[fixed] = False
    assert not info.converged and info.iterations == 0 and lib.igx_solver_last_breakdown(S.handle) == _lib.IGX_BREAKDOWN_NONFINITE
    assert not u[free].any() and np.array_equal(u[fixed], g)
    S.b[:] = np.nan
    try:
        un = S.solve(tol=1e-8, maxiter=5)
        assert S.info['breakdown'] == 'nonfinite' and not S.info['converged'] and not un[free].any()
    finally:
        S.b[:] = 0.0

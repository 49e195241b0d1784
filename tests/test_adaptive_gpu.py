"""Adaptive steps and Rosenbrock methods on the device (solvers.ParabolicSystem.integrate_adaptive, igx_solver_step_*; DESIGN.md
section 18), on an MI355X.

1. The reference's adaptive runs of golden_adaptive.npz: the identical accept/reject sequence, times and states within
   _adaptive_model.T (heat 2D / 3D by CG, convection-diffusion by BiCGStab with its mass solves by CG).
2. The constant-step Rosenbrock goldens through integrate and integrate_adaptive(tol=None).
3. Exact stability on the identity map: discrete eigenvectors take u_N = prod_k R(-tau_k lam) u0, every reported r is the
   analytic one, and with the Kronecker preconditioner every stage solve and every mass solve takes one iteration although tau
   changes (the eigenvalue refresh and the mass preconditioner are right).
4. k_err_norm alone against numpy.  5. A rejected attempt leaves the state (and F_1) untouched.
6. Non-convergence ends by max_attempts; constant-step integration afterwards is unchanged.
"""
import warnings

import numpy as np
import pytest

from pyiga_amd import _lib, bspline, geometry, solvers

import _adaptive_model as AM
import _parabolic_model as P

pytestmark = pytest.mark.gpu

CD2_FORM = '(inner(diff_coeff*grad(u),grad(v))+inner((x[1],-x[0]),grad(u))*v)*dx'
RUNS = {'heat2': ('esdirk23', 'sdirk21', 'esdirk34', 'rodasp', 'rosi2p1', 'rowdaind2', 'ros3p'),
        'heat3': ('esdirk23', 'rodasp'), 'cd2': ('esdirk34', 'rodasp')}


def _boundary(ndofs):
    idx = np.indices(ndofs).reshape(len(ndofs), -1)
    on = np.zeros(idx.shape[1], dtype=bool)
    for k, n in enumerate(ndofs):
        on |= (idx[k] == 0) | (idx[k] == n - 1)
    return np.flatnonzero(on)


def _system(g, case):
    pre = case + '_'
    bcs = (g[pre + 'bc_idx'], g[pre + 'bc_val'])
    if case == 'heat3':
        kvs = (bspline.make_knots(2, 0.0, 1.0, 6),) * 3
        geo = geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.quarter_annulus())
        return solvers.ParabolicSystem(kvs, geo, g[pre + 'rhs'], bcs)
    kvs = (bspline.make_knots(3, 0.0, 1.0, 16),) * 2
    geo = geometry.quarter_annulus()
    if case == 'heat2':
        return solvers.ParabolicSystem(kvs, geo, g[pre + 'rhs'], bcs)
    return solvers.ParabolicSystem(kvs, geo, g[pre + 'rhs'], bcs, problem=CD2_FORM, diff_coeff=lambda x, y: 0.2 + 0.1 * x * y)


@pytest.fixture(scope='module')
def systems(golden):
    """One device system per golden problem, shared by the tests of this module."""
    g = golden('adaptive')
    made = {}

    def get(case):
        if case not in made:
            made[case] = _system(g, case)
        return made[case]
    yield get
    for S in made.values():
        S.close()


def _deviation(times, sols, ref_times, ref_sols, t_end):
    scale = max(np.abs(u).max() for u in ref_sols)
    return (np.abs(np.array(times) - np.array(ref_times)).max() / t_end,
            max(np.abs(a - b).max() for a, b in zip(sols, ref_sols)) / scale)


@pytest.mark.parametrize('case, name', [(c, s) for c in RUNS for s in RUNS[c]])
def test_golden_adaptive_runs(golden, systems, case, name):
    g = golden('adaptive')
    pre = case + '_'
    S = systems(case)
    assert S.method == ('bicgstab' if case == 'cd2' else 'cg')
    times, sols = S.integrate_adaptive(g[pre + 'u0'], float(g['tau0']), float(g['t_end']), float(g['tol']), scheme=name,
                                       step_factor=float(g['step_factor']))
    info = S.info
    G = g[pre + name + '_log']
    U, tt = g[pre + name + '_u'], g[pre + name + '_times']
    print(case, name, 'attempts', info['attempts'], 'rejections', info['rejections'], 'reformations', info['reformations'],
          'stage iterations', int(info['stage_iterations'].sum()), 'mass iterations', int(info['mass_iterations'].sum()),
          'precond', info['precond'], 'method', info['method'])
    assert info['converged'] and info['attempts'] == len(G), (info['attempts'], len(G))
    assert np.array_equal(info['accepted'], G[:, 2] != 0)                     # the identical accept/reject sequence
    assert len(sols) == len(U) and len(times) == len(tt)
    dt, du = _deviation(times, sols, tt, U, float(g['t_end']))
    dr = np.abs(info['r'] / G[:, 1] - 1).max() if name != 'ros3p' else info['r'].max()
    print(case, name, 'deviation of the times %.2e, of the states %.2e, of r %.2e; T = %.1e' % (dt, du, dr, AM.T))
    assert dt <= AM.T and du <= AM.T, (case, name, dt, du)
    if name == 'ros3p':
        assert info['r'].max() < 1e-6                                         # its estimate vanishes: rounding level
    assert info['precond'] == 'kron' and info['method'] == S.method
    assert info['reformations'] >= info['rejections']                         # every change of tau forms C again, nothing else does
    if name in solvers.ADAPTIVE_DIRK_SCHEMES:
        assert np.all(info['mass_iterations'] >= 1)


@pytest.mark.parametrize('name', ['esdirk23', 'rodasp'])
def test_golden_runs_with_the_jacobi_preconditioner(golden, systems, name):
    """The session's Jacobi preconditioner: the diagonal of the values in use, made again by k_diag for every C and for M."""
    g = golden('adaptive')
    S = systems('heat2')
    times, sols = S.integrate_adaptive(g['heat2_u0'], float(g['tau0']), float(g['t_end']), float(g['tol']), scheme=name,
                                       step_factor=float(g['step_factor']), precond='jacobi')
    info = S.info
    G = g['heat2_%s_log' % name]
    assert info['converged'] and info['precond'] == 'jacobi' and np.array_equal(info['accepted'], G[:, 2] != 0)
    dt, du = _deviation(times, sols, g['heat2_%s_times' % name], g['heat2_%s_u' % name], float(g['t_end']))
    print('jacobi', name, 'stage iterations', int(info['stage_iterations'].sum()), 'mass iterations',
          int(info['mass_iterations'].sum()), 'deviation of the times %.2e, of the states %.2e' % (dt, du))
    assert dt <= AM.T and du <= AM.T, (name, dt, du)


def test_constant_step_rosenbrock_goldens(golden, systems):
    g = golden('adaptive')
    S = systems('heat2')
    tau, t_end = float(g['const_tau']), float(g['const_t_end'])
    for name, run in (('rodasp', lambda: S.integrate(g['heat2_u0'], tau, t_end, scheme='rodasp', tol=1e-12)),
                      ('ros3pw', lambda: S.integrate_adaptive(g['heat2_u0'], tau, t_end, None, scheme='ros3pw', solve_tol=1e-12))):
        times, sols = run()
        U = g['heat2_%s_const_u' % name]
        assert len(sols) == len(U) and S.info['converged'] and S.info['rejections'] == 0
        assert np.allclose(times, g['heat2_%s_const_times' % name], rtol=0, atol=1e-15)
        d = max(np.abs(a - b).max() for a, b in zip(sols, U)) / np.abs(U).max()
        print('constant steps', name, 'rel. difference %.2e' % d, 'reformations', S.info['reformations'])
        assert d < 1e-8, (name, d)
        assert S.info['reformations'] <= 1                                    # one tau: C is formed once


@pytest.mark.parametrize('d, p, n', [(2, 3, 16), (3, 2, 6)])
def test_exact_stability_with_changing_steps(d, p, n):
    kvs = (bspline.make_knots(p, 0.0, 1.0, n),) * d
    geo = geometry.unit_square() if d == 2 else geometry.unit_cube()
    ndofs = tuple(kv.numdofs for kv in kvs)
    fixed = _boundary(ndofs)
    tol = 1e-3
    S = solvers.ParabolicSystem(kvs, geo, 0.0, bcs=(fixed, np.zeros(fixed.size)))
    try:
        U, lam, _ = solvers.fastdiag_factors(kvs, (1,) * d, tuple(m - 1 for m in ndofs), True)
        k = len(lam[0]) // 2
        mode = U[0][:, k]
        for e in range(1, d):
            mode = np.multiply.outer(mode, U[e][:, k])
        u0 = np.zeros(ndofs)
        u0[(slice(1, -1),) * d] = mode
        u0 = u0.ravel()
        free = np.ones(u0.size, dtype=bool)
        free[fixed] = False
        lk = d * lam[0][k]
        for name in ('esdirk23', 'sdirk21', 'rodasp'):
            times, sols = S.integrate_adaptive(u0, 1.0 / lk, 6.0 / lk, tol, scheme=name, precond='kron')
            info = S.info
            if name in solvers.ROSENBROCK_SCHEMES:
                A, G, b, bh, _ = solvers.rosenbrock_tableau(name)
                B, implicit = A + G, np.arange(len(b))
            else:
                E, _ = solvers.embedded_tableau(name)
                s = E.shape[1]
                B, b, bh, implicit = E[:s], E[s], E[s + 1], np.flatnonzero(np.diag(E[:s]))
            assert info['converged'] and len(set(info['tau'])) > 2 and info['attempts'] >= 4     # (tau does change)
            amp, worst_r = 1.0, 0.0
            for tau, r, ok in zip(info['tau'], info['r'], info['accepted']):
                z = -tau * lk
                R, Rh = AM.stability_weights(B, b, z), AM.stability_weights(B, bh, z)
                u = amp * u0[free]
                want = abs(Rh - R) * abs(amp) * np.linalg.norm(u0[free] / (tol + tol * np.abs(u))) / np.sqrt(u.size)
                worst_r = max(worst_r, abs(r / want - 1))
                if ok:
                    amp *= R
            err = np.abs(sols[-1] - amp * u0).max() / np.abs(u0).max()
            print('identity map', d, name, 'attempts', info['attempts'], 'rejections', info['rejections'],
                  'final state error %.2e' % err, 'largest relative error of r %.2e' % worst_r)
            assert err < 1e-10, (name, err)
            assert worst_r < 1e-8, (name, worst_r)
            assert np.all(info['stage_iterations'][:, implicit] == 1), (name, info['stage_iterations'])
            if name in solvers.ADAPTIVE_DIRK_SCHEMES:
                assert np.all(info['mass_iterations'] == 1), (name, info['mass_iterations'])
                assert abs(AM.stability_weights(B, b, -0.7) - P.stability(solvers.dirk_tableau(name), -0.7)) < 1e-14
    finally:
        S.close()


@pytest.mark.parametrize('p, n', [(2, (6, 6)), (2, (15, 17)), (1, (513, 513))])
def test_err_norm_against_numpy(p, n):
    """k_err_norm alone: 64 dofs (less than a block), 17 x 19 = 323 (odd: the last dof is the tail lane's) and the 264196 dofs that
    pass one grid of the vector kernels; 1, 3 and COMB_MAX vectors."""
    import _solver_cases as sc
    kvs = tuple(bspline.make_knots(p, 0.0, 1.0, m) for m in n)
    ndofs = tuple(kv.numdofs for kv in kvs)
    N = int(np.prod(ndofs))
    assert N == {(6, 6): 64, (15, 17): 323, (513, 513): 264196}[n]
    if N > 1000:
        assert N > sc.vec_pass_rows()
    fixed = _boundary(ndofs)
    free = np.ones(N, dtype=bool)
    free[fixed] = False
    rng = np.random.default_rng(5)
    S = solvers.ParabolicSystem(kvs, geometry.unit_square(), 0.0, bcs=(fixed, np.zeros(fixed.size)))
    try:
        x = rng.standard_normal(N) * 10.0 ** rng.integers(-3, 3, N)
        for nv in (1, 3, _lib.COMB_MAX):
            V = [rng.standard_normal(N) for _ in range(nv)]
            c = rng.standard_normal(nv)
            for tol in (1e-3, 0.5):
                e = sum(ck * v for ck, v in zip(c, V))
                want = np.linalg.norm((e / (tol + tol * np.abs(x)))[free].astype(np.longdouble)) / np.sqrt(free.sum())
                for offset in (0, 1):                                          # 16-byte aligned vectors, and the scalar path
                    r1 = S.error_ratio(V, c, x, tol, offset=offset)
                    r2 = S.error_ratio(V, c, x, tol, offset=offset)
                    assert r1 == r2                                            # the same bits
                    rel = abs(r1 / float(want) - 1)
                    assert rel < 1e-13, (N, nv, tol, offset, rel)
            # large finite values on the fixed dofs do not reach the sum
            W = [v.copy() for v in V]
            W[0][fixed] = 1e200 * np.sign(c[0])
            for offset in (0, 1):
                assert S.error_ratio(W, c, x, 1e-3, offset=offset) == S.error_ratio(V, c, x, 1e-3, offset=offset)
        print('k_err_norm', N, 'dofs ok')
    finally:
        S.close()


@pytest.mark.parametrize('name', ['esdirk23', 'sdirk21', 'rodasp'])
def test_a_rejected_attempt_leaves_the_state_untouched(golden, systems, name):
    g = golden('adaptive')
    S = systems('heat2')
    tau, tol = float(g['tau0']), float(g['tol'])
    st, x0 = S.begin_steps(g['heat2_u0'], name)
    first = S.attempt_step(tau / 8, tol)
    assert first.converged
    S.accept_step()                                                            # (ESDIRK: F_1 is now the last stage's F)
    state = S.step_state()
    a = S.attempt_step(tau, tol)
    cand_a = S.step_state(candidate=True)
    assert a.converged and a.reformed and not np.array_equal(cand_a, state)
    b = S.attempt_step(tau / 3, tol)                                           # another step in between: C, the eigenvalues, F_s change
    cand_b = S.step_state(candidate=True)
    assert b.converged and b.reformed and not np.array_equal(cand_b, cand_a)
    assert np.array_equal(S.step_state(), state)
    c = S.attempt_step(tau, tol)
    assert c.converged and c.reformed
    assert np.array_equal(S.step_state(candidate=True), cand_a) and c.r == a.r            # bit-identical
    assert list(c.stage_iterations) == list(a.stage_iterations) and c.mass_iterations == a.mass_iterations
    again = S.attempt_step(tau, tol)
    assert not again.reformed and np.array_equal(S.step_state(candidate=True), cand_a)    # the same tau: C stays
    assert np.array_equal(S.step_state(), state)
    S.accept_step()
    assert np.array_equal(S.step_state(), cand_a)
    with pytest.raises(_lib.IgxError, match='no candidate'):
        S.accept_step()


def test_non_convergence_ends_by_max_attempts_and_leaves_constant_steps_intact(golden):
    gp = golden('parabolic')
    kvs = (bspline.make_knots(3, 0.0, 1.0, 16),) * 2
    S = solvers.ParabolicSystem(kvs, geometry.quarter_annulus(), gp['heat2_rhs'], (gp['heat2_bc_idx'], gp['heat2_bc_val']))
    try:
        with pytest.warns(RuntimeWarning, match='attempts allowed ran out'):
            times, sols = S.integrate_adaptive(gp['heat2_u0'], 2.0 ** -6, 0.25, 1e-3, scheme='esdirk23', maxiter=1, precond=None,
                                               max_attempts=6)
        info = S.info
        assert not info['converged'] and info['attempts'] == 6 and info['rejections'] == 6 and not info['accepted'].any()
        assert len(sols) == 1 and times == [0.0] and np.array_equal(sols[0], gp['heat2_u0'])
        assert np.allclose(info['tau'], 2.0 ** -6 * 0.5 ** np.arange(6), rtol=1e-15, atol=0) and np.isnan(info['r']).all()
        # at the ABI the constant-step run refuses the C and the preconditioner data a session left behind
        import ctypes
        lib, dirk_info, one = _lib.load(), _lib.DirkInfo(), np.empty((1, S.n))
        rc = lib.igx_solver_dirk_run(S.handle, _lib.dptr(S.b), _lib.dptr(S.bc_values), _lib.dptr(sols[0]), 1, 1, 1e-10, 10, 1, 0,
                                     _lib.dptr(one), None, ctypes.byref(dirk_info))
        assert rc == _lib.IGX_ERR_ARG and 'stepping session' in _lib.last_error()
        # constant steps afterwards: C and the preconditioner are formed again
        with warnings.catch_warnings():
            warnings.simplefilter('error')
            times, sols = S.integrate(gp['heat2_u0'], float(gp['heat2_tau']), float(gp['heat2_t_end']), scheme='sdirk3', tol=1e-12)
        U = gp['heat2_sdirk3_u']
        assert len(sols) == len(U) and S.info['converged'] and S.info['precond'] == 'kron'
        d = max(np.abs(a - b).max() for a, b in zip(sols, U)) / np.abs(U).max()
        print('sdirk3 after an adaptive run: rel. difference %.2e' % d)
        assert d < 1e-8, d
        # and an adaptive run after the constant steps uploads its factors again and converges
        times, sols = S.integrate_adaptive(gp['heat2_u0'], 2.0 ** -6, 0.05, 1e-3, scheme='rodasp')
        assert S.info['converged'] and S.info['accepted'].sum() >= 2
    finally:
        S.close()

"""Adaptive steps and Rosenbrock methods of parabolic problems (solvers.ParabolicSystem.integrate_adaptive, igx_solver_step_*):
what can be checked without a GPU.

- embedded_tableau / rosenbrock_tableau equal the arrays the reference's coeffs_* return (golden_adaptive.npz).
- The main rule of every Rosenbrock scheme meets the order conditions 1 and 2 with B = A + Gamma; R(-inf) is recorded.
- The host models (tests/_adaptive_model.py) reproduce every golden run: decisions, times and states; the lifted formulation the
  device runs equals the restricted one to 1e-12.
- What a relative residual of 1e-10 in every solve does to the golden runs: the measurement behind the tolerance T of the GPU test.
- The controller: both clips, r == 0, halving on non-convergence, termination by max_attempts.
- The estimates of ros3p and ros3pw vanish for an affine right-hand side.
- Every refusal is a ValueError before any device work; the new ABI is declared, bound and exported; igx_step_info's layout
  matches gcc's; a stepping session fails loudly without a GPU.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from pyiga_amd import _lib, solvers

import _adaptive_model as AM

from conftest import ROOT

NEW_NAMES = ('igx_solver_set_stepper', 'igx_solver_set_step_precond', 'igx_solver_step_begin', 'igx_solver_step_attempt',
             'igx_solver_step_accept', 'igx_solver_step_state', 'igx_solver_error_ratio_d')
ADAPTIVE_RUNS = [('heat2', s) for s in ('esdirk23', 'sdirk21', 'esdirk34', 'rodasp', 'rosi2p1', 'rowdaind2', 'ros3p')] + \
    [('heat3', 'esdirk23'), ('heat3', 'rodasp'), ('cd2', 'esdirk34'), ('cd2', 'rodasp')]
CONSTANT_RUNS = [('heat2', 'rodasp'), ('heat2', 'ros3pw')]
# R(-inf) = 1 - b^T (A + Gamma)^-1 1 of the main rules as the reference runs them (recorded, to 1e-6): ros3p and ros3pw have
# 1 - sqrt(3), the other three are L-stable
R_INF = {'ros3p': -0.7320508, 'ros3pw': -0.7320508, 'rowdaind2': 0.0, 'rodasp': 0.0, 'rosi2p1': 0.0}


def test_scheme_lists():
    assert solvers.ADAPTIVE_DIRK_SCHEMES == ('sdirk21', 'dirk34', 'esdirk23', 'esdirk34')
    assert solvers.ROSENBROCK_SCHEMES == ('ros3p', 'ros3pw', 'rowdaind2', 'rodasp', 'rosi2p1')
    assert solvers.DIRK_SCHEMES == ('implicit_euler', 'crank_nicolson', 'sdirk3', 'sdirk21', 'dirk34', 'esdirk23', 'esdirk34')
    assert _lib.COMB_MAX == 8 and _lib.IGX_DIRK_MAX_STAGES == 6


@pytest.mark.parametrize('name', solvers.ADAPTIVE_DIRK_SCHEMES)
def test_embedded_tableaux_equal_the_reference(golden, name):
    g = golden('adaptive')
    A, order = solvers.embedded_tableau(name)
    s = A.shape[1]
    assert A.shape == (s + 2, s) == g['tab_%s_A' % name].shape and order == int(g['tab_%s_order' % name])
    # (to the last bit but for gamma = 1 - sqrt(1/2), which dirk_tableau writes another way than the reference: 2 ulp at most)
    assert np.abs(A - g['tab_%s_A' % name]).max() <= 4.5e-16
    assert np.array_equal(A[:s + 1], solvers.dirk_tableau(name))
    assert solvers.embedded_tableau(name)[0] is not A


@pytest.mark.parametrize('name', solvers.ROSENBROCK_SCHEMES)
def test_rosenbrock_tableaux_equal_the_reference(golden, name):
    g = golden('adaptive')
    A, G, b, bh, order = solvers.rosenbrock_tableau(name)
    for key, a in (('A', A), ('Gamma', G), ('b', b), ('bhat', bh)):
        assert np.array_equal(a, g['tab_%s_%s' % (name, key)]), (name, key)
    assert order == int(g['tab_%s_order' % name])
    s = len(b)
    assert s <= _lib.IGX_DIRK_MAX_STAGES and A.shape == G.shape == (s, s)
    assert not np.triu(A).any() and not np.triu(G, 1).any() and np.all(np.diag(G) == G[0, 0]) and G[0, 0] > 0


@pytest.mark.parametrize('name', solvers.ROSENBROCK_SCHEMES)
def test_rosenbrock_order_conditions_and_stability_at_infinity(name):
    A, G, b, bh, _ = solvers.rosenbrock_tableau(name)
    res = AM.rosenbrock_order_conditions(A, G, b)
    # (ros3p's coefficients are given with 10 digits)
    assert abs(res[1]) < 1e-9 and abs(res[2]) < 1e-9, (name, res)
    r = AM.stability_rosenbrock(A, G, b, -np.inf)
    print('R(-inf) of', name, r)
    assert abs(r - R_INF[name]) < 1e-6, (name, r)
    assert abs(AM.stability_rosenbrock(A, G, b, -1e9) - r) < 1e-6
    for z in -np.logspace(-3, 6, 40):
        assert abs(AM.stability_rosenbrock(A, G, b, z)) <= 1 + 1e-9, (name, z)


def _golden_mats(oracle, case):
    """M and K of the golden problems (those of golden_parabolic.npz) from the oracle."""
    if case == 'heat3':
        kvs = (oracle.make_knots(2, 0.0, 1.0, 6),) * 3
        geo = oracle.geo_cylinder()
        return oracle.assemble('mass', kvs, geo), oracle.assemble('stiffness', kvs, geo)
    kvs = (oracle.make_knots(3, 0.0, 1.0, 16),) * 2
    geo = oracle.geo_quarter_annulus()
    M = oracle.assemble('mass', kvs, geo)
    if case == 'heat2':
        return M, oracle.assemble('stiffness', kvs, geo)
    kappa = lambda x, y: 0.2 + 0.1 * x * y
    table = [[None, lambda x, y: y, lambda x, y: -x], [None, kappa, None], [None, None, kappa]]
    return M, oracle.assemble_nonsymmetric('form', kvs, geo, table=table)


def _step(model, name):
    if name in solvers.ROSENBROCK_SCHEMES:
        T = solvers.rosenbrock_tableau(name)
        return (lambda x, tau, Fx: model.rosenbrock(T, x, tau, Fx)), T[4]
    A, order = solvers.embedded_tableau(name)
    return (lambda x, tau, Fx: model.dirk(A, x, tau, Fx)), order


def _model_run(g, mats, case, name, cls, perturb=0.0, **kw):
    pre = case + '_'
    M, K = mats
    model = cls(M, K, g[pre + 'rhs'], g[pre + 'bc_idx'], g[pre + 'bc_val'], perturb=perturb, seed=11, **kw)
    step, order = _step(model, name)
    return AM.run(step, model, g[pre + 'u0'], float(g['tau0']), float(g['t_end']), float(g['tol']), order,
                  step_factor=float(g['step_factor']))


@pytest.fixture(scope='module')
def mats(oracle):
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = _golden_mats(oracle, case)
        return cache[case]
    return get


def _deviation(times, sols, ref_times, ref_sols, t_end):
    scale = max(np.abs(u).max() for u in ref_sols)
    return max(np.abs(np.array(times) - np.array(ref_times)).max() / t_end,
               max(np.abs(a - b).max() for a, b in zip(sols, ref_sols)) / scale)


@pytest.mark.parametrize('case, name', ADAPTIVE_RUNS)
def test_models_reproduce_the_adaptive_golden_runs(golden, mats, case, name):
    g = golden('adaptive')
    pre = case + '_' + name
    times, sols, log, done = _model_run(g, mats(case), case, name, AM.Restricted)
    G = g[pre + '_log']
    assert done and len(log) == len(G) and np.array_equal(log[:, 2], G[:, 2])             # the decisions
    assert np.allclose(log[:, 0], G[:, 0], rtol=1e-9, atol=0)
    if name == 'ros3p':
        assert log[:, 1].max() < 1e-6 and G[:, 1].max() < 1e-6
    else:
        assert np.allclose(log[:, 1], G[:, 1], rtol=1e-6, atol=0)
    U, tt = g[pre + '_u'], g[pre + '_times']
    assert len(sols) == len(U)
    assert _deviation(times, sols, tt, U, float(g['t_end'])) < 1e-10
    lt, ls, llog, ldone = _model_run(g, mats(case), case, name, AM.Lifted)
    assert ldone and np.array_equal(llog[:, 2], log[:, 2])
    assert _deviation(lt, ls, times, sols, float(g['t_end'])) < 1e-12
    if name in solvers.ADAPTIVE_DIRK_SCHEMES:
        # The device solves M e = tau sum (b^_i - b_i) F_i for the estimate e = x_est - x_new itself.  In exact arithmetic that is
        # the same e; in floating point the reference's form carries the rounding of a mass solve for x_est, eps cond(M_ff) |x|
        # with cond(M_ff) < 1e4, into an estimate of the size tol |x| = 1e-3 |x|: r, and with it every later step, agree to
        # 1e-16 x 1e4 / 1e-3 = 1e-9 only.
        dt_, ds, dlog, ddone = _model_run(g, mats(case), case, name, AM.Lifted, difference=True)
        assert ddone and np.array_equal(dlog[:, 2], log[:, 2])
        assert _deviation(dt_, ds, times, sols, float(g['t_end'])) < 1e-9


@pytest.mark.parametrize('case, name', CONSTANT_RUNS)
def test_models_reproduce_the_constant_step_golden_runs(golden, mats, case, name):
    g = golden('adaptive')
    pre = case + '_'
    M, K = mats(case)
    T = solvers.rosenbrock_tableau(name)
    tau = float(g['const_tau'])
    U = g[pre + name + '_const_u']
    assert np.allclose(g[pre + name + '_const_times'], np.arange(len(U)) * tau, rtol=0, atol=1e-15)
    out = []
    for cls in (AM.Restricted, AM.Lifted):
        model = cls(M, K, g[pre + 'rhs'], g[pre + 'bc_idx'], g[pre + 'bc_val'])
        x = model.start(g[pre + 'u0'])
        sols = [model.complete(x)]
        for _ in range(len(U) - 1):
            x = model.rosenbrock(T[:3] + (None,), x, tau)[0]
            sols.append(model.complete(x))
        out.append(sols)
    scale = np.abs(U).max()
    assert max(np.abs(a - b).max() for a, b in zip(out[0], U)) / scale < 1e-10
    assert max(np.abs(a - b).max() for a, b in zip(out[0], out[1])) / scale < 1e-12


def test_sensitivity_to_the_solve_tolerance(golden, mats):
    """Every solve of the model left with a relative residual of 1e-10 (the device's solve_tol): the largest relative deviation
    of times and states over the golden runs.  AM.SENSITIVITY_MEASURED records it; T = min(10 x, 1e-6) is the GPU tolerance."""
    g = golden('adaptive')
    worst = 0.0
    for case, name in ADAPTIVE_RUNS:
        t0, s0, log0, _ = _model_run(g, mats(case), case, name, AM.Lifted, difference=True)
        t1, s1, log1, _ = _model_run(g, mats(case), case, name, AM.Lifted, perturb=1e-10, difference=True)
        assert np.array_equal(log0[:, 2], log1[:, 2]), (case, name)                      # no decision flips
        dev = _deviation(t1, s1, t0, s0, float(g['t_end']))
        print('sensitivity', case, name, '%.2e' % dev)
        worst = max(worst, dev)
    print('largest deviation %.3e, recorded %.3e, T %.3e' % (worst, AM.SENSITIVITY_MEASURED, AM.T))
    assert worst <= AM.SENSITIVITY_MEASURED                         # the recorded value is the measured one, rounded up
    assert worst >= AM.SENSITIVITY_MEASURED / 2
    assert AM.T == min(10 * AM.SENSITIVITY_MEASURED, 1e-6)


@pytest.mark.parametrize('controller', [AM.controller, solvers.next_step])
def test_controller(controller):
    assert controller(0.5, 1e-9, True, 0.9, 2) == (True, 2.5)                              # the upper clip 5
    assert controller(0.5, 1e6, True, 0.9, 2) == (False, 0.1)                              # the lower clip 0.2
    ok, tau = controller(1.0, 0.0, True, 0.9, 3)                                           # r == 0 counts as 1e-15
    assert ok and tau == 5.0
    ok, tau = controller(1.0, 0.25, True, 0.9, 2)
    assert ok and tau == pytest.approx(1.8, rel=1e-15)
    ok, tau = controller(1.0, 4.0, True, 0.9, 2)                                           # rejected steps shrink by the same rule
    assert not ok and tau == pytest.approx(0.45, rel=1e-15)
    assert controller(1.0, 1.0, True, 1.0, 2) == (True, 1.0)                               # accepted iff r <= 1
    assert controller(1.0, np.nextafter(1.0, 2.0), True, 1.0, 2)[0] is False
    assert controller(0.75, 0.1, False, 0.9, 2) == (False, 0.375)                          # no convergence: halved


def test_model_run_halves_on_non_convergence_and_stops_at_max_attempts():
    class Model:
        start = complete = weight = staticmethod(lambda x: np.asarray(x, dtype=float))
    calls = []

    def step(x, tau, Fx):
        calls.append(tau)
        if len(calls) <= 2:
            raise AM.NoConvergence()
        return x + tau, x + tau + 1e-4 * (1 + abs(x)), None          # r = 0.1

    times, sols, log, done = AM.run(step, Model, [1.0], 1.0, 10.0, 1e-3, 2)
    assert done and calls[:3] == [1.0, 0.5, 0.25] and np.isnan(log[:2, 1]).all() and not log[:2, 2].any()
    assert np.allclose(log[2:, 1], 0.1) and log[2:, 2].all() and times[-1] >= 10.0
    never = lambda x, tau, Fx: (_ for _ in ()).throw(AM.NoConvergence())
    times, sols, log, done = AM.run(never, Model, [1.0], 1.0, 10.0, 1e-3, 2, max_attempts=6)
    assert not done and len(log) == 6 and len(sols) == 1 and np.allclose(log[:, 0], 0.5 ** np.arange(6))


@pytest.mark.parametrize('name', ['ros3p', 'ros3pw'])
def test_estimates_of_ros3p_and_ros3pw_vanish_for_an_affine_right_hand_side(golden, mats, name):
    g = golden('adaptive')
    M, K = mats('heat2')
    T = solvers.rosenbrock_tableau(name)
    A, G = T[0], T[1]
    assert G[1, 0] == -A[1, 0]                                       # stage 2 has the right-hand side of stage 1
    model = AM.Restricted(M, K, g['heat2_rhs'], g['heat2_bc_idx'], g['heat2_bc_val'])
    x = model.start(g['heat2_u0'])
    for tol in (1e-2, 1e-4, 1e-6):
        for tau in (2.0 ** -6, 2.0 ** -3):
            x_new, x_est, _ = model.rosenbrock(T, x, tau)
            r = AM.error_ratio(x_est, x_new, x, tol)
            step = np.abs(x_new - x).max()
            assert step > 1e-3 and np.abs(x_est - x_new).max() < 1e-9 * step, (name, tau, r)
    # the weights b_hat - b are orthogonal to every (k, k, k3): those of stage 1 and 2 cancel, that of stage 3 vanishes
    d = T[3] - T[2]
    assert abs(d[0] + d[1]) < 1e-15 and abs(d[2]) < 1e-15


class _Stub(solvers.ParabolicSystem):
    """A ParabolicSystem without a device: integrate_adaptive must refuse before touching the handle."""

    def __init__(self):
        self.handle = None
        self.box = ((0, 0), (3, 3))
        self._precond = None
        self._step_precond = None

    def _live(self):
        raise AssertionError('device work')


@pytest.mark.parametrize('kw, match', [
    (dict(tol=0.0), 'tol'),
    (dict(tol=-1e-3), 'tol'),
    (dict(step_factor=0.0), 'step_factor'),
    (dict(step_factor=1.5), 'step_factor'),
    (dict(scheme='sdirk3'), 'no embedded rule'),
    (dict(scheme='crank_nicolson'), 'no embedded rule'),
    (dict(scheme='rk4'), 'unknown DIRK scheme'),
    (dict(scheme='rk4', tol=None), 'unknown DIRK scheme'),
    (dict(max_attempts=0), 'max_attempts'),
    (dict(tau0=0.0), 'tau0'),
    (dict(t_end=0.0), 't_end'),
    (dict(save_every=0), 'save_every'),
    (dict(precond='ilu'), 'preconditioner'),
])
def test_refusals_before_any_device_work(kw, match):
    args = dict(u0=np.zeros(9), tau0=1e-3, t_end=1e-2, tol=1e-3)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        _Stub().integrate_adaptive(**args)


def test_integrate_routes_rosenbrock_names_and_keeps_its_refusal():
    with pytest.raises(AssertionError, match='device work'):          # accepted: it reaches the device
        _Stub().integrate(np.zeros(9), 1e-3, 1e-2, scheme='rodasp')
    with pytest.raises(ValueError, match='unknown DIRK scheme'):
        _Stub().integrate(np.zeros(9), 1e-3, 1e-2, scheme='ros4')
    with pytest.raises(ValueError, match='unknown Rosenbrock scheme'):
        solvers.rosenbrock_tableau('rodas5')
    with pytest.raises(ValueError, match='no embedded rule'):
        solvers.embedded_tableau('sdirk3')


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(ROOT, 'pyiga_amd', 'libigx.so')):
        ge.build()
    return _lib


def test_new_abi_declared_bound_exported(lib):
    hdr = open(os.path.join(ROOT, 'include', 'igx.h')).read()
    bound = {name for name, _, _ in lib.SYMBOLS}
    nm = subprocess.run(['nm', '-D', '--defined-only', lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in NEW_NAMES:
        assert name + '(' in hdr and name in bound, name
        assert ' T %s\n' % name in nm, name
    lib.load()


def test_step_info_layout_matches_gcc(lib, tmp_path):
    src = tmp_path / 'sz.c'
    fields = [f for f, _ in lib.StepInfo._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "igx.h"\nint main(){printf("%zu", sizeof(igx_step_info));' +
                   ''.join('printf(" %%zu", offsetof(igx_step_info, %s));' % f for f in fields) +
                   'printf(" %d %d %d %d\\n", IGX_STEPPER_DIRK, IGX_STEPPER_ROSENBROCK, IGX_STEP_STATE, IGX_STEP_CANDIDATE); return 0;}')
    exe = tmp_path / 'sz'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    D = lib.StepInfo
    assert out == [ctypes.sizeof(D)] + [getattr(D, f).offset for f in fields] + \
        [lib.IGX_STEPPER_DIRK, lib.IGX_STEPPER_ROSENBROCK, lib.IGX_STEP_STATE, lib.IGX_STEP_CANDIDATE]


def test_session_fails_loudly_without_gpu(lib):
    code = ('import sys; sys.path.insert(0, %r)\n'
            'import numpy as np\n'
            'import pyiga_amd\n'
            'from pyiga_amd import bspline, geometry, solvers\n'
            'kv = bspline.make_knots(2, 0.0, 1.0, 4)\n'
            'assert hasattr(solvers.ParabolicSystem, "integrate_adaptive")\n'
            'try:\n'
            '    S = solvers.ParabolicSystem((kv, kv), geometry.unit_square(), 1.0)\n'
            '    S.integrate_adaptive(np.zeros(S.n), 1e-3, 1e-2, 1e-3)\n'
            'except pyiga_amd._lib.IgxError as e:\n'
            '    print("RAISED", e)\n' % ROOT)
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1')
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, env=env)
    assert 'RAISED' in out.stdout, out.stdout + out.stderr

"""The Oseen solver without a device: the host model of the device GMRES (tests/_gmres_model.py) on the golden systems of
golden_oseen.npz, the recorded constants of tests/_oseen_cases.py, the summed coefficient tables, the refusals and the ABI.
`python3 tests/test_oseen_cpu.py` prints the model's results in the form of the tables of _oseen_cases.py."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import iga_oracle as orc                  # noqa: E402
from pyiga_amd import _lib, bspline, solvers, tforms    # noqa: E402

import _gmres_model as gm       # noqa: E402
import _oseen_cases as oc       # noqa: E402
import _saddle_cases as sc      # noqa: E402

ITER_SLACK = 1                  # another BLAS moves the stop of the model by a step


def _err(u, ref):
    return abs(u - ref).max() / abs(ref).max()


@pytest.mark.parametrize('key', sorted(oc.MODEL, key=str))
def test_model_reproduces_the_goldens(key, golden):
    """The model converges to the golden solutions at tol = 1e-12.  The error: within 10 amp 1e-12 -- the golden amplification of
    a relative perturbation of the data, times the residual the solve stops at, times the margin of 10 of the Stokes tests -- and
    not above twice the recorded one; steps within ITER_SLACK of the recorded count (restarted runs: within the 1.5 x + 5 of the
    device tests, a restart amplifies a shifted stop), residual not above twice the recorded one."""
    name, tri, restart, tol = key
    its, restarts, err, res = oc.MODEL[key]
    S = oc.system(golden, name)
    u, info = oc.model_solve(S, orc, tri, restart, tol)
    e = _err(u, S.u)
    print("    (%r, %r, %r, %.0e): (%d, %d, %.2e, %.2e)," % (name, tri, restart, tol, info['iterations'], info['restarts'], e, info['relres']))
    assert info['converged'] and info['breakdown'] is None
    assert e <= 10 * S.amp * 1e-12 and e <= 2 * err and info['relres'] <= 2 * res
    if restarts == 0:
        assert abs(info['iterations'] - its) <= ITER_SLACK and info['restarts'] <= (0 if restart is None else 1)
    else:
        assert info['iterations'] <= 1.5 * its + 5 and its <= 1.5 * info['iterations'] + 5 and info['restarts'] > 0


def test_restarted_and_unrestarted_agree(golden):
    """On `stokes` (pinned, triangular preconditioner, tol 1e-12) restart = 20 and one long cycle give the same solution within
    1e-8 max |u|, the bound of the device test (at tol 1e-10 the two differ by 7.3e-8: the error of a solve is some 1e2 to 1e3
    times its relative residual on this system).
    restart = 5 stagnates (see _oseen_cases.py): what holds for it is GMRES's monotone residual -- after 60 steps not above that
    after 30 -- and the count of its restarts."""
    tol = 1e-12
    u0, i0 = oc.model_stokes(golden, orc, 'stokes', 'pinned', tol, triangular=True)
    u20, i20 = oc.model_stokes(golden, orc, 'stokes', 'pinned', tol, maxiter=3000, restart=20, triangular=True)
    d = _err(u20, u0)
    print('restart 20: %d steps, %d restarts; one cycle: %d steps; |difference| = %.2e' % (i20['iterations'], i20['restarts'], i0['iterations'], d))
    assert i0['converged'] and i0['restarts'] == 0 and abs(i0['iterations'] - oc.MODEL_LONG[0]) <= ITER_SLACK
    assert i20['converged'] and i20['restarts'] > 0 and d <= 1e-8
    assert i20['iterations'] <= 1.5 * oc.MODEL_RESTART20[0] + 5 and oc.MODEL_RESTART20[0] <= 1.5 * i20['iterations'] + 5
    _, a = oc.model_stokes(golden, orc, 'stokes', 'pinned', tol, maxiter=oc.RESTART5_STEPS // 2, restart=5, triangular=True)
    _, b = oc.model_stokes(golden, orc, 'stokes', 'pinned', tol, maxiter=oc.RESTART5_STEPS, restart=5, triangular=True)
    print('restart 5: true residual %.3e after %d steps, %.3e after %d' % (a['relres'], a['iterations'], b['relres'], b['iterations']))
    assert not b['converged'] and b['iterations'] == oc.RESTART5_STEPS and b['restarts'] == oc.RESTART5_STEPS // 5 - 1
    assert b['relres'] <= a['relres'] * (1 + 1e-12) < 1.0


@pytest.mark.parametrize('name', oc.CASES)
def test_triangular_needs_fewer_steps(name):
    diag, tri = oc.MODEL[(name, False, None, 1e-12)][0], oc.MODEL[(name, True, None, 1e-12)][0]
    print('%s: %d steps block-diagonal, %d block-triangular' % (name, diag, tri))
    assert tri < diag


@pytest.mark.parametrize('key', sorted(oc.MODEL_STOKES))
def test_stokes_by_gmres_reaches_the_minres_goldens(key, golden):
    """convection=None: GMRES on the symmetric Stokes systems against stokes_u / stokes3_u: not above twice the recorded error,
    and -- pinned, where the golden solution answers the same question -- within 10 amp 1e-12.  (GMRES stops on the residual's
    2-norm, MINRES on its P-norm: at one tolerance their errors differ, 2.0e-10 against 2.6e-13 on `stokes`.)"""
    base, which = key
    its, err, res = oc.MODEL_STOKES[key]
    u, info = oc.model_stokes(golden, orc, base, which, restart=128)
    ref = sc.system(golden, base).u
    e = _err(u, ref)
    print("    (%r, %r): (%d, %.2e, %.2e)," % (base, which, info['iterations'], e, info['relres']))
    assert info['converged'] and abs(info['iterations'] - its) <= ITER_SLACK
    assert e <= 2 * err and info['relres'] <= 2 * res
    if which == 'pinned':
        amp = float(golden('pair')['stokes_amp']) if base == 'stokes' else float(golden('saddle')['stokes3_amp'])
        assert e <= 10 * amp * 1e-12
    # both methods build the same Krylov space: not more steps than 1.5 x MINRES's + 5
    assert its <= 1.5 * sc.MODEL[(base, which, 1e-12)][0] + 5


def test_model_breakdowns_and_lucky_stop():
    K = lambda x: np.array([2.0, -1.0]) * x
    ident = lambda r: r.copy()
    x, it, restarts, conv, brk, _ = gm.gmres(K, ident, np.array([1.0, 1.0]), 1e-12, 10, 5)
    assert conv and brk is None and it == 2 and restarts == 0 and abs(x - [0.5, -1.0]).max() < 1e-14
    x, it, restarts, conv, brk, _ = gm.gmres(lambda x: x * np.nan, ident, np.array([1.0, 1.0]), 1e-8, 10, 5)
    assert not conv and brk == 'nonfinite' and not x.any()
    # an eigenvector as right-hand side: h_{1,0} = 0 in the first step, the lucky breakdown, converged
    x, it, restarts, conv, brk, _ = gm.gmres(K, ident, np.array([3.0, 0.0]), 1e-30, 10, 5)
    assert conv and it == 1 and abs(x - [1.5, 0.0]).max() < 1e-15
    # maxiter reached: the last iterate, not converged; restart = 1 is steepest residual descent
    x, it, restarts, conv, brk, _ = gm.gmres(K, ident, np.array([1.0, 1.0]), 1e-30, 3, 1)
    assert not conv and it == 3 and restarts == 2 and np.isfinite(x).all()


def test_summed_tables_are_those_of_the_single_form():
    """viscosity * tables(a) + tables(convection), as OseenSystem hands them over, against the tables of the one string
    'nu * a + convection' on the same grid: equal to rounding of the one product and sum per entry, absent blocks in the same
    places."""
    rng = np.random.default_rng(2)
    G = (5, 4)
    X = rng.standard_normal(G + (2,))
    wind = lambda x, y: (-y, x)
    bf = [('u', 2), ('v', 2)]
    nu = 0.3
    _, _, ta, _ = tforms.evaluate('inner(grad(u), grad(v)) * dx', G, X, {}, bf)
    _, _, tc, _ = tforms.evaluate('grad(u).dot(w).dot(v) * dx', G, X, {'w': wind}, bf)
    _, _, tw, _ = tforms.evaluate('(0.3 * inner(grad(u), grad(v)) + grad(u).dot(w).dot(v)) * dx', G, X, {'w': wind}, bf)
    scaled = [[[[None if e is None else nu * e for e in row] for row in tab] for tab in trow] for trow in ta]
    summed = solvers.add_block_tables(scaled, tc)
    assert not solvers.symmetric_block_tables(summed)
    for p in range(2):
        for q in range(2):
            for r in range(3):
                for s in range(3):
                    a, b = summed[p][q][r][s], tw[p][q][r][s]
                    assert (a is None) == (b is None), (p, q, r, s)
                    if a is not None:
                        assert abs(a - b).max() <= 4 * 2.0 ** -53 * abs(b).max()
    # the off-diagonal blocks are absent in both forms and stay so
    assert all(e is None for row in summed[0][1] for e in row) and all(e is None for row in summed[1][0] for e in row)
    assert solvers.add_block_tables(scaled, [[[[None] * 3] * 3] * 2] * 2)[0][0][1][1] is scaled[0][0][1][1]


# ---------------------------------------------------------------------------------------------
# refusals without a device
def _spaces():
    return (tuple(bspline.make_knots(3, 0.0, 1.0, n, mult=2) for n in (3, 2)), tuple(bspline.make_knots(2, 0.0, 1.0, n) for n in (3, 2)))


class _NoGeo:
    dim = sdim = 2


_WIND = {'w': lambda x, y: (1.0 + 0 * x, 0 * x)}


@pytest.mark.parametrize('convection,kw', [
    ('grad(u).dot(w).dot(v) * ds', _WIND),                       # a boundary measure
    ('inner(w, v) * dx', _WIND),                                 # linear, not bilinear
    ('grad(u).dot(w).dot(v)', _WIND),                            # no measure
    ('grad(u).dot(w).dot(v) * dx', {'w': lambda x, y: (1.0 + 0 * x, 0 * x, 0 * x)}),        # three wind components for ncomp = 2
    ('grad(u).dot(w).dot(v) * dx', {}),                          # the wind is missing
    (3.0, {}),
])
def test_refuses_bad_convection(convection, kw):
    with pytest.raises(ValueError, match='convection'):
        solvers.OseenSystem(_spaces(), _NoGeo(), None, convection=convection, **kw)


def test_refuses_other_arguments():
    with pytest.raises(ValueError, match='restart'):
        solvers.OseenSystem(_spaces(), _NoGeo(), None, restart=129, **_WIND)
    with pytest.raises(ValueError, match='restart'):
        solvers.OseenSystem(_spaces(), _NoGeo(), None, restart=0, **_WIND)
    with pytest.raises(ValueError, match='kvs_u, kvs_p'):
        solvers.OseenSystem(_spaces()[0], _NoGeo(), None, **_WIND)
    # `a` is checked as SaddlePointSystem checks it: the convection term does not come in through it
    with pytest.raises(ValueError, match='not supported'):
        solvers.OseenSystem(_spaces(), _NoGeo(), None, a='(inner(grad(u), grad(v)) + inner(dot(grad(u), w), v)) * dx', **_WIND)
    S = object.__new__(solvers.OseenSystem)              # (no device: the arguments are checked before the handle is touched)
    S.restart = 40
    with pytest.raises(ValueError, match='method'):
        S.set_method('minres')
    with pytest.raises(ValueError, match='restart'):
        S.solve(restart=200)
    with pytest.raises(ValueError, match='preconditioner'):
        S.solve(precond='ilu')
    S.set_method('gmres')
    assert S.method == 'gmres' and issubclass(solvers.OseenSystem, solvers.SaddlePointSystem)


def test_wind_as_an_array_over_the_gauss_grid_passes_the_check():
    kvs_u, kvs_p = _spaces()
    G = tuple(kv.numspans * 4 for kv in kvs_u)
    solvers._check_convection('grad(u).dot(w).dot(v) * dx', kvs_u, kvs_p, 2, {'w': np.ones(G + (2,))})
    with pytest.raises(ValueError, match='convection'):
        solvers._check_convection('grad(u).dot(w).dot(v) * dx', kvs_u, kvs_p, 2, {'w': np.ones(G + (3,))})


# ---------------------------------------------------------------------------------------------
# the ABI
NEW_FUNCTIONS = ('igx_solver_set_gmres', 'igx_solver_gmres_orth_d', 'igx_solver_gmres_timing', 'igx_solver_gmres_combine_d',
                 'igx_solver_gmres_restarts')


def test_abi():
    hdr = open(os.path.join(ROOT, 'include', 'igx.h')).read()
    lib_src = open(os.path.join(ROOT, 'pyiga_amd', '_lib.py')).read()
    for fn in NEW_FUNCTIONS:
        assert re.search(r'\bint\s+%s\(' % fn, hdr), fn
        assert "('%s'," % fn in lib_src, fn
    # GMRES is selected by a call of its own: no new method or breakdown constant
    assert _lib.METHODS == {'cg': 0, 'bicgstab': 1} and _lib.SADDLE_METHODS == {'cg': 0, 'bicgstab': 1, 'minres': 2}
    assert sorted(k for k in _lib.BREAKDOWNS if k) == [1, 2, 3, 4, 5]
    src = open(os.path.join(ROOT, 'pyiga_amd', 'csrc', 'solve_gmres.hip')).read()
    assert int(re.search(r'constexpr int MB = (\d+);', src).group(1)) == oc.MB
    assert int(re.search(r'constexpr int GM_MAX_RESTART = (\d+);', src).group(1)) == solvers.OseenSystem.MAX_RESTART
    assert oc.dot_blocks(10 ** 7) * (oc.RESTART + 1) + oc.NB_VEC <= 2 * sc.NB_SPMV_MAX


if __name__ == '__main__':
    cache = {}

    def gold(n):
        if n not in cache:
            cache[n] = np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_%s.npz' % n))
        return cache[n]
    print('MODEL = {')
    for key in oc.MODEL:
        name, tri, restart, tol = key
        S = oc.system(gold, name)
        u, info = oc.model_solve(S, orc, tri, restart, tol)
        print("    (%r, %r, %r, %.0e): (%d, %d, %.2e, %.2e)," % (name, tri, restart, tol, info['iterations'], info['restarts'], _err(u, S.u),
                                                                 info['relres']))
    print('}\nMODEL_STOKES = {')
    for base, which in oc.MODEL_STOKES:
        u, info = oc.model_stokes(gold, orc, base, which, restart=128)
        print("    (%r, %r): (%d, %.2e, %.2e)," % (base, which, info['iterations'], _err(u, sc.system(gold, base).u), info['relres']))
    print('}')
    for name in oc.CASES:
        S = oc.system(gold, name)
        print('%s: nu = %g, amp = %.2f, golden model steps %d' % (name, S.nu, S.amp, int(gold('oseen')[name + '_model_steps'])))

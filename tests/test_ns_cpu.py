"""The stationary Navier-Stokes solver without a device: the host model (tests/_ns_model.py) against the goldens of the reference
(tests/golden/golden_ns*.npz), the tolerance T of the device runs measured on the model, the table rule against tforms.evaluate,
the refusals that need no device, the bookkeeping of the loop and the new symbols of the ABI.

``python3 tests/test_ns_cpu.py`` prints the measured deviations in the form _ns_model.py records them."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import _ns_model as nm          # noqa: E402

from pyiga_amd import solvers, tforms      # noqa: E402

NEW_NAMES = ('igx_patch_eval_vspline_d', 'igx_patch_set_form_sum_d', 'igx_solver_replace_block', 'igx_solver_hide_block',
             'igx_solver_saddle_residual_d', 'igx_solver_saddle_correct_d')


@pytest.fixture(scope='module')
def cases(golden, oracle):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = nm.Case(golden, oracle, name)
        return cache[name]
    return get


@pytest.fixture(scope='module')
def exact_runs(cases):
    """The model with exact solves from the golden Stokes start, computed once per (case, method)."""
    cache = {}

    def get(name, method):
        if (name, method) not in cache:
            c = cases(name)
            cache[(name, method)] = c.run(method, c.iterates(method)[0][0], c.solve_exact)
        return cache[(name, method)]
    return get


def _rel(A, B):
    D = abs(A - B)
    return (D.max() if D.nnz else 0.0) / abs(B).max()


@pytest.mark.parametrize('tag', ['stokes', 'rand'])
@pytest.mark.parametrize('name', nm.CASES)
def test_model_matrices_match_the_reference(name, tag, cases, golden):
    c = cases(name)
    x = c.iterates('picard')[0][0] if tag == 'stokes' else c.random_wind(golden)
    for which, M in (('conv', c.conv(x)), ('newt', c.newt(x))):
        e = _rel(M, c.golden_matrix(golden, which, tag))
        print('%s A_%s at the %s wind: %.2e' % (name, which, tag, e))
        assert e <= 1e-12


@pytest.mark.parametrize('method', nm.METHODS)
@pytest.mark.parametrize('name', nm.CASES)
def test_model_reproduces_the_golden_iterates(name, method, cases, exact_runs):
    c = cases(name)
    gold, norms = c.iterates(method)
    its, info = exact_runs(name, method)
    assert info['converged'] and info['iterations'] == nm.GOLDEN_STEPS[(name, method)] == gold.shape[0] - 1
    assert its.shape == gold.shape
    err = max(abs(a - b).max() / abs(b).max() for a, b in zip(its, gold))
    print('%s %s: %d steps, iterates within %.2e, residual norms %.3e -> %.3e' % (name, method, info['iterations'], err, norms[0], norms[-1]))
    assert err <= 1e-10
    # (a residual carries the rounding of b - K x, some eps max(|K| |x|): below 1e-12 of the first norm on these cases)
    assert np.allclose(info['residual_norms'][:-1], norms[:-1], rtol=1e-6, atol=1e-12 * norms[0])
    assert info['blocks_assembled'] == nm.blocks_assembled(c.nc, method, info['iterations'])


def _deviation(c, method, exact):
    x0, s = c.stokes(c.solve_model)
    assert s['converged'] and s['restarts'] == 0
    its, info = c.run(method, x0, c.solve_model)
    assert info['converged'] and info['iterations'] == exact[1]['iterations']
    assert all(s['converged'] and s['restarts'] == 0 and s['iterations'] <= nm.RESTART for s in info['solves'])
    return max(abs(a - b).max() / abs(b).max() for a, b in zip(its, exact[0]))


@pytest.mark.parametrize('method', nm.METHODS)
@pytest.mark.parametrize('name', nm.CASES)
def test_tolerance_of_the_device_runs(name, method, cases, exact_runs):
    """T: every linear solve stopped at lin_tol = 1e-10 against exact solves.  The recorded deviation is not exceeded by more than
    a factor of 2 (the stop of a Krylov solve may shift by a step between BLAS builds), and T is 10 times the largest."""
    dev = _deviation(cases(name), method, exact_runs(name, method))
    print("    (%r, %r): %.2e," % (name, method, dev))
    assert dev <= 2 * nm.MEASURED_DEVIATION[(name, method)]
    assert nm.T == 10 * max(nm.MEASURED_DEVIATION.values())


@pytest.mark.parametrize('d', [2, 3])
def test_table_rule_against_the_form_strings(d):
    """The tables the device forms from the wind arrays are those tforms.evaluate gives for the two form strings at sampled
    winds.  tforms does not differentiate an input, so the Newton string is evaluated with grad(w) given as its sampled values."""
    rng = np.random.default_rng(d)
    G = (3, 4) if d == 2 else (2, 3, 2)
    X = rng.uniform(size=G + (d,))
    w = rng.standard_normal(G + (d,))
    gw = rng.standard_normal(G + (d, d))
    bf = [('u', d), ('v', d)]
    for form, inputs, rule in (('grad(u).dot(w).dot(v) * dx', dict(w=w), nm.conv_tables([w[..., j] for j in range(d)], d)),
                               ('gw.dot(u).dot(v) * dx', dict(gw=gw), nm.newt_tables([[gw[..., p, q] for q in range(d)] for p in range(d)], d))):
        arity, measure, table, ncs = tforms.evaluate(form, G, X, inputs, bf)
        assert (arity, measure, tuple(ncs)) == (2, 'dx', (d, d))
        for p in range(d):
            for q in range(d):
                for r in range(d + 1):
                    for s in range(d + 1):
                        mine = None if rule[p][q] is None else rule[p][q][r][s]
                        theirs = table[p][q][r][s]
                        assert (mine is None) == (theirs is None), (form, p, q, r, s)
                        if mine is not None:
                            assert np.array_equal(mine, theirs), (form, p, q, r, s)


def test_value_errors_before_any_device_work():
    S = object.__new__(solvers.NavierStokesSystem)          # (no constructor: nothing exists on a device)
    S.n = 10
    with pytest.raises(ValueError, match='unknown method'):
        S.solve(method='fixpoint')
    with pytest.raises(ValueError, match='picard_steps'):
        S.solve(method='newton', picard_steps=-1)
    with pytest.raises(ValueError, match='picard_steps'):
        S.solve(method='newton', picard_steps=1.5)
    with pytest.raises(ValueError, match='x0 has 9 entries'):
        S.solve(x0=np.zeros(9))
    from pyiga_amd import bspline
    kv = bspline.make_knots(2, 0.0, 1.0, 2)
    with pytest.raises(ValueError, match='as many velocity components as dimensions'):
        solvers.NavierStokesSystem(((kv, kv), (kv, kv)), None, None, ncomp=3)
    with pytest.raises(ValueError, match='kvs=\\(kvs_u, kvs_p\\)'):
        solvers.NavierStokesSystem((kv, kv), None, None)


@pytest.mark.parametrize('method,picard_steps', [('picard', 0), ('newton', 0), ('newton', 2)])
def test_bookkeeping_of_the_loop(method, picard_steps):
    """The callbacks of solvers.newton_loop in the order NavierStokesSystem.solve gives them, on a made-up residual sequence: the
    target is tested before every step, the Jacobian callback runs before every update, and the block count is
    _ns_model.blocks_assembled's."""
    norms = [1.0, 0.3, 0.05, 1e-4, 1e-9, 1e-13]
    nc, log, inner, count = 3, [], [], [0]

    def residual():
        log.append('r')
        count[0] += nc
        return norms[len(inner)]

    def jacobian():
        log.append('j')
        if method == 'newton' and len(inner) >= picard_steps:
            count[0] += nc * nc

    def update():
        log.append('u')
        inner.append(7)
        return 7
    conv, info = solvers.newton_loop(residual, jacobian, update, 0.0, 1e-10, 50, 1)
    assert conv and info['iterations'] == 5 and info['residual_norms'] == norms and info['target'] == 1e-10
    assert ''.join(log) == 'r' + 'jur' * 5
    assert count[0] == nm.blocks_assembled(nc, method, 5, picard_steps)
    conv, info = solvers.newton_loop(lambda: 1.0, lambda: None, lambda: 1, 0.0, 1e-10, 3, 1)
    assert not conv and info['iterations'] == 3
    e = solvers.NoConvergenceError('picard', 3, np.arange(4.0))
    assert (e.method, e.num_iter) == ('picard', 3) and np.array_equal(e.last_iterate, np.arange(4.0))


def test_new_symbols_are_declared():
    with open(os.path.join(ROOT, 'include', 'igx.h')) as f:
        header = f.read()
    with open(os.path.join(ROOT, 'pyiga_amd', '_lib.py')) as f:
        lib = f.read()
    for name in NEW_NAMES:
        assert re.search(r'\b%s\(' % name, header), name
        assert "('%s'," % name in lib, name
    assert hasattr(solvers, 'NavierStokesSystem') and hasattr(solvers.OseenSystem, 'update')
    for attr in ('solve', 'residual', 'split', 'close'):
        assert callable(getattr(solvers.NavierStokesSystem, attr))


if __name__ == '__main__':
    from oracle import iga_oracle as orc
    orc.build()
    cache = {}

    def gold(name):
        if name not in cache:
            cache[name] = np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_%s.npz' % name))
        return cache[name]
    print('MEASURED_DEVIATION = {')
    devs = []
    for name in nm.CASES:
        c = nm.Case(gold, orc, name)
        for method in nm.METHODS:
            exact = c.run(method, c.iterates(method)[0][0], c.solve_exact)
            devs.append(_deviation(c, method, exact))
            print("    (%r, %r): %.2e," % (name, method, devs[-1]))
    print('}\nT = 10 * %.2e' % max(devs))

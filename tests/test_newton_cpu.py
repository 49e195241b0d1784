"""Newton's method on the device, the parts that need no GPU: the numpy model (tests/_newton_model.py) against the golden iterates
of the reference, the sensitivity measurement behind the tolerance T of the GPU tests, tracing of the form strings into C tables
in x, y, z, f0 .., the host-only compilation of the generated kernel with inputs, the refusals (raised before any device work),
and the stopping rule and freeze_jac bookkeeping of the driver."""
import ctypes as C

import numpy as np
import pytest

from pyiga_amd import _lib, assemble, bspline, forms, geometry, symbolic

import _newton_model as model
from _newton_model import RES_CUBIC, JAC_CUBIC, RES_BURG, JAC_BURG


@pytest.fixture(scope='module')
def problems():
    return {case: model.Problem(case) for case in model.CASES}


@pytest.mark.parametrize('case', sorted(model.CASES))
def test_model_assembles_what_the_reference_assembles(case, problems, golden):
    """F and J of the numpy model against the reference's, at x0 and at the non-smooth random w."""
    g, prob = golden('newton'), problems[case]
    for tag, x in (('x0', g[case + 'x0']), ('rand', g[case + 'w_rand'])):
        F = g[case + 'F_' + tag]
        assert abs(prob.F(x) - F).max() <= 1e-12 * abs(F).max()
        if case + 'J_indptr' in g.files:
            import scipy.sparse
            J = scipy.sparse.csr_matrix((g[case + 'J_%s_data' % tag], g[case + 'J_indices'], g[case + 'J_indptr']), shape=(prob.n, prob.n))
            assert abs(prob.J(x) - J.toarray()).max() <= 1e-12 * abs(J).max()


@pytest.mark.parametrize('case,freeze', model.RUNS)
def test_model_reproduces_the_golden_iterates(case, freeze, problems, golden):
    g, prob = golden('newton'), problems[case]
    key = model.run_key(case, freeze)
    gold, gnorms = g[key + 'iterates'], g[key + 'norms']
    assert 3 <= len(gold) - 1 <= 10
    assert np.linalg.norm(gold[-1] - gold[-2]) < 1e-11 * np.linalg.norm(gold[-1])
    its, norms, ok = model.newton(prob, g[case + 'bc_idx'], g[case + 'x0'], 1e-12 * gnorms[0], 0.0, 20, freeze)
    assert ok and len(its) == len(gold), 'the reference\'s number of iterations'
    assert abs(np.array(its) - gold).max() <= 1e-10 * abs(gold).max()
    assert np.allclose(norms[:-1], gnorms[:-1], rtol=1e-6, atol=1e-12 * gnorms[0])


def test_sensitivity_to_the_linear_solves(golden):
    """What a relative residual of 1e-10 in every linear solve does to the golden runs: the measurement behind T."""
    s = model.measure_sensitivity(golden('newton'))
    print('sensitivity measured: %.2e (recorded %.2e, T = %.2e)' % (s, model.SENSITIVITY_MEASURED, model.T))
    assert 0.0 < s <= model.SENSITIVITY_MEASURED
    assert model.T == min(10 * model.SENSITIVITY_MEASURED, 1e-6)


def _space(d, p=2, n=3):
    kvs = tuple(bspline.make_knots(p, 0.0, 1.0, n) for _ in range(d))
    return kvs, bspline.BSplineFunc(kvs, np.zeros(tuple(kv.numdofs for kv in kvs)))


def f2(x, y):
    return np.sin(x) * y


def f3(x, y, z):
    return np.sin(x) * y + z


def _table(form, d, **inputs):
    slots = symbolic.FieldSlots(d)
    return forms.symbolic_table(form, d, inputs, fields=slots), slots.slots


def _jet(form, d, **inputs):
    slots = symbolic.FieldSlots(d)
    jet = forms.functional_jet(form, (1,) * d, symbolic.coordinates(d), inputs, traced=True, fields=slots)
    return [None if e is None else symbolic.c_source(e) for e in jet], slots.slots


def test_jacobian_strings_give_the_hand_written_tables():
    _, w2 = _space(2)
    _, w3 = _space(3)
    t, slots = _table(JAC_CUBIC, 2, w=w2)
    assert t == [['((f0 * f0) * 3.0)', None, None], [None, '1.0', None], [None, None, '1.0']] and slots == [('w', 0)]
    t, slots = _table(JAC_CUBIC, 3, w=w3)
    assert t == [['((f0 * f0) * 3.0)', None, None, None], [None, '1.0', None, None], [None, None, '1.0', None], [None, None, None, '1.0']]
    assert slots == [('w', 0)]
    # P[r][s]: r the jet index of v, s of u; w * d/dx u * v is entry (0, 1), d/dx w * u * v entry (0, 0)
    t, slots = _table(JAC_BURG, 2, w=w2, nu=0.1)
    assert t == [['f1', 'f0', None], [None, '0.1', None], [None, None, '0.1']]
    assert slots == [('w', 0), ('w', 1), ('w', 2)]


def test_residual_strings_give_the_hand_written_jets():
    _, w2 = _space(2)
    _, w3 = _space(3)
    j, slots = _jet(RES_CUBIC, 2, w=w2, f=f2)
    assert j == ['(((f0 * f0) * f0) + ((sin(x) * y) * (-1.0)))', 'f1', 'f2'] and slots == [('w', 0), ('w', 1), ('w', 2)]
    j, slots = _jet(RES_CUBIC, 3, w=w3, f=f3)
    assert j == ['(((f0 * f0) * f0) + (((sin(x) * y) + z) * (-1.0)))', 'f1', 'f2', 'f3']
    assert slots == [('w', 0), ('w', 1), ('w', 2), ('w', 3)]
    j, slots = _jet(RES_BURG, 2, w=w2, f=f2, nu=0.1)
    assert j == ['((f0 * f1) + ((sin(x) * y) * (-1.0)))', '(f1 * 0.1)', '(f2 * 0.1)']


def test_grad_of_an_expression_in_the_input_is_refused():
    _, w2 = _space(2)
    with pytest.raises(NotImplementedError):
        _table('(inner(grad(w*w), grad(v)) * u) * dx', 2, w=w2)
    with pytest.raises(NotImplementedError):                      # without the slots there is no sampled path
        forms.symbolic_table(JAC_CUBIC, 2, dict(w=w2))


def _compile(exprs, m):
    lib = _lib.load()
    arr = (C.c_char_p * len(exprs))(*[e.encode() for e in exprs])
    path = C.create_string_buffer(512)
    hit = C.c_int(-1)
    rc = lib.igx_rtc_compile_exprs_inputs(len(exprs), arr, m, b'gfx950', path, 512, C.byref(hit))
    return rc, hit.value, path.value.decode()


def test_generated_kernel_with_inputs_compiles_and_is_cached(tmp_path, monkeypatch):
    monkeypatch.setenv('IGX_CACHE_DIR', str(tmp_path / 'cache'))
    exprs = ['((f0 * f0) * 3.0)', 'f1 * x + sin(pi * y)']
    rc, hit, path = _compile(exprs, 2)
    assert rc == _lib.IGX_OK and hit == 0, _lib.last_error()
    assert path.startswith(str(tmp_path / 'cache')) and open(path, 'rb').read(4) == b'\x7fELF'
    rc, hit2, path2 = _compile(exprs, 2)
    assert rc == _lib.IGX_OK and hit2 == 1 and path2 == path
    rc, hit3, path3 = _compile(exprs, 3)                          # m is part of the source: another code object
    assert rc == _lib.IGX_OK and hit3 == 0 and path3 != path
    for bad in ('f0; f1', 'f0 } + { f1', 'f0 // f1', 'f0 \\\n f1'):
        assert _compile([bad], 2)[0] == _lib.IGX_ERR_ARG
    assert _compile(['f0'], 17)[0] == _lib.IGX_ERR_ARG
    assert _compile(['f2'], 2)[0] == _lib.IGX_ERR_COMPILE         # f2 is not in scope with two inputs


def test_refusals_name_their_case_before_any_device_work(monkeypatch):
    kvs, w = _space(2)
    geo = geometry.unit_square()
    # (no patch may be created: the refusals come first)
    from pyiga_amd import assemblers
    monkeypatch.setattr(assemblers.DevicePatch, '__init__', lambda *a, **k: pytest.fail('device work before the refusal'))
    vec = bspline.BSplineFunc(kvs, np.zeros(tuple(kv.numdofs for kv in kvs) + (2,)))
    with pytest.raises(NotImplementedError, match='vector-valued'):
        assemble.assemble('inner(w, grad(u)) * v * dx', kvs, geo=geo, w=vec)
    with pytest.raises(NotImplementedError, match='bfuns'):
        assemble.assemble('w * inner(u, v) * dx', kvs, geo=geo, w=w, bfuns=[('u', 2), ('v', 2)])
    with pytest.raises(NotImplementedError, match='boundary'):
        assemble.assemble('w * u * v * ds', kvs, geo=geo, w=w, boundary='left')
    with pytest.raises(NotImplementedError, match='second or parametric'):
        assemble.assemble('w * inner(hess(u), hess(v)) * dx', kvs, geo=geo, w=w)
    with pytest.raises(ValueError):
        assemble.Assembler(JAC_CUBIC, kvs, geo=geo, w=w, updatable=['q'])


def test_newton_loop_bookkeeping():
    """Stopping rule and freeze_jac of the driver (pyiga/solvers.py:335-361) with the device calls replaced by a scalar model:
    F(x) = x**2 - 2, Newton from x = 3."""
    from pyiga_amd import solvers

    def run(atol, rtol, maxiter, freeze):
        st = dict(x=3.0, J=None, nJ=0)

        def form():
            st['J'] = 2.0 * st['x']
            st['nJ'] += 1

        def update():
            st['x'] -= (st['x'] ** 2 - 2.0) / st['J']
            return 1
        ok, info = solvers.newton_loop(lambda: abs(st['x'] ** 2 - 2.0), form, update, atol, rtol, maxiter, freeze)
        return ok, info, st
    ok, info, st = run(1e-12, 0.0, 50, 1)
    assert ok and abs(st['x'] - 2.0 ** 0.5) < 1e-12 and info['jacobians'] == info['iterations'] == st['nJ'] == len(info['inner_iterations'])
    assert len(info['residual_norms']) == info['iterations'] + 1 and info['residual_norms'][-1] < 1e-12 <= info['residual_norms'][-2]
    ok2, info2, _ = run(1e-12, 0.0, 50, 2)
    assert ok2 and info2['iterations'] > info['iterations'] and info2['jacobians'] == (info2['iterations'] + 1) // 2
    ok3, info3, _ = run(0.0, 1e-3, 50, 1)                        # relative to the first residual, 7
    assert ok3 and info3['target'] == 7e-3 and info3['residual_norms'][-1] < 7e-3 <= info3['residual_norms'][-2]
    ok4, info4, _ = run(1e-12, 0.0, 2, 1)                         # the test comes BEFORE each step: two steps, no verdict on the last
    assert not ok4 and info4['iterations'] == 2
    ok5, info5, _ = run(10.0, 0.0, 5, 1)                          # converged at the start: no Jacobian at all
    assert ok5 and info5['iterations'] == 0 and info5['jacobians'] == 0
    with pytest.raises(ValueError):
        run(1e-12, 0.0, 5, 0)
    e = solvers.NoConvergenceError('newton', 3, np.zeros(2))
    assert (e.method, e.num_iter) == ('newton', 3) and e.last_iterate.shape == (2,)

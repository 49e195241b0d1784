"""solvers.NewtonSystem and the spline-function inputs behind it against the real reference (tests/golden/golden_newton.npz,
made by tests/golden/make_golden_newton.py): the assembled F and J at x0 and at a non-smooth random w, the updatable Assembler,
and every Newton iterate of the three cases -- cubic2_ (p = 3, 16 spans, quarter annulus, CG), cubic3_ (p = 2, 6 spans, annulus
cylinder, CG), burg2_ (nu = 0.1, grad(w) in the coefficients, BiCGStab) -- within T of the golden one, T from the measured
sensitivity of the runs to linear solves of relative residual 1e-10 (tests/_newton_model.py).

The manufactured problem: on the identity map with u_exact a polynomial of degree <= p per variable, f = -laplace(u_exact) +
u_exact**3 and g = u_exact, the discrete problem has u_exact's coefficients as its solution EXACTLY -- u**3 - f is evaluated
point by point, so the cubic terms cancel at every Gauss point, and the remaining integrands have degree <= 2 p - 1 per variable,
which the p + 1 Gauss points integrate exactly.  Its tolerance is the 1e-9 (relative to the largest entry) of the solves of
test_solve_gpu.py."""
import numpy as np
import pytest
import scipy.sparse

from pyiga_amd import assemble, bspline, geometry, solvers

import _newton_model as model
from _newton_model import RES_CUBIC, JAC_CUBIC
from conftest import rel_maxdiff

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return abs(np.asarray(a).ravel() - np.asarray(b).ravel()).max() / abs(np.asarray(b)).max()


def _space(case):
    dim, p, n = model.CASES[case][:3]
    kvs = dim * (bspline.make_knots(p, 0.0, 1.0, n),)
    geo = geometry.quarter_annulus() if dim == 2 else geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.quarter_annulus())
    return kvs, geo


def _golden_J(g, case, tag, n):
    return scipy.sparse.csr_matrix((g[case + 'J_%s_data' % tag], g[case + 'J_indices'], g[case + 'J_indptr']), shape=(n, n))


# ---- 1. assembly parity with the reference
@pytest.mark.parametrize('case', sorted(model.CASES))
def test_assembly_parity_with_the_reference(case, golden):
    g = golden('newton')
    kvs, geo = _space(case)
    res, jac, extra = model.forms(case)
    f = model.CASES[case][4]
    N = tuple(kv.numdofs for kv in kvs)
    for tag, x in (('x0', g[case + 'x0']), ('rand', g[case + 'w_rand'])):
        w = bspline.BSplineFunc(kvs, x.reshape(N))
        F = assemble.assemble(res, kvs, geo=geo, w=w, f=f, **extra)
        err = _rel(F, g[case + 'F_' + tag])
        print('%s F(%s): %.2e' % (case, tag, err))
        assert err <= 1e-12
        if case + 'J_indptr' in g.files:
            J = assemble.assemble(jac, kvs, geo=geo, w=w, **extra)
            errJ = rel_maxdiff(J, _golden_J(g, case, tag, x.size))
            print('%s J(%s): %.2e' % (case, tag, errJ))
            assert errJ <= 1e-12


# ---- 2. the updatable Assembler
@pytest.mark.parametrize('case', ['cubic2_', 'burg2_'])
def test_updatable_assembler_gives_the_golden_matrix_of_the_second_w(case, golden):
    g = golden('newton')
    kvs, geo = _space(case)
    res, jac, extra = model.forms(case)
    N = tuple(kv.numdofs for kv in kvs)
    asm = assemble.Assembler(jac, kvs, geo=geo, w=bspline.BSplineFunc(kvs, g[case + 'x0'].reshape(N)), updatable=['w'], **extra)
    assert rel_maxdiff(asm.assemble(), _golden_J(g, case, 'x0', g[case + 'x0'].size)) <= 1e-12
    dev, patch, handle = asm.asm, asm.asm.patch, asm.asm.patch.handle
    A2 = asm.assemble(w=bspline.BSplineFunc(kvs, g[case + 'w_rand'].reshape(N)))
    assert asm.asm is dev and asm.asm.patch is patch and patch.handle == handle, 'the same device assembler and patch'
    assert asm.asm.coeff_cache_hit is True
    assert rel_maxdiff(A2, _golden_J(g, case, 'rand', g[case + 'x0'].size)) <= 1e-12
    with pytest.raises(RuntimeError):
        asm.update(f=1.0)


# ---- 3. the Newton iterates of the reference
@pytest.fixture(scope='module')
def systems(golden):
    made = {}

    def get(case):
        if case not in made:
            g = golden('newton')
            kvs, geo = _space(case)
            res, jac, extra = model.forms(case)
            made[case] = solvers.NewtonSystem(kvs, geo, res, jac, (g[case + 'bc_idx'], g[case + 'bc_val']), f=model.CASES[case][4], **extra)
        return made[case]
    yield get
    for S in made.values():
        S.close()


def _solve(S, g, case, freeze=1, **kw):
    iterates = [None]
    nF0 = g[model.run_key(case, freeze) + 'norms'][0]
    x = S.solve(x0=g[case + 'x0'], atol=1e-12 * nF0, rtol=0.0, freeze_jac=freeze, callback=lambda k, xk: iterates.append(xk), **kw)
    iterates[0] = g[case + 'x0']
    return x, iterates


@pytest.mark.parametrize('case,freeze', model.RUNS)
def test_newton_iterates_follow_the_reference(case, freeze, systems, golden):
    g, S = golden('newton'), systems(case)
    key = model.run_key(case, freeze)
    gold, gnorms = g[key + 'iterates'], g[key + 'norms']
    x, iterates = _solve(S, g, case, freeze)
    info = S.info
    dev = [abs(a - b).max() / abs(gold).max() for a, b in zip(iterates, gold)]
    print('%s freeze %d: %d steps (reference %d), method %s / %s, inner %s, deviation per iterate %s (T %.1e)' % (
        case, freeze, info['iterations'], len(gold) - 1, info['method'], info['precond'], info['inner_iterations'],
        ' '.join('%.1e' % d for d in dev), model.T))
    assert info['converged'] and info['iterations'] == len(gold) - 1, 'the reference\'s number of iterations'
    assert info['method'] == ('bicgstab' if case == 'burg2_' else 'cg') and S.symmetric == (case != 'burg2_')
    assert len(iterates) == len(gold) and max(dev) <= model.T
    assert np.array_equal(x, iterates[-1])
    assert info['jacobians'] == (info['iterations'] + freeze - 1) // freeze
    assert np.allclose(info['residual_norms'][:-1], gnorms[:-1], rtol=1e-6, atol=1e-12 * gnorms[0])


# ---- 4. a manufactured solution on the identity map
def _interpolate(kvs, fn):
    """Coefficients of a function of the spline space: interpolation at the Greville points (exact on the space)."""
    grev = [kv.greville() for kv in kvs]
    c = fn(*np.meshgrid(*grev, indexing='ij')[::-1])            # fn(x, y[, z]), x belonging to the last axis
    for k in range(len(kvs)):
        Ck = np.asarray(bspline.collocation(kvs[k], grev[k]).todense())
        c = np.moveaxis(np.tensordot(np.linalg.inv(Ck), c, axes=(1, k)), 0, k)
    return c


@pytest.mark.parametrize('dim', [2, 3])
def test_manufactured_solution_is_reproduced(dim):
    if dim == 2:
        kvs = (bspline.make_knots(2, 0.0, 1.0, 6), bspline.make_knots(3, 0.0, 1.0, 5))
        geo = geometry.unit_square()
        uex = lambda x, y: 1.0 + x * x * (1.0 - 0.5 * y) + 0.3 * y * y - x * y
        lap = lambda x, y: 2.0 * (1.0 - 0.5 * y) + 0.6
    else:
        kvs = 3 * (bspline.make_knots(2, 0.0, 1.0, 4),)
        geo = geometry.unit_cube()
        uex = lambda x, y, z: 1.0 + x * x * z - 0.5 * y * y + x * y * z
        lap = lambda x, y, z: 2.0 * z - 1.0
    f = lambda *X: -lap(*X) + uex(*X) ** 3
    c = _interpolate(kvs, uex)
    S = solvers.NewtonSystem(kvs, geo, RES_CUBIC, JAC_CUBIC, assemble.compute_dirichlet_bcs(kvs, geo, ('all', uex)), f=f)
    try:
        x = S.solve(atol=1e-10, rtol=0.0, lin_tol=1e-12)
        rng = np.random.default_rng(3)
        w = rng.uniform(-1.0, 1.0, size=c.shape)
        w.ravel()[S.bc_indices] = S.bc_values                 # (residual() and jacobian() complete their argument with g)
        spl = bspline.BSplineFunc(kvs, w)
        assert _rel(S.residual(w), assemble.assemble(RES_CUBIC, kvs, geo=geo, w=spl, f=f)) <= 1e-13
        assert rel_maxdiff(S.jacobian(w), assemble.assemble(JAC_CUBIC, kvs, geo=geo, w=spl)) <= 1e-13
    finally:
        S.close()
    print('dim %d: %d Newton steps, ||R F|| %s, error %.2e' % (dim, S.info['iterations'], ' '.join('%.1e' % v for v in S.info['residual_norms']), _rel(x, c)))
    assert S.info['converged'] and S.info['method'] == 'cg' and S.info['precond'] == 'kron'
    assert _rel(x, c) <= 1e-9


# ---- 5. error handling, 6. determinism
def test_no_convergence_carries_the_first_iterate_and_solves_are_repeatable(systems, golden):
    g, S = golden('newton'), systems('cubic2_')
    gold = g['cubic2_iterates']
    x1, _ = _solve(S, g, 'cubic2_')
    with pytest.raises(solvers.NoConvergenceError) as e:
        _solve(S, g, 'cubic2_', maxiter=1)
    assert e.value.method == 'newton' and e.value.num_iter == 1
    assert abs(e.value.last_iterate - gold[1]).max() <= model.T * abs(gold).max()
    x2, _ = _solve(S, g, 'cubic2_')                           # the system solves again normally afterwards
    assert abs(x2 - gold[-1]).max() <= model.T * abs(gold).max()
    assert np.array_equal(x1, x2), 'two solves give bit-identical results'

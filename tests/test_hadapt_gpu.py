"""``HierarchicalSystem.error_norms`` / ``estimate`` against the host model applied level by level with the active-cell masks
(tests/_hadapt_model.py), and ``solvers.adaptive_solve`` against the same calls made one by one and against the model's loop.

(The file name: tests/test_adaptive_gpu.py belongs to the adaptive time steps of DESIGN.md section 18.)"""
import numpy as np
import pytest
import scipy.sparse

from pyiga_amd import approx, assemblers, bspline, geometry, hierarchical, solvers
from pyiga_amd.hierarchical import HSpace

import _hadapt_model as hm
import _hier_cases as hc
import _quad_model as qm
import _resid_model as rm

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
LIP_F = 3.0 * (1.3 + 0.7 + 0.9)            # of _f below: sum of the absolute partials


def _f(*X):
    v = np.sin(1.3 * X[0] + 0.2) * np.cos(0.7 * X[1])
    if len(X) == 3:
        v = v * np.cos(0.9 * X[2] + 0.1)
    return 3.0 * v


def _rules(hs, geo):
    """per level with active cells, the Gauss rule of a device patch of the level"""
    out = {}
    for lv in range(hs.numlevels):
        if hs._cact[lv].any():
            P = assemblers.DevicePatch(hs.knotvectors(lv), geo)
            rule = [P.gauss(k) for k in range(hs.dim)]
            P.close()
            out[lv] = ([r[0] for r in rule], [r[1] for r in rule])
    return out


def _system(name):
    hs, _ = hc.build(bspline, HSpace, name)
    geo = hc.geometry_of(geometry, hs.dim)
    return hs, geo, solvers.HierarchicalSystem(hs, hc.STIFF, None, geo=geo, f=_f)


@pytest.mark.parametrize('name', ['hb2', 'thb2inf', 'hb2d', 'hb3'])
def test_estimate_against_the_model(name):
    hs, geo, S = _system(name)
    try:
        u = np.random.default_rng(11).uniform(-1.0, 1.0, hs.numdofs)
        eta, eta2 = S.estimate(u)                                          # f: the system's own input
        elem, bound = hm.estimate_model(hs, geo, u, f=_f, f_lip=LIP_F, rules=_rules(hs, geo))
        assert eta2.shape == (hs.total_active_cells,)
        # eta_K^2 = V^(2/dim) R: relative errors (2/dim) dV / V + dR / R, and 4 EPS for the power and the product
        want = rm.eta2(elem, hs.dim)
        tol = want.astype(np.float64) * ((2.0 / hs.dim) * bound[1] / elem[1].astype(np.float64) + 4 * EPS) + \
            np.power(elem[1].astype(np.float64), 2.0 / hs.dim) * bound[0]
        err = abs(eta2 - want.astype(np.float64))
        print('%s: eta %.6e, worst err / bound %.2e' % (name, eta, (err / tol).max()))
        assert (err <= tol).all()
        assert eta == float(np.sqrt(eta2.sum()))
        eta_b, eta2_b = S.estimate(u, f=_f)
        assert eta_b == eta and np.array_equal(eta2_b, eta2), 'two calls with the same inputs differ'
    finally:
        S.close()


def _error_model(hs, geo, u, exact, rules):
    """per-cell error sums [2][ncells] and their bounds from _quad_model.error_model, level by level with the active masks"""
    u_hb = hm.hb_coeffs(hs, u)
    extra = 0.0
    if hs.truncate:
        T = scipy.sparse.csr_matrix(hs.thb_to_hb())
        extra = (int(np.diff(T.indptr).max()) + 2) * EPS * float(abs(T).dot(abs(u)).max())
    elems, bounds = [], []
    for lv in range(hs.numlevels):
        mask = hs._cact[lv]
        if not mask.any():
            continue
        kvs = hs.knotvectors(lv)
        c, c_err = hm.level_coeffs(hs, u_hb, lv)
        c_err += float(abs(scipy.sparse.csr_matrix(hs.level_restriction(lv))).sum(axis=1).max()) * extra + EPS * float(abs(c).max())
        nodes, weights = rules[lv]
        S = qm._S([qm.collocation_ld(kv, nd) for kv, nd in zip(kvs, nodes)])
        X, J, _ = qm.geometry_ld(geo, nodes)
        Jimax = float(abs(qm._det_inv(J)[1]).max())
        dv = c_err * float(np.prod([s[0] for s in S]))
        dg = c_err * max(float(np.prod([S[k][1 if k == r else 0] for k in range(hs.dim)])) for r in range(hs.dim)) * hs.dim * Jimax
        ex, d_ex = None, (0.0, 0.0)
        if exact:
            Xd = X.astype(np.float64)
            xs = [Xd[..., k] for k in range(hs.dim)]
            ex = [np.ascontiguousarray(np.broadcast_to(v, Xd.shape[:-1])) for v in (_f(*xs),) + tuple(_grad_f(*xs))]
            dX = qm.point_error(geo, nodes)
            d_ex = (LIP_F * dX, 1.3 * LIP_F * dX)                           # (a second partial of _f is at most 1.3 times a first)
        m = qm.error_model(kvs, geo, c.astype(np.float64), True, exact=ex, nodes=nodes, weights=weights, d_exact=(dv + d_ex[0], dg + d_ex[1]))
        elems.append(m['elem'][:, mask])
        bounds.append(m['elem_bound'][:, mask])
    return np.concatenate(elems, axis=1), np.concatenate(bounds, axis=1)


def _grad_f(*X):
    s0, c0 = np.sin(1.3 * X[0] + 0.2), np.cos(1.3 * X[0] + 0.2)
    c1, s1 = np.cos(0.7 * X[1]), np.sin(0.7 * X[1])
    if len(X) == 2:
        return (3.0 * 1.3 * c0 * c1, -3.0 * 0.7 * s0 * s1)
    c2, s2 = np.cos(0.9 * X[2] + 0.1), np.sin(0.9 * X[2] + 0.1)
    return (3.0 * 1.3 * c0 * c1 * c2, -3.0 * 0.7 * s0 * s1 * c2, -3.0 * 0.9 * s0 * c1 * s2)


@pytest.mark.parametrize('name', ['hb2', 'thb2inf', 'hb2d', 'hb3'])
def test_error_norms_against_the_model(name):
    hs, geo, S = _system(name)
    try:
        u = np.random.default_rng(12).uniform(-1.0, 1.0, hs.numdofs)
        rules = _rules(hs, geo)
        for exact in (False, True):
            got = S.error_norms(u, _f, _grad_f, elementwise=True) if exact else S.error_norms(u, elementwise=True)
            elem, bound = _error_model(hs, geo, u, exact, rules)
            for k in range(2):
                err = abs(got[k] - elem[k].astype(np.float64))
                print('%s exact=%s [%d]: worst err / bound %.2e' % (name, exact, k, (err / bound[k]).max()))
                assert got[k].shape == (hs.total_active_cells,) and (err <= bound[k]).all()
            tot = S.error_norms(u, _f, _grad_f) if exact else S.error_norms(u)
            assert tot == (float(np.sqrt(got[0].sum())), float(np.sqrt(got[1].sum())))
        l2, h1 = S.error_norms(u, _f)
        assert h1 is None and l2 == float(np.sqrt(S.error_norms(u, _f, elementwise=True)[0].sum()))
    finally:
        S.close()


def test_a_space_with_level_0_only_is_the_tensor_product_patch():
    """the per-cell arrays are the element arrays of approx.error_norms / residual_estimator, bit for bit (their totals are formed
    differently: a device tree there, the sum over the cells here)"""
    kvs = (bspline.make_knots(2, 0.0, 1.0, 5), bspline.make_knots(3, 0.0, 1.0, 4))
    hs = HSpace(kvs, bdspecs=[(a, s) for a in range(2) for s in (0, 1)])
    geo = geometry.bspline_quarter_annulus()
    S = solvers.HierarchicalSystem(hs, hc.STIFF, None, geo=geo, f=_f)
    try:
        u = np.random.default_rng(13).uniform(-1.0, 1.0, hs.numdofs)
        a = S.error_norms(u, _f, _grad_f, elementwise=True)
        b = approx.error_norms(kvs, geo, u, _f, _grad_f, elementwise=True)
        assert np.array_equal(a[0], b[0].ravel()) and np.array_equal(a[1], b[1].ravel())
        eta, eta2 = S.estimate(u)
        assert np.array_equal(eta2, approx.residual_estimator(kvs, geo, u, _f).ravel())
        l2, h1 = S.error_norms(u, _f, _grad_f)
        l2p, h1p = approx.error_norms(kvs, geo, u, _f, _grad_f)
        assert abs(l2 - l2p) <= a[0].size * EPS * l2p and abs(h1 - h1p) <= a[0].size * EPS * h1p
    finally:
        S.close()


def test_estimate_refuses_spaces_that_are_not_c1():
    for hs in (hc.build(bspline, HSpace, 'hb2p1')[0], hm.c0_line_space(bspline, HSpace)):
        S = solvers.HierarchicalSystem(hs, hc.STIFF, None, geo=hc.geometry_of(geometry, 2), f=_f)
        try:
            with pytest.raises(ValueError, match='jump'):
                S.estimate(np.zeros(hs.numdofs))
            assert S.error_norms(np.zeros(hs.numdofs))[0] == 0.0              # (the norms serve any space)
        finally:
            S.close()


def _loop_inputs(name, p):
    geo = geometry.unit_square() if name == 'square' else geometry.quarter_annulus()
    kv = bspline.make_knots(p, 0.0, 1.0, 8)
    hs0 = HSpace((kv, kv), truncate=False, bdspecs=[(a, s) for a in range(2) for s in (0, 1)])
    return geo, hs0, hm.problem(name), dict(tol=hm.SOLVER_TOL)


def _round(hs, geo, f, opts, exact=None):
    S = solvers.HierarchicalSystem(hs, hc.STIFF, None, geo=geo, f=f)
    try:
        u = S.solve(**opts)
        eta, eta2 = S.estimate(u)
        h1 = S.error_norms(u, *exact)[1] if exact else None
        return u, eta, eta2, h1, S.info['iterations']
    finally:
        S.close()


@pytest.mark.parametrize('p', [2, 3])
@pytest.mark.parametrize('name', ['square', 'annulus'])
def test_adaptive_loop_history_is_that_of_the_calls_one_by_one(name, p):
    """bit-equal eta2, equal marked sets and iteration counts (`solve_tol` is the linear solver's tolerance, `tol` the
    estimator's)"""
    geo, hs0, (u_ex, grad_ex, f), opts = _loop_inputs(name, p)
    cells0 = hs0.active_cells(flat=True)
    hs_end, u_end, hist = solvers.adaptive_solve(hs0, geo, f, theta=hm.THETA, max_rounds=hm.ROUNDS, solve_tol=opts['tol'])
    assert hs0.active_cells(flat=True) == cells0 and hs0.numlevels == 1, 'inplace=False leaves the space untouched'
    assert len(hist) == hm.ROUNDS and hist[-1]['marked'] == {} and u_end.shape == (hs_end.numdofs,)
    hs = hs0.copy()
    for rnd, rec in enumerate(hist):
        u, eta, eta2, _, its = _round(hs, geo, f, opts)
        assert rec['dofs'] == hs.numdofs and rec['cells'] == tuple(int(m.sum()) for m in hs._cact)
        print('%s p=%d round %d: eta %r in the history, %r one by one' % (name, p, rnd, rec['eta'], eta))
        assert rec['eta'] == eta and np.array_equal(rec['eta2'], eta2) and rec['iterations'] == its > 0
        if rnd < len(hist) - 1:
            marked = hierarchical.mark(hs, eta2, hm.THETA)
            assert rec['marked'] == marked
            hs.refine(marked, truncate=hs.truncate)
    assert hs.active_cells(flat=True) == hs_end.active_cells(flat=True)
    # inplace: the caller's space is the one refined
    hs_in = hs0.copy()
    got, _, _ = solvers.adaptive_solve(hs_in, geo, f, theta=hm.THETA, max_rounds=2, inplace=True, solve_tol=opts['tol'])
    assert got is hs_in and hs_in.numdofs == hist[1]['dofs']


@pytest.mark.parametrize('p', [2, 3])
@pytest.mark.parametrize('name', ['square', 'annulus'])
def test_adaptive_loop_against_the_model(name, p):
    """The marked sets are those of the host loop (tests/_hadapt_model.py; tests/test_resid_cpu.py keeps its Doerfler cut clear of
    its neighbours), and the H1 error falls from round to round (nested spaces).  The model forms the load vector as the device
    does: every level on its whole patch with the level's own rule.  The effectivity eta / |u - u_h|_H1 is
    printed, not asserted (DESIGN.md section 38 has the figures)."""
    geo, hs0, (u_ex, grad_ex, f), opts = _loop_inputs(name, p)
    model = hm.loop_model(hs0, geo, f, hm.THETA, hm.ROUNDS, hierarchical.mark)
    hs = hs0.copy()
    h1 = []
    for rnd in range(hm.ROUNDS):
        u, eta, eta2, err, _ = _round(hs, geo, f, opts, exact=(u_ex, grad_ex))
        h1.append(err)
        rel = abs(eta2 - model[rnd]['eta2']).sum() / model[rnd]['eta2'].sum()
        print('%s p=%d round %d: dofs %d, eta %.4e, |u - u_h|_H1 %.4e, effectivity %.3f, eta2 against the model (relative, summed) %.1e'
              % (name, p, rnd, hs.numdofs, eta, h1[-1], eta / h1[-1], rel))
        assert hs.numdofs == model[rnd]['dofs']
        if rnd < hm.ROUNDS - 1:
            marked = hierarchical.mark(hs, eta2, hm.THETA)
            assert marked == model[rnd]['marked']
            hs.refine(marked, truncate=hs.truncate)
    assert all(b < a for a, b in zip(h1, h1[1:])), 'nested spaces: the H1 error decreases from round to round'

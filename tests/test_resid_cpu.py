"""The residual estimator without a GPU: the host model (tests/_resid_model.py) is exact on polynomial data -- B-spline maps and a
rational net that represents a polynomial map, so that the quotient rule with its w' and w'' terms is exercised --,
``HSpace.level_restriction`` against the level-wise functions, ``hierarchical.mark`` on hand-made arrays, the case table against
the launch logic, and the Doerfler cut of the loop case (tests/test_hadapt_gpu.py compares marked sets exactly)."""
import os
import re
import types

import numpy as np
import pytest

from pyiga_amd import bspline, geometry, hierarchical, solvers
from pyiga_amd.hierarchical import HSpace

import _hadapt_model as hm
import _hier_cases as hc
import _resid_cases as rc
import _resid_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = rm.LD


def _affine(dim):
    """x -> A x + b on the unit cube as a degree-1 single-span B-spline map (grid axis k <-> coordinate dim - 1 - k)"""
    A = np.array([[1.5, 0.3, -0.2], [0.4, 0.9, 0.1], [-0.3, 0.2, 1.2]])[:dim, :dim]
    b = np.array([0.5, -1.0, 2.0])[:dim]
    kv = bspline.make_knots(1, 0.0, 1.0, 1)
    net = np.zeros((2,) * dim + (dim,))
    for idx in np.ndindex(*(2,) * dim):
        net[idx] = A @ np.array(idx[::-1], dtype=float) + b
    return bspline.BSplineFunc((kv,) * dim, net)


def _polynomial_geometries():
    return {'identity2': geometry.unit_square(), 'identity3': geometry.unit_cube(), 'affine2': _affine(2), 'affine3': _affine(3),
            'twisted_box': geometry.twisted_box(), 'bspline_quarter_annulus': geometry.bspline_quarter_annulus()}


def _space_for(geo, spans=2):
    """knot vectors whose degree holds |G|^2 for the single-span polynomial map `geo`, on `spans` spans per axis"""
    return tuple(bspline.make_knots(max(2, 2 * int(kv.p)), 0.0, 1.0, spans) for kv in geo.kvs)


def _interpolation_nodes(kvs):
    return [np.linspace(0.0, 1.0, kv.numdofs) for kv in kvs]


def _check_exact(kvs, geo):
    dim = len(kvs)
    nodes = _interpolation_nodes(kvs)
    X = rm.geometry2_ld(geo, nodes)[0]
    c = rm.interpolate_ld(kvs, (X * X).sum(-1), nodes)                    # u = |x|^2: Lap u = 2 dim
    m0 = rm.residual_model(kvs, geo, c)
    assert float(abs(m0['lap'] - 2 * dim).max()) < 1e-13                  # (long double: 1e-19 times dofs of O(10) and second-derivative tables of O(1e3))
    vol = float(m0['total'][1])
    assert abs(float(m0['total'][0]) - 4 * dim * dim * vol) < 1e-12 * 4 * dim * dim * vol
    assert np.allclose(m0['elem'][0].astype(float), 4 * dim * dim * m0['elem'][1].astype(float), rtol=1e-12, atol=0)
    f = np.full(m0['lap'].shape, -2.0 * dim)
    m1 = rm.residual_model(kvs, geo, c, f=f)
    assert float(m1['total'][0]) < 1e-26 * vol                            # eta = 0 to rounding: the square of residuals below 1e-13
    assert float(rm.eta2(m1['elem'], dim).max()) < 1e-20
    return m0


def m0_nodes(kvs):
    q = max(int(kv.p) for kv in kvs) + 1
    return [rm.gauss_rule(kv, q)[0] for kv in kvs]


@pytest.mark.parametrize('name', sorted(_polynomial_geometries()))
def test_model_is_exact_on_polynomial_geometries(name):
    geo = _polynomial_geometries()[name]
    _check_exact(_space_for(geo), geo)


@pytest.mark.parametrize('name', ['bspline_quarter_annulus', 'twisted_box'])
def test_model_is_exact_on_a_rational_net_of_a_polynomial_map(name):
    """homogeneous numerator w P, weight w of degree 1 in every direction: the map equals P, the quotient rule does the work"""
    P = _polynomial_geometries()[name]
    dim = len(P.kvs)
    kvs_g = tuple(bspline.make_knots(int(kv.p) + 1, 0.0, 1.0, 1) for kv in P.kvs)
    nodes = _interpolation_nodes(kvs_g)
    X = rm.geometry2_ld(P, nodes)[0]
    grid = np.meshgrid(*[np.asarray(n, dtype=LD) for n in nodes], indexing='ij')
    w = 1 + sum(LD(0.3 + 0.2 * k) * g for k, g in enumerate(grid))       # positive, degree 1
    net = np.concatenate((rm.interpolate_ld(kvs_g, w[..., None] * X, nodes), rm.interpolate_ld(kvs_g, w, nodes)[..., None]), axis=-1)
    R = types.SimpleNamespace(kvs=kvs_g, coeffs=net)
    kvs = _space_for(P)
    # the rational map IS P: same points, Jacobians and second derivatives
    gn = m0_nodes(kvs)
    a, b = rm.geometry2_ld(R, gn), rm.geometry2_ld(P, gn)
    for k in range(3):
        assert float(abs(a[k] - b[k]).max()) < 1e-15 * max(1.0, float(abs(b[k]).max()))
    assert float(abs(rm.geometry2_ld(R, gn)[2]).max()) > 0.1             # (second derivatives are there to be got wrong)
    _check_exact(kvs, R)


@pytest.mark.parametrize('name', list(hc.CASES))
def test_level_restriction_gives_the_function_on_the_active_cells(name):
    hs, _ = hc.build(bspline, HSpace, name)
    rng = np.random.default_rng(sorted(hc.CASES).index(name))
    u = rng.uniform(-1.0, 1.0, hs.numdofs)
    u_hb = hm.hb_coeffs(hs, u)
    funcs = hs.coeffs_to_levelwise_funcs(u)                               # (THB coefficients for a THB space)
    nt = np.cumsum(hs.numactive)
    for lv in range(hs.numlevels):
        R = hs.level_restriction(lv)
        assert R.shape == (hs.mesh(lv).numbf, hs.numdofs) and R.format == 'csr'
        assert not R[:, nt[lv]:].nnz, 'functions of finer levels do not reach an active cell of the level'
        if not hs._cact[lv].any():
            continue
        kvs = hs.knotvectors(lv)
        # two points inside every active cell per axis, as a tensor grid over the whole level; compared on the active cells
        pts = [np.sort(np.concatenate([kv.mesh[:-1] + t * np.diff(kv.mesh) for t in (0.31, 0.77)])) for kv in kvs]
        mask = hs._cact[lv]
        for ax in range(hs.dim):
            mask = np.repeat(mask, 2, axis=ax)
        c = (R @ u_hb).reshape(hs.mesh(lv).numdofs)
        mine = rm._expand([rm.tables_ld(kv, p) for kv, p in zip(kvs, pts)], (0,) * hs.dim, c.astype(LD))
        want = 0
        for fn in funcs:
            want = want + rm._expand([rm.tables_ld(kv, p) for kv, p in zip(fn.kvs, pts)], (0,) * hs.dim, np.asarray(fn.coeffs).reshape([kv.numdofs for kv in fn.kvs]).astype(LD))
        assert float(abs(mine - want)[mask].max()) < 1e-13, (name, lv)


def _toy_space():
    kv = bspline.make_knots(2, 0.0, 1.0, 4)
    hs = HSpace((kv, kv))
    hs.refine({0: [(0, 0), (0, 1), (1, 0), (1, 1)]})
    return hs


def test_mark():
    hs = _toy_space()
    cells = hs.active_cells(flat=True)
    n = len(cells)
    assert n == 12 + 16
    e = np.zeros(n)
    e[[3, 7, 20]] = [4.0, 1.0, 3.0]
    assert hierarchical.mark(hs, e, 0.5) == {cells[3][0]: {cells[3][1]}}
    assert hierarchical.mark(hs, e, 0.51) == {0: {cells[3][1]}, 1: {cells[20][1]}}
    # theta = 1: everything that carries error, nothing else
    got = hierarchical.mark(hs, e, 1.0)
    assert sum(len(v) for v in got.values()) == 3 and cells[7][1] in got[0]
    # ties: canonical position ascending
    e = np.ones(n)
    got = hierarchical.mark(hs, e, 0.25)
    assert got == {0: {c for _, c in cells[:7]}}
    # zeros: the empty prefix reaches theta * 0; 'max' takes every cell (eta2 >= theta^2 * 0)
    assert hierarchical.mark(hs, np.zeros(n), 0.5) == {}
    assert sum(len(v) for v in hierarchical.mark(hs, np.zeros(n), 0.5, 'max').values()) == n
    # max strategy
    e = np.arange(n, dtype=float)
    got = hierarchical.mark(hs, e, 0.9, 'max')
    want = [cells[i] for i in range(n) if e[i] >= 0.81 * (n - 1)]
    assert sum(len(v) for v in got.values()) == len(want) and all(c in got[lv] for lv, c in want)
    # a single cell
    kv = bspline.make_knots(2, 0.0, 1.0, 1)
    one = HSpace((kv, kv))
    assert hierarchical.mark(one, [2.5], 0.5) == {0: {(0, 0)}} == hierarchical.mark(one, [2.5], 1.0, 'max')
    # the result is what refine takes
    e = np.zeros(n)
    e[[3, 20]] = 1.0
    marked = hierarchical.mark(hs, e, 1.0)
    before = hs.total_active_cells
    refined = hs.refine(marked)
    assert refined == marked and hs.total_active_cells == before + 2 * 3
    with pytest.raises(ValueError):
        hierarchical.mark(hs, np.zeros(3))
    with pytest.raises(ValueError):
        hierarchical.mark(hs, np.zeros(hs.total_active_cells), 0.0)
    with pytest.raises(ValueError):
        hierarchical.mark(hs, np.zeros(hs.total_active_cells), 0.5, 'best')


def test_case_table_reaches_the_launch_paths():
    for name, (d, s, dbl, _) in rc.CASES.items():
        want = {'2d_long': 1, '2d_one_wave': 1, '2d_two_waves': 2}.get(name, rc.MAXWAVES)
        assert rc.res12_waves(d, s, dbl) == want, name
    assert rc.res12_waves(*rc.TOO_LONG[:3]) == 0
    d, s, dbl, _ = rc.CASES['3d_manylines_p2']
    assert rc.nlines(rc.shape(d, s, dbl)[1]) == 49284 and rc.lpw(rc.shape(d, s, dbl)[1]) == 3
    assert rc.res12_per_wave(*rc.TOO_LONG[:3]) == 9006 and rc.res12_per_wave(*rc.CASES['2d_two_waves'][:3]) == 2256
    assert rc.res12_per_wave(*rc.CASES['3d_straddle'][:3]) == 6 * 25 + 2 * 69
    assert {'3d_straddle', '3d_straddle5', '3d_mixed_double', '2d_double', '3d_manylines', '3d_onespan0', '3d_onespan1', '3d_onespan2',
            '2d_long'} <= set(rc.CASES)
    assert sorted(max(rc.CASES['3d_p%d' % p][0]) + 1 for p in range(1, 6)) == [2, 3, 4, 5, 6]
    assert {rc.CASES[n][3] for n in rc.CASES} >= {'identity', 'annulus', 'twisted', 'bspline_annulus'}      # both kinds of geometry


def test_launch_logic_is_that_of_the_source():
    src = open(os.path.join(ROOT, 'pyiga_amd', 'csrc', 'kern_quad.hip')).read()
    assert '(size_t)(dim == 3 ? 6 : 3) * Nlast + (size_t)2 * Glast' in src
    assert 'const int nw = quad_waves(per_wave);' in src
    assert re.search(r'constexpr int NL = DIM == 3 \? 6 : 3;', src)
    assert 'span_sums(stage, 2, Gl, ql, Sl, lane, part, nlines * Sl, L);' in src
    assert 'return quad_finish(st, s, 2, d_ws, d_elem, d_tot);' in src
    assert not re.search(r'atomic\w*\s*\(', src)


def _loop_space(p):
    kv = bspline.make_knots(p, 0.0, 1.0, 8)
    return HSpace((kv, kv), truncate=False, bdspecs=[(a, s) for a in range(2) for s in (0, 1)])


@pytest.mark.parametrize('p', [2, 3])
@pytest.mark.parametrize('name', ['square', 'annulus'])
def test_the_doerfler_cut_of_the_loop_case_is_clear(name, p):
    geo = geometry.unit_square() if name == 'square' else geometry.quarter_annulus()
    _, _, f = hm.problem(name)
    out = hm.loop_model(_loop_space(p), geo, f, hm.THETA, hm.ROUNDS, hierarchical.mark)
    dofs = [r['dofs'] for r in out]
    assert all(b > a for a, b in zip(dofs, dofs[1:])), 'a round that adds no function cannot lower the error'
    for r in out[:-1]:
        n, margins = hm.dorfler_margins(r['eta2'], hm.THETA)
        assert n == sum(len(v) for v in r['marked'].values())
        assert min(margins) >= 1e3 * hm.SOLVER_TOL, (name, p, margins)


def test_estimate_refuses_what_it_cannot_serve():
    """the checks come before any device work"""
    S = solvers.HierarchicalSystem.__new__(solvers.HierarchicalSystem)
    S._H, S._bufs, S._matrix = None, [], None
    hs, _ = hc.build(bspline, HSpace, 'hb2p1')
    S.hs, S.problem, S.rhs_form, S.inputs = hs, hc.STIFF, None, {}
    with pytest.raises(ValueError, match='C\\^1'):
        S._check_estimate()
    # a C^0 line: a double interior knot at degree 2.  ('aniso_m2' of the hierarchical case table has double knots at degree 3: that
    # space is C^1, no interior knot reaches multiplicity p, and the estimator serves it.)
    S.hs = hm.c0_line_space(bspline, HSpace)
    with pytest.raises(ValueError, match='jump'):
        S._check_estimate()
    S.hs = hc.build(bspline, HSpace, 'aniso_m2')[0]
    S._check_estimate()
    S.hs = hc.build(bspline, HSpace, 'hb2')[0]
    S._check_estimate()
    S.problem = hc.MASS
    with pytest.raises(ValueError, match='Poisson'):
        S._check_estimate()
    S.problem, S.rhs_form = ' inner( grad(u), grad(v) ) * dx', 'g * v * dx'
    with pytest.raises(ValueError):
        S._check_estimate()
    S.rhs_form = None
    S._check_estimate()
    # a right-hand side that is no callable is refused by name, before any device work
    S._matrix, S.inputs = object(), {'f': 1.0}
    with pytest.raises(TypeError, match='callable'):
        S.estimate(np.zeros(S.hs.numdofs))
    S._matrix = None


def test_adaptive_solve_hands_its_keywords_on(monkeypatch):
    """`tol` is the estimator's, `solve_tol` the linear solver's `tol`; the other keywords reach solve(); no device is touched"""
    seen = []

    class Fake:
        info = {'iterations': 3}

        def __init__(self, hs, problem, rhs, geo=None, lift=None, **inputs):
            seen.append(('init', problem, rhs, lift, sorted(inputs)))
            self.hs = hs

        def solve(self, **kw):
            seen.append(('solve', kw))
            return np.zeros(self.hs.numdofs)

        def estimate(self, u):
            e2 = np.zeros(self.hs.total_active_cells)
            e2[:3] = [3.0, 2.0, 1.0]
            return float(np.sqrt(e2.sum())), e2

        def close(self):
            seen.append(('close',))
    monkeypatch.setattr(solvers, 'HierarchicalSystem', Fake)
    kv = bspline.make_knots(2, 0.0, 1.0, 4)
    hs0 = HSpace((kv, kv))
    hs, u, hist = solvers.adaptive_solve(hs0, None, 'f', max_rounds=2, solve_tol=1e-11, smoother='symmetric_gs', lift=lambda h: np.zeros(h.numdofs))
    assert [s for s in seen if s[0] == 'solve'] == [('solve', {'tol': 1e-11, 'smoother': 'symmetric_gs'})] * 2
    assert seen[0][1] == 'inner(grad(u),grad(v))*dx' and seen[0][2] is None and seen[0][3].shape == (hs0.numdofs,) and seen[0][4] == ['f']
    assert sum(1 for s in seen if s[0] == 'close') == 2 and hs0.numlevels == 1 and hs is not hs0
    assert len(hist) == 2 and hist[0]['marked'] == {0: {(0, 0)}} and hist[1]['marked'] == {} and hist[0]['iterations'] == 3
    assert hist[1]['dofs'] == hs.numdofs and u.shape == (hs.numdofs,)
    # the estimator's tolerance ends the loop; so does max_dofs
    assert len(solvers.adaptive_solve(hs0, None, 'f', tol=10.0)[2]) == 1
    assert len(solvers.adaptive_solve(hs0, None, 'f', max_dofs=hs0.numdofs)[2]) == 1
    assert [s[1] for s in seen if s[0] == 'solve'][-1] == {}

"""assemble.integrate, approx.error_norms and the error_norms methods of the device systems and of Multipatch: against the
reference (tests/golden/golden_quad.npz, made by make_golden_quad.py) at the reference-golden tolerance 1e-12, the two routes of
an exact function (generated kernel / sampled on the host) against each other, and the first convergence-rate test of the
solver stack.  Rounding bounds come from tests/_quad_model.py."""
import os

import numpy as np
import pytest
import scipy.interpolate

from pyiga_amd import approx, assemble, bspline, geometry, solvers
from pyiga_amd.operators import DeviceArray

import _quad_model as qm

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'golden_quad.npz'))
EPS = np.finfo(np.float64).eps
RTOL = 1e-12                      # reference goldens (test_golden_matrices)


# FUNCS: the functions of make_golden_quad.py, restated
def f_phys(*X):
    return np.sin(X[0]) * np.cos(X[1]) + 2.0 + (X[2] * X[2] if len(X) == 3 else 0.0)


def f_par(*X):
    return X[0] * X[0] + X[1] + (np.exp(X[2]) if len(X) == 3 else 0.0)


def f_vec(*X):
    return (X[0] + X[1], X[0] * X[-1] + 1.0)


def g_exact(*X):
    return np.sin(X[0]) * np.cos(X[1]) * (np.cos(X[2]) if len(X) == 3 else 1.0)


def g_grad(*X):
    cz = np.cos(X[2]) if len(X) == 3 else 1.0
    out = (np.cos(X[0]) * np.cos(X[1]) * cz, -np.sin(X[0]) * np.sin(X[1]) * cz)
    return out + ((-np.sin(X[0]) * np.cos(X[1]) * np.sin(X[2]),) if len(X) == 3 else ())


def one(*X):
    return 1.0


def _cylinder():
    return geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.quarter_annulus())


def _setup(tag):
    geo = geometry.quarter_annulus() if tag == '2d' else _cylinder()
    p, n = (int(v) for v in GOLD[tag + '_pn'])
    return geo.sdim * (bspline.make_knots(p, 0.0, 1.0, n),), geo


def _close(a, b):
    return np.all(abs(np.asarray(a) - np.asarray(b)) <= RTOL * abs(np.asarray(b)))


@pytest.mark.parametrize('tag', ['2d', '3d'])
def test_integrate_matches_the_reference(tag):
    kvs, geo = _setup(tag)
    assert _close(assemble.integrate(kvs, f_phys, f_physical=True, geo=geo), GOLD[tag + '_phys'])
    assert _close(assemble.integrate(kvs, f_par, geo=geo), GOLD[tag + '_par_geo'])
    assert _close(assemble.integrate(kvs, f_par), GOLD[tag + '_par'])
    uh = bspline.BSplineFunc(kvs, GOLD[tag + '_dofs'])
    v = assemble.integrate(kvs, uh, geo=geo)
    assert np.ndim(v) == 0 and _close(v, GOLD[tag + '_spline'])
    v = assemble.integrate(kvs, f_vec)
    assert v.shape == (2,) and _close(v, GOLD[tag + '_vec'])
    # with a geometry a vector-valued function is integrated component by component (the reference stops there)
    v = assemble.integrate(kvs, f_vec, f_physical=True, geo=geo)
    comps = [assemble.integrate(kvs, lambda *X, k=k: f_vec(*X)[k], f_physical=True, geo=geo) for k in range(2)]
    assert v.shape == (2,) and _close(v, comps)


def test_integrate_identities_of_the_reference():
    sq, cube = geometry.unit_square(), geometry.unit_cube()
    for geo, key in ((sq, 'one_square'), (cube, 'one_cube')):
        got = [assemble.integrate(geo.kvs, one), assemble.integrate(geo.kvs, one, f_physical=True, geo=geo)]
        assert _close(got, GOLD[key]) and abs(np.asarray(got) - 1.0).max() < 1e-8
    v = assemble.integrate(2 * (bspline.make_knots(3, 0.0, 1.0, 10),), one, geo=geometry.quarter_annulus())
    assert _close(v, GOLD['one_annulus']) and abs(v - 3 * np.pi / 4) < 1e-8


def _rule(kvs, geo):
    """Gauss nodes and weights of a patch of (kvs, geo), and the bound on how far a point the device computes may be from the
    model's (dim components, tests/_quad_model.py point_error): the exact functions are evaluated on the device at its own points."""
    from pyiga_amd import assemblers
    P = assemblers.DevicePatch(kvs, geo)
    try:
        rule = [P.gauss(k) for k in range(len(kvs))]
    finally:
        P.close()
    nodes, weights = [r[0] for r in rule], [r[1] for r in rule]
    return nodes, weights, len(kvs) * qm.point_error(geo, nodes)


@pytest.mark.parametrize('tag', ['2d', '3d'])
def test_error_norms_match_the_reference_on_both_routes(tag, monkeypatch):
    kvs, geo = _setup(tag)
    c = GOLD[tag + '_dofs']
    dim = len(kvs)
    l2, h1 = approx.error_norms(kvs, geo, c, g_exact, g_grad)
    assert _close(l2 ** 2, GOLD[tag + '_l2sq']) and _close(h1 ** 2, GOLD[tag + '_h1sq'])
    only, none = approx.error_norms(kvs, geo, c, g_exact)
    assert none is None and abs(only - l2) <= 4 * EPS * l2
    e2, eh = approx.error_norms(kvs, geo, c, g_exact, g_grad, elementwise=True)
    assert e2.shape == tuple(kv.numspans for kv in kvs) == eh.shape
    assert abs(e2.sum() - l2 ** 2) <= e2.size * EPS * l2 ** 2 and abs(eh.sum() - h1 ** 2) <= eh.size * EPS * h1 ** 2
    # a DeviceArray of the dofs is read where it is, a BSplineFunc gives its coefficients
    from pyiga_amd import _lib
    d_u = DeviceArray.from_host(_lib.context(), c)
    assert approx.error_norms(kvs, geo, d_u, g_exact, g_grad) == (l2, h1)
    assert approx.error_norms(kvs, geo, bspline.BSplineFunc(kvs, c), g_exact, g_grad) == (l2, h1)
    d_u.free()
    # sampled on the host (no generated kernel): both routes lie within the model's bound of the long-double sums
    monkeypatch.setenv('IGX_FORM_RTC', '0')
    s2, sh = approx.error_norms(kvs, geo, c, g_exact, g_grad)
    monkeypatch.delenv('IGX_FORM_RTC')
    nodes, weights, dX = _rule(kvs, geo)
    X = qm.geometry_ld(geo, nodes)[0].astype(np.float64)
    Xs = tuple(X[..., k] for k in range(dim))
    dg = dX + 12 * EPS              # |grad g| and the second derivatives <= 1 per component; sin, cos within 2 ulp, 3 factors
    m = qm.error_model(kvs, geo, c, True, exact=[g_exact(*Xs)] + list(g_grad(*Xs)), nodes=nodes, weights=weights, d_exact=(dg, dg))
    for name, got, k in (('l2 traced', l2, 0), ('l2 sampled', s2, 0), ('h1 traced', h1, 1), ('h1 sampled', sh, 1)):
        err = abs(got ** 2 - float(m['total'][k]))
        print('%s %s: %.15e, |square - model| %.2e (bound %.2e)' % (tag, name, got, err, m['total_bound'][k]))
        assert err <= m['total_bound'][k]
    assert _close(s2 ** 2, GOLD[tag + '_l2sq']) and _close(sh ** 2, GOLD[tag + '_h1sq'])
    # the norms of u_h itself
    n2, nh = approx.error_norms(kvs, geo, c)
    m0 = qm.error_model(kvs, geo, c, True, nodes=nodes, weights=weights)
    assert abs(n2 ** 2 - float(m0['total'][0])) <= m0['total_bound'][0] and abs(nh ** 2 - float(m0['total'][1])) <= m0['total_bound'][1]


def test_multipatch_error_norms_equal_the_one_patch_value():
    """The quarter annulus split at r = 1.5 into two patches, against one patch whose radial knot vector has a C^0 knot there:
    the same spline, the same elements, the same Gauss points."""
    p, n = 2, 3
    kv = bspline.make_knots(p, 0.0, 1.0, n)
    kv_r = bspline.make_knots(p, 0.0, 1.0, 2 * n)
    kv_r = bspline.KnotVector(np.sort(np.append(kv_r.kv, (p - 1) * [0.5])), p)             # multiplicity p at 0.5
    kvs1, geo1 = (kv, kv_r), geometry.quarter_annulus()
    rng = np.random.default_rng(5)
    c1 = rng.uniform(-1.0, 1.0, size=(kv.numdofs, kv_r.numdofs))
    assert kv_r.numdofs == 2 * kv.numdofs - 1
    halves = [geometry.quarter_annulus(1.0, 1.5), geometry.quarter_annulus(1.5, 2.0)]
    MP = assemble.Multipatch([((kv, kv), g) for g in halves], automatch=True)
    u = np.zeros(MP.numdofs)
    for k, part in enumerate((c1[:, :kv.numdofs], c1[:, kv.numdofs - 1:])):
        u[MP.patch_to_global_idx(k)] = part.ravel()
    one_l2, one_h1 = approx.error_norms(kvs1, geo1, c1, g_exact, g_grad)
    mp_l2, mp_h1 = MP.error_norms(u, g_exact, g_grad)
    bound = np.zeros(2)
    for kvs, geo, c in [(kvs1, geo1, c1)] + [((kv, kv), g, MP.global_to_patch(k) @ u) for k, g in enumerate(halves)]:
        nodes, weights, dX = _rule(kvs, geo)
        X = qm.geometry_ld(geo, nodes)[0].astype(np.float64)
        Xs = tuple(X[..., k] for k in range(2))
        m = qm.error_model(kvs, geo, np.reshape(c, [k.numdofs for k in kvs]), True, exact=[g_exact(*Xs)] + list(g_grad(*Xs)),
                           nodes=nodes, weights=weights, d_exact=(dX + 12 * EPS,) * 2)
        bound += m['total_bound']
    print('one patch %.15e %.15e, two patches %.15e %.15e, bound on the squares %.2e %.2e' % (one_l2, one_h1, mp_l2, mp_h1, bound[0], bound[1]))
    assert abs(mp_l2 ** 2 - one_l2 ** 2) <= bound[0] and abs(mp_h1 ** 2 - one_h1 ** 2) <= bound[1]
    assert MP.error_norms(u, g_exact)[1] is None
    MP.close()


# ---------------------------------------------------------------------------------------------
# convergence: -Laplace u = 2 pi^2 sin(pi x) sin(pi y) on the unit square, u = 0 on the boundary, p = 2
def u_exact(x, y):
    return np.sin(np.pi * x) * np.sin(np.pi * y)


def u_grad(x, y):
    return (np.pi * np.cos(np.pi * x) * np.sin(np.pi * y), np.pi * np.sin(np.pi * x) * np.cos(np.pi * y))


def _host_galerkin(kv):
    """Dofs of the Galerkin solution, mass and stiffness matrix, by dense numpy with scipy.interpolate.BSpline tables and the
    p + 1 point rule.  The right-hand side is separable: b = 2 pi^2 b1 (x) b1."""
    p, N = kv.p, kv.numdofs
    x, w = qm.gauss_rule(kv, p + 1)
    B = np.stack([scipy.interpolate.BSpline(kv.kv, np.eye(N)[i], p)(x) for i in range(N)])
    D = np.stack([scipy.interpolate.BSpline(kv.kv, np.eye(N)[i], p).derivative()(x) for i in range(N)])
    M1, K1, b1 = (B * w) @ B.T, (D * w) @ D.T, (B * w) @ np.sin(np.pi * x)
    M, A = np.kron(M1, M1), np.kron(K1, M1) + np.kron(M1, K1)
    free = np.zeros((N, N), dtype=bool)
    free[1:-1, 1:-1] = True
    free = free.ravel()
    u = np.zeros(N * N)
    u[free] = np.linalg.solve(A[np.ix_(free, free)], 2 * np.pi ** 2 * np.kron(b1, b1)[free])
    return u, M, A


def test_poisson_converges_at_the_optimal_rates():
    geo = geometry.unit_square()
    dev, host = {}, {}
    for n in (8, 16):
        kv = bspline.make_knots(2, 0.0, 1.0, n)
        kvs = (kv, kv)
        bcs = assemble.compute_dirichlet_bcs(kvs, geo, ('all', 0.0))
        S = solvers.PatchSystem(kvs, geo, lambda x, y: 2 * np.pi ** 2 * u_exact(x, y), bcs)
        try:
            u_dev = S.solve(tol=1e-12)
            assert S.info['converged']
            dev[n] = S.error_norms(u_dev, u_exact, u_grad)
        finally:
            S.close()
        u_host, M, A = _host_galerkin(kv)
        # the errors of the host solution and of the device solution in long double, with the model's bound on the device's sums:
        # the exact values are evaluated on the device at points it computes (|grad g| <= pi, second derivatives <= pi^2, the
        # argument pi x rounded once)
        nodes, weights, dX = _rule(kvs, geo)
        Xs = tuple(np.broadcast_to(a, (len(nodes[0]), len(nodes[1]))) for a in (nodes[1][None, :], nodes[0][:, None]))
        ex = [u_exact(*Xs)] + list(u_grad(*Xs))
        dg = (np.pi * (dX + 2 * EPS) + 8 * EPS, np.pi ** 2 * (dX + 2 * EPS) + 8 * np.pi * EPS)
        shape = (kv.numdofs, kv.numdofs)
        mh = qm.error_model(kvs, geo, u_host.reshape(shape), True, exact=ex, nodes=nodes, weights=weights)
        md = qm.error_model(kvs, geo, u_dev.reshape(shape), True, exact=ex, nodes=nodes, weights=weights, d_exact=dg)
        host[n] = tuple(float(np.sqrt(mh['total'][k])) for k in range(2))
        d = u_dev - u_host
        for k, mat, name in ((0, M, 'L2'), (1, A, 'H1')):
            e_model = float(np.sqrt(md['total'][k]))
            slack = np.sqrt(max(d @ mat @ d, 0.0)) + md['total_bound'][k] / e_model      # |sqrt a - sqrt b| <= |a - b| / sqrt b
            print('n = %2d %s: device %.9e host %.9e, |difference| %.2e <= %.2e' % (n, name, dev[n][k], host[n][k], abs(dev[n][k] - host[n][k]), slack))
            assert abs(dev[n][k] - host[n][k]) <= slack
    r_l2 = np.log2(dev[8][0] / dev[16][0])
    r_h1 = np.log2(dev[8][1] / dev[16][1])
    print('rates: L2 %.3f, H1 %.3f' % (r_l2, r_h1))
    assert 2.9 < r_l2 < 3.2
    assert 1.9 < r_h1 < 2.1

"""Host model of the hierarchical error norms, the residual estimator and the adaptive loop.

The per-level sums are ``_resid_model.residual_model`` / ``_quad_model.error_model`` applied level by level with the active-cell
masks.  Of the library only the host-side bookkeeping of ``HSpace`` is used (knot vectors, active-cell arrays,
``level_restriction`` -- which tests/test_resid_cpu.py checks on its own against the level-wise functions); nothing runs on a device.

The Poisson model of the loop (2D): per level the tensor-product stiffness matrix and load vector over the ACTIVE cells of the
level from this package's long-double tables (rounded to float64), ``A = sum_lv R_lv^t K_lv R_lv`` with
``R_lv = level_restriction(lv)``, the load vector level by level on the whole patch as the device forms it, a sparse direct solve on
the non-Dirichlet dofs."""
import numpy as np
import scipy.sparse
import scipy.sparse.linalg

import _resid_model as rm

EPS = rm.EPS
LD = rm.LD


def level_coeffs(hs, u_hb, lv):
    """(level dofs in long double, bound on a float64 row sum formed in any order) of the canonical HB coefficients `u_hb`"""
    R = scipy.sparse.csr_matrix(hs.level_restriction(lv))
    u = np.asarray(u_hb, dtype=np.float64)
    c = np.zeros(R.shape[0], dtype=LD)
    mag = np.zeros(R.shape[0])
    for i in range(R.shape[0]):
        lo, hi = R.indptr[i], R.indptr[i + 1]
        c[i] = (R.data[lo:hi].astype(LD) * u[R.indices[lo:hi]].astype(LD)).sum()
        mag[i] = abs(R.data[lo:hi] * u[R.indices[lo:hi]]).sum()
    rowmax = int(np.diff(R.indptr).max()) if R.shape[0] else 0
    return c.reshape(hs.mesh(lv).numdofs), (rowmax + 2) * EPS * float(mag.max())


def hb_coeffs(hs, u):
    return hs.thb_to_hb() @ np.asarray(u, dtype=np.float64) if hs.truncate else np.asarray(u, dtype=np.float64)


def estimate_model(hs, geo, u, f=None, f_lip=0.0, rules=None):
    """(element sums [2][ncells] in long double, their bounds [2][ncells]) over the active cells in canonical order.  `rules`:
    ``{lv: (nodes per axis, weights per axis)}``, the rule a device patch of the level uses (default: ``_resid_model.gauss_rule``)."""
    u_hb = hb_coeffs(hs, u)
    # (THB: the device forms T u in float64 as well; its rounding is of the size of the row-sum bound and is added to it)
    extra = 0.0
    if hs.truncate:
        T = scipy.sparse.csr_matrix(hs.thb_to_hb())
        extra = (int(np.diff(T.indptr).max()) + 2) * EPS * float(abs(T).dot(abs(np.asarray(u, dtype=np.float64))).max())
    elems, bounds = [], []
    for lv in range(hs.numlevels):
        mask = hs._cact[lv]
        if not mask.any():
            continue
        c, c_err = level_coeffs(hs, u_hb, lv)
        R = scipy.sparse.csr_matrix(hs.level_restriction(lv))
        c_err += float(abs(R).sum(axis=1).max()) * extra
        nodes, weights = rules[lv] if rules else (None, None)
        m = rm.residual_model(hs.knotvectors(lv), geo, c, f=f, nodes=nodes, weights=weights, c_err=c_err, f_lip=f_lip)
        elems.append(m['elem'][:, mask])
        bounds.append(m['elem_bound'][:, mask])
    return np.concatenate(elems, axis=1), np.concatenate(bounds, axis=1)


def eta2_model(hs, geo, u, f=None):
    e, _ = estimate_model(hs, geo, u, f)
    return rm.eta2(e, hs.dim).astype(np.float64)


# ---------------------------------------------------------------------------------------------
def _kron_tables(Ms, orders):
    out = None
    for M, d in zip(Ms, orders):
        A = scipy.sparse.csr_matrix(M[d].astype(np.float64))
        out = A if out is None else scipy.sparse.kron(out, A, format='csr')
    return out


def level_poisson(kvs, geo, mask, f):
    """(K, b) of one level over the cells of `mask` (2D), float64 sparse"""
    dim = len(kvs)
    assert dim == 2
    q = max(int(kv.p) for kv in kvs) + 1
    rules = [rm.gauss_rule(kv, q) for kv in kvs]
    nodes, weights = [r[0] for r in rules], [r[1] for r in rules]
    Ms = [rm.tables_ld(kv, nd) for kv, nd in zip(kvs, nodes)]
    X, J, _, _, _, _ = rm.geometry2_ld(geo, nodes)
    det, JI = rm._det_inv(J)
    pm = mask
    for ax in range(dim):
        pm = np.repeat(pm, q, axis=ax)
    W = (weights[0][:, None] * weights[1][None, :] * abs(det).astype(np.float64) * pm).ravel()
    JI = JI.astype(np.float64).reshape(-1, dim, dim)
    D = [_kron_tables(Ms, rm._orders(dim, (c,))) for c in range(dim)]        # parametric partial c (x, y order)
    B = _kron_tables(Ms, (0,) * dim)
    K = 0
    for r in range(dim):                                                      # D_r = sum_c JI[c][r] Dhat_c
        G = sum(scipy.sparse.diags(JI[:, c, r]) @ D[c] for c in range(dim))
        K = K + G.T @ scipy.sparse.diags(W) @ G
    Xd = X.astype(np.float64)
    fv = np.broadcast_to(np.asarray(f(Xd[..., 0], Xd[..., 1]), dtype=np.float64), Xd.shape[:-1]).ravel()
    return scipy.sparse.csr_matrix(K), B.T @ (W * fv)


def solve_model(hs, geo, f):
    """The Galerkin solution with homogeneous Dirichlet data on the sides of ``hs.bdspecs``: canonical coefficients of the basis
    of `hs` (HB or THB)."""
    n = hs.numdofs
    A, b = scipy.sparse.csr_matrix((n, n)), np.zeros(n)
    for lv in range(hs.numlevels):
        if not hs._cact[lv].any():
            continue
        K, rhs = level_poisson(hs.knotvectors(lv), geo, hs._cact[lv], f)
        R = scipy.sparse.csr_matrix(hs.level_restriction(lv))
        A = A + R.T @ K @ R
    # the load vector as the device assembles it: every level on its WHOLE patch with its own rule, the
    # entries of the level's active functions gathered -- for an f that is no polynomial not the same numbers as the cell-wise sum
    off = 0
    for lv, act in enumerate(hs.active_indices()):
        if act.size:
            whole = np.ones(hs.mesh(lv).numspans, dtype=bool)
            b[off:off + act.size] = level_poisson(hs.knotvectors(lv), geo, whole, f)[1][act]
            off += act.size
    if hs.truncate:
        T = scipy.sparse.csr_matrix(hs.thb_to_hb())
        A, b = T.T @ A @ T, T.T @ b
    free = np.asarray(hs.non_dirichlet_dofs(), dtype=np.int64)
    u = np.zeros(n)
    u[free] = scipy.sparse.linalg.spsolve(scipy.sparse.csc_matrix(A[free][:, free]), b[free])
    return u


def dorfler_margins(eta2, theta):
    """(n, margins): the length of the Doerfler prefix and how far the cut keeps clear of its neighbours, relative to the total:
    the prefix sum above theta * total, theta * total above the prefix one shorter, and the gap between the last cell taken and
    the first one left."""
    e = np.sort(np.asarray(eta2, dtype=np.float64))[::-1]
    cs = np.cumsum(e)
    tot = cs[-1]
    n = int(np.searchsorted(cs, theta * tot, side='left')) + 1
    below = cs[n - 2] if n >= 2 else 0.0
    gap = e[n - 1] - e[n] if n < e.size else np.inf
    return n, ((cs[n - 1] - theta * tot) / tot, (theta * tot - below) / tot, gap / tot)


def loop_model(hs, geo, f, theta, rounds, mark):
    """The adaptive loop on the host: per round (dofs, eta2, marked, u); `mark` is ``hierarchical.mark``.  Works on a copy."""
    hs = hs.copy()
    out = []
    for rnd in range(rounds):
        u = solve_model(hs, geo, f)
        e2 = eta2_model(hs, geo, u, f)
        marked = mark(hs, e2, theta, 'dorfler') if rnd < rounds - 1 else {}
        out.append(dict(dofs=hs.numdofs, eta2=e2, marked=marked, u=u, hs=hs.copy()))
        if marked:
            hs.refine(marked, truncate=hs.truncate)
    return out


# the loop case of tests/test_resid_cpu.py (the cut is clear) and tests/test_hadapt_gpu.py
PEAK = (0.37, 0.61)                               # off-centre; different widths along x and y: no symmetric ties
WIDTH = (0.3, 0.45)
SOLVER_TOL = 1e-10
THETA, ROUNDS = 0.5, 3


def problem(name):
    """The manufactured Poisson problem of the loop on 'square' (unit square) or 'annulus' (quarter annulus, radii 1 and 2):
    u = phi E with phi a polynomial that vanishes on the boundary and E = exp(-((x - a) / s)^2 - ((y - b) / t)^2) an off-centre peak
    with different widths along x and y.  Returns (u, grad_u, f) with f = -Lap u = -(E Lap phi + 2 grad phi . grad E + phi Lap E),
    all callables of (x, y) made of arithmetic and ``numpy.exp``."""
    if name == 'square':
        a, b = PEAK
        phi = lambda x, y: x * (1.0 - x) * y * (1.0 - y)
        dphi = lambda x, y: ((1.0 - 2.0 * x) * y * (1.0 - y), x * (1.0 - x) * (1.0 - 2.0 * y))
        lphi = lambda x, y: -2.0 * y * (1.0 - y) - 2.0 * x * (1.0 - x)
    else:
        a, b = 1.1, 0.9
        m = lambda s: (s - 1.0) * (4.0 - s)
        dm = lambda s: 5.0 - 2.0 * s
        phi = lambda x, y: x * y * m(x * x + y * y)
        dphi = lambda x, y: (y * m(x * x + y * y) + 2.0 * x * x * y * dm(x * x + y * y), x * m(x * x + y * y) + 2.0 * x * y * y * dm(x * x + y * y))
        lphi = lambda x, y: x * y * (12.0 * dm(x * x + y * y) - 8.0 * (x * x + y * y))
    s, t = WIDTH
    E = lambda x, y: np.exp(-((x - a) * (x - a)) / (s * s) - ((y - b) * (y - b)) / (t * t))
    gx = lambda x: -2.0 * (x - a) / (s * s)
    gy = lambda y: -2.0 * (y - b) / (t * t)
    u = lambda x, y: phi(x, y) * E(x, y)
    grad = lambda x, y: ((dphi(x, y)[0] + phi(x, y) * gx(x)) * E(x, y), (dphi(x, y)[1] + phi(x, y) * gy(y)) * E(x, y))
    f = lambda x, y: -(lphi(x, y) + 2.0 * (dphi(x, y)[0] * gx(x) + dphi(x, y)[1] * gy(y))
                       + phi(x, y) * (gx(x) * gx(x) + gy(y) * gy(y) - 2.0 / (s * s) - 2.0 / (t * t))) * E(x, y)
    return u, grad, f


def c0_line_space(bspline, HSpace):
    """'aniso_m2' of tests/_hier_cases.py with the degree of its first axis lowered to the multiplicity of its interior knots: a
    C^0 line at every one of them"""
    kvs = (bspline.make_knots(2, 0.0, 1.0, 4, mult=2), bspline.make_knots(2, 0.0, 1.0, 5))
    hs = HSpace(kvs, bdspecs=[(a, s) for a in range(2) for s in (0, 1)])
    hs.refine_region(0, lambda *X: abs(X[0] - X[-1]) < 0.5)
    return hs

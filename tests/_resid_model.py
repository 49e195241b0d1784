"""Host model of the residual kernel (pyiga_amd/csrc/kern_quad.hip: k_res12): per-element sums and totals of
    W (f + Lap u_h)^2   and   W,      W = gw |det J|,
in long double.  Nothing of the library is used: the order-0/1/2 collocation tables are this module's own Cox-de Boor recursion
(``tables_ld``), the rule is ``numpy.polynomial.legendre.leggauss``, a spline or NURBS geometry is evaluated from its control net
with the same tables (second-order quotient rule for NURBS), the 2x2 / 3x3 inverse is written out.

The formula (all parametric indices in the order x, y, z: index 0 belongs to the LAST grid axis):
    J[r][c] = d G_r / d xi_c,  JI = J^-1,  K = JI JI^t,  H2[m][e][u] = d^2 G_m / d xi_e d xi_u,
    b_c = -sum_m JI[c][m] s_m,  s_m = sum_eu H2[m][e][u] K[e][u],
    Lap u_h = sum_cd K[c][d] D_c D_d u^ + sum_c b_c D_c u^.

The rounding bound the GPU test uses (``EPS`` = 2^-52), derived from operation counts and magnitudes, no fitted constant.  The
``S`` below are taken from ABSOLUTE tables: the derivative recursion  B' = p (B_low[i] / h_i - B_low[i+1] / h_i+1)  with a plus
sign, so that the cancellation inside a table entry (a double table entry is wrong by a few EPS of that uncancelled magnitude)
is covered.

* A parametric derivative of u_h of orders o = (o_0, .., o_dim-1) is a sum of at most P^dim <= 216 products of table entries and
  a dof:  d_par(o) = 250 EPS max|c| prod_k S_k[o_k],  S_k[d] = max_g sum_l A_k[d][g][l]  (250 = 216 products and additions plus the
  error of the three table entries of a product, as tests/_quad_model.py counts them).
* An entry of the homogeneous geometry derivatives likewise:  e_j = 250 EPS max|net| max_{|o| = j} prod_k S^geo_k[o_k],  j = 0, 1, 2.
* Quotient rule, first order in the e_j, every formula rounded with at most 8 operations on its uncancelled magnitude:
      x  = A / w                                 dx  = (e_0 (1 + |x|)) / wmin + 2 EPS |x|
      x_a = (A_a - w_a x) / w                    dJ  = (e_1 (1 + |x|) + |w_a| dx + |x_a| e_0) / wmin + 8 EPS (|A_a| + |w_a x|) / wmin
      x_ab = (A_ab - w_a x_b - w_b x_a - w_ab x) / w
                                                 dH2 = (e_2 (1 + |x|) + 2 (e_1 |x_a| + |w_a| dJ) + |w_ab| dx + |x_ab| e_0) / wmin
                                                       + 8 EPS (|A_ab| + 2 |w_a x_b| + |w_ab x|) / wmin
  with the maxima over the grid of every magnitude.  A B-spline map has w = 1 and no weight derivatives: dJ = e_1, dH2 = e_2.
* JI = cofactors / det.  A cofactor is a sum of (dim-1)! products of dim - 1 entries, det one of dim! products of dim entries:
      dcof = (dim-1)! ((dim-1) Jmax^(dim-2) dJ + 2 dim EPS Jmax^(dim-1)),   ddet = dim! (dim Jmax^(dim-1) dJ + 2 dim EPS Jmax^dim),
      dJI = dcof / detmin + JImax (ddet / detmin + 3 EPS).
  The weight W = gw |det J| comes from the patch's field kernel: relative error g_W = ddet / detmin + 4 EPS (tests/_quad_model.py).
* K = JI JI^t, dim products per entry:   dK = 2 dim JImax dJI + 2 dim EPS JImax^2.
* s_m, dim^2 products:                   ds = dim^2 (H2max dK + Kmax dH2) + 2 dim^2 EPS H2max Kmax.
* b_c, dim products:                     db = dim (JImax ds + smax dJI) + 2 dim EPS JImax smax.
* Lap u_h at a point, n_op = dim (dim + 1) / 2 + dim + 3 operations:
      dlap = sum_cd (|K_cd| d_par(cd) + dK |H_cd|) + sum_c (|b_c| d_par(c) + db |D_c u^|) + n_op EPS M,
      M = |f| + sum_cd |K_cd H_cd| + sum_c |b_c D_c u^|          (the magnitude that rounds: the bound scales with sum W M^2)
* A term t = W r^2, r = f + Lap u_h (f is the same double on both sides):  dt = W (2 |r| dlap + dlap^2) + (g_W + 3 EPS) t;  the
  term W itself: g_W W.
* A sum of n terms adds  EPS n sum|t|:  n = q^dim for an element; the total adds the  ceil(nelem / 256) + 8  additions of the
  strided sum and the tree of k_quad_total.
"""
import itertools
import math

import numpy as np

LD = np.longdouble
EPS = np.finfo(np.float64).eps


def gauss_rule(kv, nqp):
    """Nodes and weights (float64) of the nqp-point Gauss rule on every span of `kv`, span after span."""
    x, w = np.polynomial.legendre.leggauss(nqp)
    mesh = np.unique(np.asarray(kv.kv, dtype=np.float64))
    a, b = mesh[:-1, None], mesh[1:, None]
    return (0.5 * (a + b) + 0.5 * (b - a) * x[None, :]).ravel(), (0.5 * (b - a) * w[None, :]).ravel()


def _dense_basis(kn, d, x):
    """All B-splines of degree d over the knots kn at the points x (right-continuous; left-continuous at the right end): (G, len(kn) - d - 1)."""
    m = kn.size - 1
    span = np.minimum(np.searchsorted(kn, x, side='right') - 1, np.searchsorted(kn, kn[-1], side='left') - 1)   # (the right end: last span)
    B = np.zeros((x.size, m), dtype=LD)
    B[np.arange(x.size), span] = 1
    for k in range(1, d + 1):
        nb = kn.size - k - 1
        out = np.zeros((x.size, nb), dtype=LD)
        for i in range(nb):
            h0, h1 = kn[i + k] - kn[i], kn[i + k + 1] - kn[i + 1]
            if h0 > 0:
                out[:, i] += (x - kn[i]) / h0 * B[:, i]
            if h1 > 0:
                out[:, i] += (kn[i + k + 1] - x) / h1 * B[:, i + 1]
        B = out
    return B


def _derive(kn, d, low, absolute):
    """degree-d functions' derivative from the table `low` of degree d - 1 (values or derivatives): (G, n_low - 1)"""
    nb = kn.size - d - 1
    out = np.zeros((low.shape[0], nb), dtype=LD)
    for i in range(nb):
        h0, h1 = kn[i + d] - kn[i], kn[i + d + 1] - kn[i + 1]
        if h0 > 0:
            out[:, i] += d * low[:, i] / h0
        if h1 > 0:
            out[:, i] += (d if absolute else -d) * low[:, i + 1] / h1
    return out


def tables_ld(kv, nodes, absolute=False):
    """(3, G, N) long double: orders 0, 1, 2 of all basis functions of `kv` at `nodes` (dense); `absolute`: the uncancelled
    magnitudes of the derivative recursion (module docstring)."""
    kn = np.asarray(kv.kv, dtype=np.float64).astype(LD)
    p = int(kv.p)
    x = np.asarray(nodes, dtype=np.float64).astype(LD)
    N = kn.size - p - 1
    C = np.zeros((3, x.size, N), dtype=LD)
    C[0] = _dense_basis(kn, p, x)
    if p >= 1:
        C[1] = _derive(kn, p, _dense_basis(kn, p - 1, x), absolute)
    if p >= 2:
        C[2] = _derive(kn, p, _derive(kn, p - 1, _dense_basis(kn, p - 2, x), absolute), absolute)
    return C


def _expand(Ms, orders, c):
    out = c
    for k, (M, d) in enumerate(zip(Ms, orders)):
        out = np.moveaxis(np.tensordot(M[d], out, axes=(1, k)), 0, k)
    return out


def _S(As):
    """S[k][d] = max_g sum_l A_k[d][g][l]"""
    return [[float(abs(A[d]).sum(axis=1).max()) for d in range(3)] for A in As]


def _orders(dim, cs):
    """order tuple (per GRID axis) of the derivative along the parametric directions `cs` (x, y, z order: c <-> axis dim-1-c)"""
    o = [0] * dim
    for c in cs:
        o[dim - 1 - c] += 1
    return tuple(o)


def _det_inv(J):
    dim = J.shape[-1]
    if dim == 2:
        det = J[..., 0, 0] * J[..., 1, 1] - J[..., 0, 1] * J[..., 1, 0]
        adj = np.stack([np.stack([J[..., 1, 1], -J[..., 0, 1]], -1), np.stack([-J[..., 1, 0], J[..., 0, 0]], -1)], -2)
        return det, adj / det[..., None, None]
    c = lambda i, j: J[..., (i + 1) % 3, (j + 1) % 3] * J[..., (i + 2) % 3, (j + 2) % 3] - J[..., (i + 1) % 3, (j + 2) % 3] * J[..., (i + 2) % 3, (j + 1) % 3]
    cof = np.stack([np.stack([c(i, j) for j in range(3)], -1) for i in range(3)], -2)
    det = (J[..., 0, :] * cof[..., 0, :]).sum(-1)
    return det, np.swapaxes(cof, -1, -2) / det[..., None, None]


def geometry2_ld(geo, nodes):
    """X: points G + (dim,); J: G + (dim, dim), J[r][c] = d G_r / d xi_c; H2: G + (dim, dim, dim), H2[m][e][u]; and the bounds
    (dJ, dH2, dX) on the error of a float64 evaluation (module docstring).  Parametric indices in x, y, z order."""
    dim = len(nodes)
    Ms = [tables_ld(kv, nd) for kv, nd in zip(geo.kvs, nodes)]
    S = _S([tables_ld(kv, nd, absolute=True) for kv, nd in zip(geo.kvs, nodes)])
    net = np.asarray(geo.coeffs).astype(LD)                      # (float64 as the device reads it; a long-double net is kept)
    nurbs = net.shape[-1] == dim + 1
    A0 = _expand(Ms, (0,) * dim, net)
    A1 = [_expand(Ms, _orders(dim, (c,)), net) for c in range(dim)]
    A2 = [[_expand(Ms, _orders(dim, (e, u)), net) for u in range(dim)] for e in range(dim)]
    nmax = float(abs(net).max())
    e = [250 * EPS * nmax * max(float(np.prod([S[k][o[k]] for k in range(dim)]))
                                for o in itertools.product(range(3), repeat=dim) if sum(o) == j) for j in range(3)]
    mx = lambda a: float(abs(a).max())
    if nurbs:
        w, w1, w2 = A0[..., -1:], [a[..., -1:] for a in A1], [[a[..., -1:] for a in row] for row in A2]
        X = A0[..., :-1] / w
        X1 = [(A1[c][..., :-1] - w1[c] * X) / w for c in range(dim)]
        X2 = [[(A2[a][b][..., :-1] - w1[a] * X1[b] - w1[b] * X1[a] - w2[a][b] * X) / w for b in range(dim)] for a in range(dim)]
        wmin, xm = float(abs(w).min()), mx(X)
        w1m, w2m = max(mx(a) for a in w1), max(mx(a) for row in w2 for a in row)
        x1m, x2m = max(mx(a) for a in X1), max(mx(a) for row in X2 for a in row)
        a1m, a2m = max(mx(a[..., :-1]) for a in A1), max(mx(a[..., :-1]) for row in A2 for a in row)
        dx = e[0] * (1 + xm) / wmin + 2 * EPS * xm
        dJ = (e[1] * (1 + xm) + w1m * dx + x1m * e[0]) / wmin + 8 * EPS * (a1m + w1m * xm) / wmin
        dH2 = ((e[2] * (1 + xm) + 2 * (e[1] * x1m + w1m * dJ) + w2m * dx + x2m * e[0]) / wmin
               + 8 * EPS * (a2m + 2 * w1m * x1m + w2m * xm) / wmin)
    else:
        X, X1, X2 = A0, A1, A2
        dJ, dH2 = e[1], e[2]
    J = np.stack(X1, axis=-1)
    H2 = np.stack([np.stack(row, axis=-1) for row in X2], axis=-2)       # [..., m, e, u]
    return X, J, H2, dJ, dH2, (dx if nurbs else e[0])


def laplace_ld(kvs, geo, c, nodes, c_err=0.0):
    """Lap u_h at the Gauss grid in long double and everything the bound needs (a dict).  `c_err`: how far the dofs the device
    uses may be from `c` (it forms them itself); it enters d_par beside the 250 EPS max|c|."""
    dim = len(kvs)
    Ms = [tables_ld(kv, nd) for kv, nd in zip(kvs, nodes)]
    S = _S([tables_ld(kv, nd, absolute=True) for kv, nd in zip(kvs, nodes)])
    cl = np.asarray(c).astype(LD)
    cmax = float(abs(cl).max())
    d_par = lambda cs: (250 * EPS * cmax + c_err) * float(np.prod([S[k][o] for k, o in enumerate(_orders(dim, cs))]))
    X, J, H2, dJ, dH2, dX = geometry2_ld(geo, nodes)
    det, JI = _det_inv(J)
    K = (JI[..., :, None, :] * JI[..., None, :, :]).sum(-1)
    s = (H2 * K[..., None, :, :]).sum((-1, -2))                          # s_m
    b = -(JI * s[..., None, :]).sum(-1)                                  # b_c = -sum_m JI[c][m] s_m
    mx = lambda a: float(abs(a).max())
    Jmax, JImax, detmin, Kmax, H2max, smax = mx(J), mx(JI), float(abs(det).min()), mx(K), mx(H2), mx(s)
    f1, f = math.factorial(dim - 1), math.factorial(dim)
    dcof = f1 * ((dim - 1) * Jmax ** (dim - 2) * dJ + 2 * dim * EPS * Jmax ** (dim - 1))
    ddet = f * (dim * Jmax ** (dim - 1) * dJ + 2 * dim * EPS * Jmax ** dim)
    dJI = dcof / detmin + JImax * (ddet / detmin + 3 * EPS)
    dK = 2 * dim * JImax * dJI + 2 * dim * EPS * JImax ** 2
    ds = dim * dim * (H2max * dK + Kmax * dH2) + 2 * dim * dim * EPS * H2max * Kmax
    db = dim * (JImax * ds + smax * dJI) + 2 * dim * EPS * JImax * smax
    lap, M, dlap = 0, 0, 0
    for cc in range(dim):
        g = _expand(Ms, _orders(dim, (cc,)), cl)
        lap = lap + b[..., cc] * g
        M = M + abs(b[..., cc] * g)
        dlap = dlap + abs(b[..., cc]) * d_par((cc,)) + db * abs(g)
        for dd in range(dim):
            h = _expand(Ms, _orders(dim, (cc, dd)), cl)
            lap = lap + K[..., cc, dd] * h
            M = M + abs(K[..., cc, dd] * h)
            dlap = dlap + abs(K[..., cc, dd]) * d_par((cc, dd)) + dK * abs(h)
    g_W = ddet / detmin + 4 * EPS
    return {'lap': lap, 'M': M, 'dlap': dlap, 'det': det, 'g_W': g_W, 'X': X, 'dX': dX}


def _element_sums(t, q):
    nk, G = t.shape[0], t.shape[1:]
    shp = (nk,) + tuple(x for g in G for x in (g // q, q))
    return t.reshape(shp).sum(axis=tuple(2 + 2 * k for k in range(len(G))))


def _finish(t, dt, q):
    """terms t and their error bounds dt (both [nk][G..]) -> element sums, totals and the two bounds.  In long double the order
    of the additions is immaterial against the bound; the kernel's order (span sums of a line ascending, the lines of an element
    ascending) enters the bound through the count n of the additions."""
    dim = t.ndim - 1
    elem = _element_sums(t, q)
    n_el = q ** dim
    eb = _element_sums(dt, q) + EPS * n_el * _element_sums(abs(t), q)
    nelem = int(np.prod(elem.shape[1:]))
    axes = tuple(range(1, 1 + dim))
    n_tot = n_el + -(-nelem // 256) + 8
    tb = dt.sum(axis=axes) + EPS * n_tot * abs(t).sum(axis=axes)
    return {'elem': elem, 'total': elem.sum(axis=axes), 'elem_bound': eb.astype(np.float64), 'total_bound': tb.astype(np.float64)}


def residual_model(kvs, geo, c, f=None, nodes=None, weights=None, c_err=0.0, f_lip=0.0):
    """The two sums of the spline with the dofs `c` (shape ndofs) over the spline / NURBS map `geo` (an object with ``kvs`` and the
    homogeneous control net ``coeffs``).  `f`: None (= 0) or float64 values on the Gauss grid.  `nodes` / `weights`: the rule per
    axis (default: this module's ``gauss_rule`` with max p + 1 points).  Returns the dict of ``_finish`` (2 quantities) plus the
    pointwise ``lap`` and the points ``X``.  `c_err`: see ``laplace_ld``.  `f` may be a callable in physical coordinates that the
    device evaluates at ITS points: it is sampled at ``X`` here and `f_lip` (a bound on sum_k |d f / d x_k|) times the bound dX on a
    float64 point is added to dlap."""
    dim = len(kvs)
    q = max(int(kv.p) for kv in kvs) + 1
    if nodes is None:
        rules = [gauss_rule(kv, q) for kv in kvs]
        nodes, weights = [r[0] for r in rules], [r[1] for r in rules]
    L = laplace_ld(kvs, geo, c, nodes, c_err)
    gw = np.asarray(weights[0], dtype=np.float64).astype(LD)
    for w in weights[1:]:
        gw = gw[..., None] * np.asarray(w, dtype=np.float64).astype(LD)
    W = gw * abs(L['det'])
    if callable(f):
        Xd = L['X'].astype(np.float64)
        f = np.broadcast_to(np.asarray(f(*(Xd[..., k] for k in range(dim))), dtype=np.float64), Xd.shape[:-1])
    fv = 0 if f is None else np.asarray(f, dtype=np.float64).astype(LD)
    r = fv + L['lap']
    n_op = dim * (dim + 1) // 2 + dim + 3
    dlap = L['dlap'] + n_op * EPS * (abs(fv) + L['M']) + f_lip * L['dX']
    t0 = W * r * r
    dt0 = W * (2 * abs(r) * dlap + dlap * dlap) + (L['g_W'] + 3 * EPS) * t0
    out = _finish(np.stack([t0, W]), np.stack([dt0, L['g_W'] * W]), q)
    out['lap'], out['X'], out['W'] = L['lap'], L['X'], W
    return out


def eta2(elem, dim):
    """eta_K^2 = (sum_K W)^(2/dim) sum_K W (f + Lap u_h)^2 from the two element sums"""
    return np.power(elem[1], LD(2) / dim) * elem[0]


# ---------------------------------------------------------------------------------------------
# long-double interpolation (the exactness tests build polynomial data with it)
def solve_ld(A, B):
    """A^-1 B by Gaussian elimination with partial pivoting in long double (numpy.linalg has none)."""
    A = np.array(A, dtype=LD)
    B = np.array(B, dtype=LD).reshape(A.shape[0], -1)
    n = A.shape[0]
    for k in range(n):
        piv = k + int(np.argmax(abs(A[k:, k])))
        if piv != k:
            A[[k, piv]], B[[k, piv]] = A[[piv, k]], B[[piv, k]]
        for i in range(k + 1, n):
            m = A[i, k] / A[k, k]
            A[i, k:] -= m * A[k, k:]
            B[i] -= m * B[k]
    for k in reversed(range(n)):
        B[k] = (B[k] - A[k, k + 1:] @ B[k + 1:]) / A[k, k]
    return B


def interpolate_ld(kvs, vals, nodes):
    """Coefficients (long double) of the tensor-product interpolant of the values `vals` (long double, leading axes = the
    numbers of nodes = dofs per axis; trailing axes kept) at the tensor grid `nodes`."""
    X = np.array(vals, dtype=LD)
    for ax, (kv, nd) in enumerate(zip(kvs, nodes)):
        C = tables_ld(kv, nd)[0]
        Y = np.moveaxis(X, ax, 0)
        shape = Y.shape
        X = np.moveaxis(solve_ld(C, Y.reshape(shape[0], -1)).reshape(shape), 0, ax)
    return X

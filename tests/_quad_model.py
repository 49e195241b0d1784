"""Host model of the quadrature kernels (pyiga_amd/csrc/kern_quad.hip): per-element sums and totals of  W f_k  and of the error
terms  W (u_h - g)^2,  W |grad u_h - grad g|^2  in long double.  Nothing of the library is used: the basis tables are
``_lv_model.collocation_ld`` (Cox-de Boor on the host), the rule is ``numpy.polynomial.legendre.leggauss``, a spline or NURBS
geometry is evaluated from its control net with the same tables (quotient rule for NURBS), the 2x2 / 3x3 inverse is written out.

The rounding bound the GPU test uses (``eps`` = 2^-53 * 2, the float64 machine epsilon), derived as tests/test_spline_eval_gpu.py
derives its own and with no fitted constant:

* u_h at a point is a sum of at most P^dim <= 216 products V_0 V_1 V_2 c:  |delta u_h| <= d_val = 250 eps max|c| prod_k S_k,
  S_k = max_g sum_l |V_k[g][l][d_k]| from the tables (that file's docstring); a parametric derivative likewise with the
  derivative table on its axis (d_par).
* An entry of the geometry Jacobian is such a sum over the control net: e0 = 250 eps max|ctrl| prod_k S_k^geo (the largest over
  the derivative orders).  For NURBS G = N / w and dG = (dN - G dw) / w, so to first order
  |delta J| <= e0 ((1 + max|G|) (1 + max|dw| / min w) + max|J|) / min w; the model takes twice that (dJ).  A B-spline has w = 1,
  dw = 0.  A geometry given as a Jacobian ARRAY has dJ = 0.
* det J is a sum of dim! products of dim entries:  |delta det| <= dim! dim max|J|^(dim-1) dJ + 2 dim! dim eps max|J|^dim; the
  weight W = gw_0 gw_1 gw_2 |det J| therefore has a relative error  g_W <= |delta det| / min|det J| + 4 eps.
* The physical gradient is J^-T times the parametric one:  d_phys = max(d_par) dim max|J^-1|  (that file's bound) plus the
  error of the inverse,  max|gpar| dim^2 max|J^-1|^2 dJ.
* A term t = W d^2 with d = u_h - g (g is the same double on both sides):  |delta t| <= W (2 |d| delta + delta^2) + (g_W + 3 eps) t;
  the gradient term W sum_r d_r^2 likewise with  W sum_r (2 |d_r| d_phys + d_phys^2) + (g_W + (dim + 3) eps) t.  For  t = W f
  (quad sums):  |delta t| <= (g_W + eps) |t|.
* A sum of n terms adds  eps n sum|t|:  n = q^dim for an element; the total adds the  ceil(nelem / 256) + 8  additions of the
  strided sum and the tree of k_quad_total.

``error_model`` / ``quad_model`` return the long-double element sums, totals and these bounds per element and for the total.
"""
import math

import numpy as np

from _lv_model import collocation_ld, LD

EPS = np.finfo(np.float64).eps


def gauss_rule(kv, nqp):
    """Nodes and weights (float64) of the nqp-point Gauss rule on every span of `kv`, span after span."""
    x, w = np.polynomial.legendre.leggauss(nqp)
    mesh = np.unique(np.asarray(kv.kv, dtype=np.float64))
    a, b = mesh[:-1, None], mesh[1:, None]
    return (0.5 * (a + b) + 0.5 * (b - a) * x[None, :]).ravel(), (0.5 * (b - a) * w[None, :]).ravel()


def _expand(Ms, orders, c):
    out = c
    for k, (M, d) in enumerate(zip(Ms, orders)):
        out = np.moveaxis(np.tensordot(M[d], out, axes=(1, k)), 0, k)
    return out


def _S(Ms):
    """S[k][d] = max_g sum_l |V_k[g][l][d]|"""
    return [[float(abs(M[d]).sum(axis=1).max()) for d in range(2)] for M in Ms]


def _det_inv(J):
    """(det, inverse) of the trailing 2x2 / 3x3 matrices in the dtype of J (numpy.linalg has no long double)."""
    dim = J.shape[-1]
    if dim == 2:
        det = J[..., 0, 0] * J[..., 1, 1] - J[..., 0, 1] * J[..., 1, 0]
        adj = np.stack([np.stack([J[..., 1, 1], -J[..., 0, 1]], -1), np.stack([-J[..., 1, 0], J[..., 0, 0]], -1)], -2)
        return det, adj / det[..., None, None]
    c = lambda i, j: J[..., (i + 1) % 3, (j + 1) % 3] * J[..., (i + 2) % 3, (j + 2) % 3] - J[..., (i + 1) % 3, (j + 2) % 3] * J[..., (i + 2) % 3, (j + 1) % 3]
    cof = np.stack([np.stack([c(i, j) for j in range(3)], -1) for i in range(3)], -2)       # cofactor matrix
    det = (J[..., 0, :] * cof[..., 0, :]).sum(-1)
    return det, np.swapaxes(cof, -1, -2) / det[..., None, None]


def geometry_ld(geo, nodes):
    """(X, J, dJ) of a spline / NURBS map at the tensor grid `nodes`: points G + (dim,), Jacobian G + (dim, dim) with
    J[r][c] = d G_r / d xi_c, c in (x, y, z) order (c = 0 belongs to the LAST grid axis), in long double, and the bound dJ on the
    error of a float64 evaluation of J (module docstring)."""
    dim = len(nodes)
    Ms = [collocation_ld(kv, nd) for kv, nd in zip(geo.kvs, nodes)]
    net = np.asarray(geo.coeffs, dtype=np.float64).astype(LD)
    nurbs = net.shape[-1] == dim + 1
    val = _expand(Ms, (0,) * dim, net)
    ders = [_expand(Ms, tuple(1 if k == dim - 1 - c else 0 for k in range(dim)), net) for c in range(dim)]
    S = _S(Ms)
    e0 = 250 * EPS * float(abs(net).max()) * float(np.prod([max(s) for s in S]))
    if nurbs:
        w = val[..., -1:]
        X = val[..., :-1] / w
        J = np.stack([(d[..., :-1] - X * d[..., -1:]) / w for d in ders], axis=-1)
        wmin = float(abs(w).min())
        dwmax = max(float(abs(d[..., -1]).max()) for d in ders)
    else:
        X = val
        J = np.stack(ders, axis=-1)
        wmin, dwmax = 1.0, 0.0
    dJ = 2 * e0 * ((1 + float(abs(X).max())) * (1 + dwmax / wmin) + float(abs(J).max())) / wmin
    return X, J, dJ


def point_error(geo, nodes):
    """Bound on the error of a float64 evaluation of the map itself, X = N / w:  2 e0 (1 + max|X|) / min w  (as dJ above)."""
    dim = len(nodes)
    Ms = [collocation_ld(kv, nd) for kv, nd in zip(geo.kvs, nodes)]
    net = np.asarray(geo.coeffs, dtype=np.float64).astype(LD)
    val = _expand(Ms, (0,) * dim, net)
    e0 = 250 * EPS * float(abs(net).max()) * float(np.prod([s[0] for s in _S(Ms)]))
    if net.shape[-1] == dim + 1:
        return 2 * e0 * (1 + float(abs(val[..., :-1] / val[..., -1:]).max())) / float(abs(val[..., -1]).min())
    return 2 * e0 * (1 + float(abs(val).max()))


def _weights(kvs, geo, jac, nodes, weights):
    """W (long double), its relative error bound g_W, J^-1, dJ"""
    dim = len(kvs)
    if jac is not None:
        J, dJ = np.asarray(jac, dtype=np.float64).astype(LD), 0.0
    else:
        _, J, dJ = geometry_ld(geo, nodes)
    det, Jinv = _det_inv(J)
    gw = np.asarray(weights[0], dtype=np.float64).astype(LD)
    for w in weights[1:]:
        gw = gw[..., None] * np.asarray(w, dtype=np.float64).astype(LD)
    Jmax = float(abs(J).max())
    f = math.factorial(dim) * dim
    ddet = f * Jmax ** (dim - 1) * dJ + 2 * f * EPS * Jmax ** dim
    g_W = ddet / float(abs(det).min()) + 4 * EPS
    return gw * abs(det), g_W, Jinv, dJ


def _element_sums(t, q):
    """[nk][G0][G1][G2] -> [nk][S0][S1][S2] (any dim): sums over the q points per span and axis"""
    nk, G = t.shape[0], t.shape[1:]
    shp = (nk,) + tuple(x for g in G for x in (g // q, q))
    return t.reshape(shp).sum(axis=tuple(2 + 2 * k for k in range(len(G))))


def _finish(t, dt, q):
    """terms t and their error bounds dt (both [nk][G..]) -> element sums, totals and the two bounds"""
    dim = t.ndim - 1
    elem = _element_sums(t, q)
    n_el = q ** dim
    eb = _element_sums(dt, q) + EPS * n_el * _element_sums(abs(t), q)
    nelem = int(np.prod(elem.shape[1:]))
    axes = tuple(range(1, 1 + dim))
    n_tot = n_el + -(-nelem // 256) + 8
    tb = dt.sum(axis=axes) + EPS * n_tot * abs(t).sum(axis=axes)
    return {'elem': elem, 'total': elem.sum(axis=axes), 'elem_bound': eb.astype(np.float64), 'total_bound': tb.astype(np.float64)}


def _rule(kvs, nodes, weights):
    q = max(int(kv.p) for kv in kvs) + 1
    if nodes is None:
        rules = [gauss_rule(kv, q) for kv in kvs]
        nodes, weights = [r[0] for r in rules], [r[1] for r in rules]
    return q, nodes, weights


def quad_model(kvs, geo, fvals, jac=None, nodes=None, weights=None):
    """sum W f_k, k over the arrays `fvals` (float64, on the Gauss grid).  `geo`: a spline / NURBS map, or `jac` the Jacobians on
    the grid; `nodes` / `weights`: the rule per axis (default: this module's own ``gauss_rule`` with max p + 1 points)."""
    q, nodes, weights = _rule(kvs, nodes, weights)
    W, g_W, _, _ = _weights(kvs, geo, jac, nodes, weights)
    t = np.stack([W * np.asarray(f, dtype=np.float64).astype(LD) for f in fvals])
    return _finish(t, (g_W + EPS) * abs(t), q)


def error_model(kvs, geo, c, want_grad, exact=None, jac=None, nodes=None, weights=None, d_exact=(0.0, 0.0)):
    """Error sums of the spline with the dofs `c` (shape ndofs).  `exact`: None, or [values, d/dx, d/dy[, d/dz]] float64 arrays
    on the Gauss grid with None for an absent one (= 0).  `d_exact`: how far the exact value / an exact partial the device uses may
    be from those arrays (evaluated there, at points it computes itself); added to d_val / d_phys.  Returns the dict of
    ``_finish`` with 1 + want_grad quantities."""
    dim = len(kvs)
    q, nodes, weights = _rule(kvs, nodes, weights)
    W, g_W, Jinv, dJ = _weights(kvs, geo, jac, nodes, weights)
    Ms = [collocation_ld(kv, nd) for kv, nd in zip(kvs, nodes)]
    S = _S(Ms)
    cl = np.asarray(c, dtype=np.float64).astype(LD)
    cmax = float(abs(cl).max())
    ex = list(exact) if exact is not None else [None] * (1 + dim)
    arr = lambda a: 0 if a is None else np.asarray(a, dtype=np.float64).astype(LD)
    d0 = _expand(Ms, (0,) * dim, cl) - arr(ex[0])
    d_val = 250 * EPS * cmax * float(np.prod([S[k][0] for k in range(dim)])) + d_exact[0]
    t = [W * d0 * d0]
    dt = [W * (2 * abs(d0) * d_val + d_val ** 2) + (g_W + 3 * EPS) * t[0]]
    if want_grad:
        gpar, d_par = [], []
        for r in range(dim):                                      # (x, y, z) order: x belongs to the LAST grid axis
            orders = tuple(1 if k == dim - 1 - r else 0 for k in range(dim))
            gpar.append(_expand(Ms, orders, cl))
            d_par.append(250 * EPS * cmax * float(np.prod([S[k][orders[k]] for k in range(dim)])))
        gpar = np.stack(gpar, axis=-1)
        gphys = (Jinv * gpar[..., :, None]).sum(axis=-2)          # D_r = sum_c Jinv[c][r] gpar[c]
        Jimax = float(abs(Jinv).max())
        d_phys = max(d_par) * dim * Jimax + float(abs(gpar).max()) * dim * dim * Jimax ** 2 * dJ + d_exact[1]
        tg, dtg = 0, 0
        for r in range(dim):
            dr = gphys[..., r] - arr(ex[1 + r])
            tg = tg + dr * dr
            dtg = dtg + 2 * abs(dr) * d_phys + d_phys ** 2
        t.append(W * tg)
        dt.append(W * dtg + (g_W + (dim + 3) * EPS) * t[1])
    return _finish(np.stack(t), np.stack(dt), q)

"""Long-double restatement of one matrix entry of the entry-wise kernels (pyiga_amd/csrc/kern_entries.hip), plain numpy: no GPU,
no library load.

The entry kernels are isolated by taking their two inputs as given (both are tested elsewhere: the fields in
tests/test_fields_kernels_gpu.py, the basis tables in tests/test_entries_kernels_gpu.py):

- ``fields``: the quadrature fields of the patch, shape (F, G0_loc, L1[, L2]) over the resident window (``DevicePatch.fields``;
  on the host, the oracle's fields brought into the same layout),
- ``tables``: per axis ``AxisTable``: V[g][a][slot] (slot 0 = value, 1 = first derivative of the a-th active function at Gauss
  node g) and the integer tables of the knot vector.

What is restated from ``entry_value``: entry (i, j) is  sum over the Gauss points of the support intersection of
sum_t  F_t * prod_k u_k[slot] * prod_k v_k[slot]  (u: column j, v: row i).  The terms of each kind, as (field, slots of u per
axis, slots of v per axis); "jet index" c: 0 = value, 1 = derivative along the LAST grid axis, 2 = along the one before, ..:

- mass: (0, value, value);
- stiffness: fields = upper triangle of the symmetric B over the jet indices 1..d, row-major: B[a][b] Du[b] Dv[a];
- convdiff (3D): stiffness + fields 6..8 = beta_b: beta_b Du[b] Dv[0];
- form, physical table: field t <-> form_ab[t] = 4 a + b for a, b over the jet indices whose block (value / derivative) is
  present in the table: F_t Du[b] Dv[a];
- form, parametric (set_pform): term k has masks (mv, mu) over the grid axes, bit k = axis k takes slot 1.

C_KIND: roundings on one monomial F * Du * Dv inside one Gauss point's term, counted from entry_value (the accumulation over
the points is the ``npts`` of the bound):
- mass 2D ``((u0*u1)*(v0*v1))*f``: 3;  mass 3D ``((u0*u1*u2)*(v0*v1*v2))*f``: 2 + 2 + 1 + 1 = 6;
- stiffness 2D ``((f0*du10 + f1*du01)*dv10) + (..)*dv01``: du 1, f*du 1, inner add 1, dv 1, *dv 1, outer add 1 = 6;
- stiffness 3D: du 2, f*du 1, inner adds 2, dv 2, *dv 1, outer adds 2 = 10;
- convdiff: the stiffness monomials get the add of the convection part: 11 (the convection monomials: 2+1+2+2+1+1 = 9);
- form, per term ``e += (F*du)*dv``: du and dv (1 each in 2D, 2 in 3D), two products, one add: 5 in 2D, 7 in 3D; times the
  number of terms (the first term sees every later add).
The bound  (npts + C_KIND) * 2**-53 * mag  holds for any order of the sum over the points (one thread, or 64 lanes and a shuffle
tree: adding the exact zeros of idle lanes does not round), FMA contraction only removes roundings.
"""
from typing import NamedTuple

import numpy as np

LD = np.longdouble
U = 2.0 ** -53


class AxisTable(NamedTuple):
    p: int
    N: int                 # dofs
    n: int                 # spans
    q: int                 # Gauss points per span
    fa: np.ndarray         # first active dof of every span
    mslo: np.ndarray       # first span of every dof's support
    mshi: np.ndarray       # one past its last span
    jlo: np.ndarray        # first column coupled to dof i
    jhi: np.ndarray        # one past the last
    V: object              # (G, p + 1, 2) long double, or None (integer bookkeeping only)


class Window(NamedTuple):
    """The resident Gauss points: planes [g0, g0 + G0) of axis 0, [b1, b1 + L1) of axis 1, [b2, b2 + L2) of axis 2."""
    g0: int
    G0: int
    b1: int
    L1: int
    b2: int
    L2: int


def axis_table(kv, q, V=None):
    p = int(kv.p)
    ms = np.asarray(kv.mesh_support_idx_all(), dtype=np.int64)
    mslo, mshi = ms[:, 0], ms[:, 1]
    fa = np.asarray(kv.mesh_span_indices(), dtype=np.int64) - p
    jlo = np.searchsorted(mshi, mslo, side='right')            # first j with mshi[j] > mslo[i]
    jhi = np.searchsorted(mslo, mshi, side='left')             # first j with mslo[j] >= mshi[i]
    if V is not None:
        V = np.asarray(V, dtype=LD)
        assert V.shape == (int(kv.numspans) * q, p + 1, 2)
    return AxisTable(p, int(kv.numdofs), int(kv.numspans), int(q), fa, mslo, mshi, jlo, jhi, V)


def tables_from_active_deriv(kvs, q, derivs):
    """derivs[k]: (>= 2, p + 1, G_k) values and derivatives at the Gauss nodes of axis k (the layout of ``active_deriv``)."""
    return [axis_table(kv, q, np.moveaxis(np.asarray(d)[:2], (0, 1, 2), (2, 1, 0))) for kv, d in zip(kvs, derivs)]


def whole_window(axes):
    G = [a.n * a.q for a in axes] + [1]
    return Window(0, G[0], 0, G[1], 0, G[2])


def slab_window(axes, row0):
    """The Gauss planes of axis 0 that the supports of the owned dofs row0[0] .. row0[1] - 1 touch (igx_patch_create)."""
    a0 = axes[0]
    s_lo, s_hi = int(a0.mslo[row0[0]]), int(a0.mshi[row0[1] - 1])
    w = whole_window(axes)
    return w._replace(g0=s_lo * a0.q, G0=(s_hi - s_lo) * a0.q)


def box_window(axes, bbox):
    q = axes[0].q
    b = [(lo * q, (hi - lo) * q) for lo, hi in bbox] + [(0, 1)]
    return Window(b[0][0], b[0][1], b[1][0], b[1][1], b[2][0], b[2][1])


# ---------------------------------------------------------------------------------------------
# the terms of every kind
def jet_slots(dim, c):
    """Slots per grid axis of jet index c: the derivative c >= 1 acts on grid axis dim - c."""
    return tuple(1 if c >= 1 and k == dim - c else 0 for k in range(dim))


def physical_form_ab(dim, present):
    """form_ab of a physical table (set_form_impl): `present` = set of (r, s) with a coefficient."""
    blk = {(r > 0, s > 0) for r, s in present}
    return [4 * a + b for a in range(dim + 1) for b in range(dim + 1) if (a > 0, b > 0) in blk]


def terms_of(dim, kind, form=None):
    """[(field, slots of u, slots of v)].  form: ('phys', form_ab list) or ('par', [(mv, mu), ..])."""
    if kind == 'mass':
        return [(0, jet_slots(dim, 0), jet_slots(dim, 0))]
    if kind in ('stiffness', 'convdiff'):
        sym, n = {}, 0
        for a in range(1, dim + 1):
            for b in range(a, dim + 1):
                sym[(a, b)] = sym[(b, a)] = n
                n += 1
        out = [(sym[(a, b)], jet_slots(dim, b), jet_slots(dim, a)) for a in range(1, dim + 1) for b in range(1, dim + 1)]
        if kind == 'convdiff':
            assert dim == 3
            out += [(5 + b, jet_slots(3, b), jet_slots(3, 0)) for b in range(1, 4)]
        return out
    assert kind == 'form' and form is not None
    if form[0] == 'phys':
        return [(t, jet_slots(dim, ab & 3), jet_slots(dim, ab >> 2)) for t, ab in enumerate(form[1])]
    return [(t, tuple((mu >> k) & 1 for k in range(dim)), tuple((mv >> k) & 1 for k in range(dim))) for t, (mv, mu) in enumerate(form[1])]


def c_kind(dim, kind, form=None):
    if kind == 'mass':
        return 3 if dim == 2 else 6
    if kind == 'stiffness':
        return 6 if dim == 2 else 10
    if kind == 'convdiff':
        return 11
    return (5 if dim == 2 else 7) * len(form[1])


# ---------------------------------------------------------------------------------------------
def unravel(axes, I):
    """Per-axis indices of the ravelled dof I, or None at or past prod(N)."""
    I = int(I)
    out = []
    for a in reversed(axes[1:]):
        out.append(I % a.N)
        I //= a.N
    if I >= axes[0].N:
        return None
    return tuple([I] + out[::-1])


def overlap(axes, I, J):
    """Per axis (first Gauss point, number of Gauss points) of the support intersection; None: class 'zero'."""
    i, j = unravel(axes, I), unravel(axes, J)
    if i is None or j is None:
        return None
    out = []
    for a, ik, jk in zip(axes, i, j):
        lo, hi = max(a.mslo[ik], a.mslo[jk]), min(a.mshi[ik], a.mshi[jk])
        if lo >= hi:
            return None
        out.append((int(lo) * a.q, int(hi - lo) * a.q))
    return out


def classify(axes, window, I, J):
    """'zero' | 'nan' | 'value', and the overlap.  From the knot vectors alone."""
    ov = overlap(axes, I, J)
    if ov is None:
        return 'zero', None
    w = [(window.g0, window.G0), (window.b1, window.L1), (window.b2, window.L2)]
    for (g, n), (b, L) in zip(ov, w):
        if g < b or g + n > b + L:
            return 'nan', ov
    return 'value', ov


def box_points(ov):
    """The points the 64 lanes of k_entries_wave split: axis 1 [x axis 2]."""
    return int(np.prod([n for _, n in ov[1:]]))


class Entry(NamedTuple):
    cls: str
    value: object          # long double (0 unless cls == 'value')
    mag: object            # the same sum over absolute values
    npts: int
    nbox: int


def entry(axes, window, fields, terms, I, J, mutate=None, fields_mag=None):
    """One entry.  mutate: None, 'shift' (the field read one point further along the last axis, cyclically inside the window),
    'drop1' (the last Gauss point of the axis-1 overlap missing), 'drop64' (box points with index >= 64 missing).  fields_mag:
    fields to take the magnitude from (default: |fields|)."""
    cls, ov = classify(axes, window, I, J)
    if cls != 'value':
        return Entry(cls, LD(0), LD(0), 0, 0 if ov is None else box_points(ov))
    dim = len(axes)
    i, j = unravel(axes, I), unravel(axes, J)
    uv = []
    for k, a in enumerate(axes):
        g = np.arange(ov[k][0], ov[k][0] + ov[k][1])
        f = a.fa[g // a.q]
        uv.append((a.V[g, j[k] - f, :], a.V[g, i[k] - f, :]))              # (ng_k, 2) each
    w0 = (window.g0, window.b1, window.b2)
    sl = tuple(slice(ov[k][0] - w0[k], ov[k][0] - w0[k] + ov[k][1]) for k in range(dim))
    F = np.asarray(fields)
    if mutate == 'shift':
        F = np.roll(F, -1, axis=-1)
    Fm = abs(F) if fields_mag is None else np.asarray(fields_mag)
    keep = np.ones([n for _, n in ov], dtype=bool)
    if mutate == 'drop1':
        keep[:, -1] = False
    if mutate == 'drop64':
        box = np.arange(box_points(ov)).reshape([n for _, n in ov[1:]])
        keep[:, box >= 64] = False
    val = mag = LD(0)
    for t, us, vs in terms:
        prod = None
        for k in range(dim):
            f = uv[k][0][:, us[k]] * uv[k][1][:, vs[k]]
            prod = f if prod is None else prod[..., None] * f
        prod = np.where(keep, prod, LD(0))
        val = val + (prod * F[(t,) + sl].astype(LD)).sum(dtype=LD)
        mag = mag + (abs(prod) * Fm[(t,) + sl].astype(LD)).sum(dtype=LD)
    return Entry(cls, val, mag, int(np.prod([n for _, n in ov])), box_points(ov))


def bound(e, c):
    return (e.npts + c) * U * e.mag


def entries(axes, window, fields, terms, idx, **kw):
    return [entry(axes, window, fields, terms, I, J, **kw) for I, J in np.asarray(idx, dtype=np.int64)]


# ---------------------------------------------------------------------------------------------
# the CSR pattern from the per-axis column ranges
def row_pattern(axes, I):
    i = unravel(axes, I)
    cols = np.zeros(1, dtype=np.int64)
    for a, ik in zip(axes, i):
        cols = (cols[:, None] * a.N + np.arange(a.jlo[ik], a.jhi[ik])[None, :]).ravel()
    return cols


def pattern(axes, row0=None):
    """(indptr, indices) of the rows of the dof planes row0[0] .. row0[1] - 1 of axis 0 (all rows without), local indptr."""
    plane = int(np.prod([a.N for a in axes[1:]]))
    lo, hi = (0, axes[0].N) if row0 is None else row0
    rows = [row_pattern(axes, I) for I in range(lo * plane, hi * plane)]
    indptr = np.concatenate(([0], np.cumsum([len(r) for r in rows])))
    return indptr, np.concatenate(rows)


# ---------------------------------------------------------------------------------------------
# Piegl-Tiller A2.3 in long double (the oracle's active_deriv_single with np.longdouble)
def findspan(kv, p, u):
    n = kv.shape[0]
    if u >= kv[n - p - 1]:
        return n - p - 2
    a, b = 0, n - 1
    while b - a > 1:
        c = a + (b - a) // 2
        if kv[c] > u:
            b = c
        else:
            a = c
    return a


def active_deriv_single_ld(kv, p, u, numderiv, dtype=LD):
    kv = np.asarray(kv, dtype=np.float64).astype(dtype)
    u = dtype(u)
    NDU = np.zeros((p + 1, p + 1), dtype=dtype)
    result = np.zeros((numderiv + 1, p + 1), dtype=dtype)
    left = np.zeros(p + 1, dtype=dtype)
    right = np.zeros(p + 1, dtype=dtype)
    span = findspan(kv, p, u)
    NDU[0, 0] = 1
    for j in range(1, p + 1):
        left[j - 1] = u - kv[span + 1 - j]
        right[j - 1] = kv[span + j] - u
        saved = dtype(0)
        for r in range(j):
            NDU[j, r] = right[r] + left[j - r - 1]
            temp = NDU[r, j - 1] / NDU[j, r]
            NDU[r, j] = saved + right[r] * temp
            saved = left[j - r - 1] * temp
        NDU[j, j] = saved
    result[0] = NDU[:, p]
    a1 = np.zeros(p + 2, dtype=dtype)
    a2 = np.zeros(p + 2, dtype=dtype)
    for r in range(p + 1):
        a1[0] = 1
        fac = p
        for k in range(1, numderiv + 1):
            rk, pk = r - k, p - k
            d = dtype(0)
            if pk < 0:
                result[k, r] = 0
                continue
            if r >= k:
                a2[0] = a1[0] / NDU[pk + 1, rk]
                d = a2[0] * NDU[rk, pk]
            j1 = 1 if rk >= -1 else -rk
            j2 = k - 1 if r - 1 <= pk else p - r
            for j in range(j1, j2 + 1):
                a2[j] = (a1[j] - a1[j - 1]) / NDU[pk + 1, rk + j]
                d += a2[j] * NDU[rk + j, pk]
            if r <= pk:
                a2[k] = -a1[k - 1] / NDU[pk + 1, r]
                d += a2[k] * NDU[r, pk]
            result[k, r] = d * fac
            fac *= pk
            a1, a2 = a2, a1
    return result


def active_deriv_ld(kv, u, numderiv, dtype=LD):
    """(numderiv + 1, p + 1, len(u)) long double (or the same arithmetic in `dtype`)."""
    u = np.asarray(u, dtype=np.float64)
    out = np.zeros((numderiv + 1, int(kv.p) + 1, u.shape[0]), dtype=dtype)
    for i in range(u.shape[0]):
        out[:, :, i] = active_deriv_single_ld(kv.kv, int(kv.p), u[i], numderiv, dtype)
    return out


def table_deviation(dev, ref):
    """Per derivative order: max |dev - ref| / max |ref|, in units of 2**-53."""
    return [float(abs(np.asarray(dev[k]).astype(LD) - ref[k]).max() / abs(ref[k]).max()) / U for k in range(ref.shape[0])]


def gauss_nodes(kv, q):
    """The iterated Gauss rule of setup_axis: nodes = h * x + m per span (same expression, same bits)."""
    gx = np.polynomial.legendre.leggauss(q)[0]
    mesh = np.asarray(kv.mesh, dtype=np.float64)
    m, h = 0.5 * (mesh[:-1] + mesh[1:]), 0.5 * (mesh[1:] - mesh[:-1])
    return (h[:, None] * gx[None, :] + m[:, None]).ravel()

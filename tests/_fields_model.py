"""Restatement of the geometry-field kernels and of the single-launch 2D kernel (pyiga_amd/csrc/kern_basis.hip, geo_device.h) in
plain numpy: no GPU, no library load, no oracle.

The arithmetic is written once and runs in the dtype it is given: ``np.longdouble`` is the reference, ``np.float64`` the
yardstick.  D of a field is the largest deviation of the float64 run from the long-double run over a case, divided by the largest
magnitude of that field over the case; the device is allowed MARGIN * D with a floor of FLOOR * 2**-53, relative to the same
magnitude (``tolerance``).  The margin covers the other contraction orders of the device (line-wise, plane-wise, FMA): each is a
valid double evaluation with an error of the size of D, not equal to it.

Geometry: a tensor-product B-spline or NURBS map; a NURBS control net is premultiplied, weight last, and goes through the
quotient rule.  Jacobian convention of geo_device.h: J[..., r, c] = d G_r / d xi_c with c = 0 the LAST grid axis.

Fields, laid out as ``DevicePatch.fields`` returns them, (F, G0_loc, L1[, L2]) over a Window (_entries_model):
- mass: W = GW |det J|;
- stiffness: upper triangle of W J^-1 J^-T, row-major;
- convdiff (3D): c W J^-1 J^-T and beta_a = W sum_r JI[a][r] b_r, b = (y, -x, 1);
- form, physical table: M = W T P T^t, T = diag(1, J^-1), the terms of form_ab only;
- form, parametric: GW * coefficient_k.

Dense 2D assembly (``assemble2d``): sum-factorised like k_single2d -- K[i0, j0, y, g1] over the support intersection of axis 0,
then the contraction of axis 1 -- stored by bands: out[i0, e, i1, d] is entry (row (i0, i1), column (i0 + e - p0, i1 + d - p1)).

C_SINGLE2D: roundings on one monomial of k_single2d beyond the two accumulations.  The kernel forms u * v of axis 0 (1), adds
n0 FMA terms (n0 roundings at most), forms u * v of axis 1 (1), adds n1 FMA terms (n1), and the stiffness form ends with
(T0 + T3) + (T1 + T2) (2): n0 + n1 + 4, and n0 + n1 <= n0 n1 + 1 = npts + 1.  So c = 5 for stiffness, 3 for mass, in
(npts + c) * 2**-53 * mag  (+ the fields' tolerance carried through the same sum, ``mag`` taken with that tolerance as field).
"""
import numpy as np

import _entries_model as em

LD = np.longdouble
U = 2.0 ** -53
MARGIN, FLOOR = 8, 16
C_SINGLE2D = {'mass': 3, 'stiffness': 5}

FIELD_MUTANTS = ('colb', 'gw_neighbour', 'no_b1', 'slab_plane', 'no_wprime', 'swap_f12', 'drop_point', 'drop_line')
ASSEMBLY_MUTANTS = ('swap_T12', 'drop1')


class KV:
    """The two attributes active_deriv_ld reads."""
    def __init__(self, knots, p):
        self.kv, self.p = np.asarray(knots, dtype=np.float64), int(p)


class Map:
    """kvs: [(knots, degree)] per grid axis; ctrl: (N0, N1[, N2], nc) float64, NURBS premultiplied with the weight last."""
    def __init__(self, kvs, ctrl, nurbs):
        self.kvs = [(np.asarray(k, dtype=np.float64), int(p)) for k, p in kvs]
        self.ctrl = np.asarray(ctrl, dtype=np.float64)
        self.nurbs = bool(nurbs)
        self.dim = len(self.kvs)
        assert self.ctrl.shape[:-1] == tuple(len(k) - p - 1 for k, p in self.kvs)
        self.ncomp = self.ctrl.shape[-1] - (1 if nurbs else 0)       # (the geometry of a patch: ncomp = dim)


def basis_matrices(knots, p, nodes, dtype):
    """(2, len(nodes), N): values and first derivatives of every basis function at the nodes (zero outside the support)."""
    nodes = np.asarray(nodes, dtype=np.float64)
    B = em.active_deriv_ld(KV(knots, p), nodes, 1, dtype)                      # (2, p + 1, n)
    N = len(knots) - p - 1
    M = np.zeros((2, len(nodes), N), dtype=dtype)
    kl = np.asarray(knots, dtype=np.float64).astype(LD)
    for g, u in enumerate(nodes):
        fa = em.findspan(kl, p, LD(u)) - p
        M[:, g, fa:fa + p + 1] = B[:, :, g]
    return M


def eval_map(geo, nodes, dtype, mutate=None):
    """(ev, J): value (.., ncomp) and Jacobian (.., ncomp, dim), c = 0 the last grid axis, at the tensor grid of `nodes`."""
    dim, nco = geo.dim, geo.ncomp
    ctrl = geo.ctrl.astype(dtype)
    if mutate == 'colb':                                                       # the control column one to the right
        ctrl = np.roll(ctrl, -1, axis=dim - 1)
    M = [basis_matrices(k, p, nodes[a], dtype) for a, (k, p) in enumerate(geo.kvs)]

    def contract(orders):
        H = ctrl
        for a in range(dim):                                                   # axis a of H: control index -> grid index
            H = np.moveaxis(np.tensordot(M[a][orders[a]], H, axes=([1], [a])), 0, a)
        return H
    val = contract([0] * dim)
    der = [contract([1 if a == k else 0 for a in range(dim)]) for k in range(dim)]      # along grid axis k
    if geo.nurbs:
        W = val[..., -1:]
        ev = val[..., :nco] / W
        cols = []
        for c in range(dim):
            dk = der[dim - 1 - c]
            dW = dk[..., -1:] * (0 if mutate == 'no_wprime' else 1)
            cols.append((dk[..., :nco] * W - val[..., :nco] * dW) / (W * W))
    else:
        ev = val
        cols = [der[dim - 1 - c] for c in range(dim)]
    return ev, np.stack(cols, axis=-1)


def inverse(J):
    """(J^-1, det) by cofactors; JI[..., a, r] = d xi_a / d x_r."""
    d = J.shape[-1]
    if d == 2:
        det = J[..., 0, 0] * J[..., 1, 1] - J[..., 0, 1] * J[..., 1, 0]
        JI = np.stack([np.stack([J[..., 1, 1], -J[..., 0, 1]], -1), np.stack([-J[..., 1, 0], J[..., 0, 0]], -1)], -2)
        return JI / det[..., None, None], det
    cof = np.empty_like(J)
    for a in range(3):
        for r in range(3):
            i0, i1 = [k for k in range(3) if k != r]
            j0, j1 = [k for k in range(3) if k != a]
            cof[..., a, r] = (-1) ** (a + r) * (J[..., i0, j0] * J[..., i1, j1] - J[..., i0, j1] * J[..., i1, j0])
    det = J[..., 0, 0] * cof[..., 0, 0] + J[..., 0, 1] * cof[..., 1, 0] + J[..., 0, 2] * cof[..., 2, 0]
    return cof / det[..., None, None], det


def window_axes(window, dim):
    w = [(window.g0, window.G0), (window.b1, window.L1), (window.b2, window.L2)]
    return w[:dim]


def fields(kind, dim, window, gauss, dtype, geo=None, jac=None, coeff=None, form=None, mutate=None, lpb=1):
    """The fields of `kind` over `window`, (F, G0, L1[, L2]) in dtype.

    gauss: per axis (nodes, weights) of the whole axis (float64).  geo: Map, or jac: the Jacobian array over the window (a
    Jacobian-array geometry).  coeff (convdiff): array over the window, or ('affine', (c0, c1, c2, c3)).  form: ('phys',
    P (dim + 1, dim + 1) nested list of arrays over the window or None, form_ab) or ('par', [arrays over the window]).
    mutate: one of FIELD_MUTANTS (lpb: lines per block of 'drop_line')."""
    wa = window_axes(window, dim)
    if mutate == 'no_b1':                                                      # g1 not offset by b1
        wa[1] = (0, wa[1][1])
    if mutate == 'slab_plane':                                                 # the slab's first plane off by one
        n0 = len(gauss[0][0])
        wa[0] = (wa[0][0] + 1 if wa[0][0] + 1 + wa[0][1] <= n0 else wa[0][0] - 1, wa[0][1])
    nodes = [np.asarray(gauss[a][0])[lo:lo + n] for a, (lo, n) in enumerate(wa)]
    wts = [np.asarray(gauss[a][1])[lo:lo + n].astype(dtype) for a, (lo, n) in enumerate(wa)]
    if mutate == 'gw_neighbour':                                               # the Gauss weight of the neighbouring point
        wts[dim - 1] = np.roll(wts[dim - 1], -1)
    GW = wts[0]
    for a in range(1, dim):
        GW = GW[..., None] * wts[a]
    if geo is not None:
        ev, J = eval_map(geo, nodes, dtype, mutate)
    else:
        ev, J = None, np.asarray(jac, dtype=np.float64).astype(dtype)
    JI, det = inverse(J)
    W = GW * abs(det)
    tri = [(a, b) for a in range(dim) for b in range(a, dim)]
    if kind == 'mass':
        F = [W]
    elif kind in ('stiffness', 'convdiff'):
        B = np.einsum('...ar,...br->...ab', JI, JI)
        c = 1
        if kind == 'convdiff':
            if isinstance(coeff, tuple):
                cc = [dtype(v) for v in coeff[1]]
                c = cc[0] + cc[1] * ev[..., 0] + cc[2] * ev[..., 1] + cc[3] * ev[..., 2]
            else:
                c = np.asarray(coeff, dtype=np.float64).astype(dtype)
        F = [c * W * B[..., a, b] for a, b in tri]
        if kind == 'stiffness' and dim == 2 and mutate == 'swap_f12':
            F[1], F[2] = F[2], F[1]
        if kind == 'convdiff':
            b = np.stack([ev[..., 1], -ev[..., 0], np.ones_like(ev[..., 0])], -1)
            F += [W * np.einsum('...r,...r->...', JI[..., a, :], b) for a in range(3)]
    elif form[0] == 'par':
        F = [GW * np.asarray(c, dtype=np.float64).astype(dtype) for c in form[1]]
    else:
        nj = dim + 1
        T = np.zeros(J.shape[:-2] + (nj, nj), dtype=dtype)
        T[..., 0, 0] = 1
        T[..., 1:, 1:] = JI
        P = np.zeros_like(T)
        for r in range(nj):
            for s in range(nj):
                if form[1][r][s] is not None:
                    P[..., r, s] = np.asarray(form[1][r][s], dtype=np.float64).astype(dtype)
        M = np.einsum('...ar,...rs,...bs->...ab', T, P, T)
        F = [W * M[..., ab >> 2, ab & 3] for ab in form[2]]
    F = np.stack([np.broadcast_to(f, GW.shape) for f in F]).astype(dtype)
    if mutate == 'drop_point':                                                 # the last point of a line missing
        F[..., -1] = 0
    if mutate == 'drop_line':                                                  # the last line of a block missing
        L = F.reshape(F.shape[0], -1, F.shape[-1])
        L[:, [min(b + lpb, L.shape[1]) - 1 for b in range(0, L.shape[1], lpb)], :] = 0
    return F


def tolerance(F64, FLD):
    """(absolute tolerance per field, D per field, magnitude per field)."""
    ax = tuple(range(1, FLD.ndim))
    mag = abs(FLD).max(axis=ax)
    D = abs(F64.astype(LD) - FLD).max(axis=ax) / mag
    return np.maximum(MARGIN * D, FLOOR * U) * mag, D, mag


def deviation(F, FLD, tol):
    """Largest |F - FLD| / tol over every field (NaN counts as infinite)."""
    r = abs(np.asarray(F).astype(LD) - FLD) / tol.reshape((-1,) + (1,) * (FLD.ndim - 1))
    return float(np.inf if np.isnan(r).any() else r.max())


# ---------------------------------------------------------------------------------------------
# the dense (banded) long-double 2D assembly
def _dofval(a, j, h):
    """V[h, j - fa(h), :] of dof j at Gauss point h, zero outside the support: (.., 2)."""
    loc = j - a.fa[h // a.q]
    ok = (loc >= 0) & (loc <= a.p) & (j >= 0) & (j < a.N)
    return np.where(ok[..., None], a.V[h, np.clip(loc, 0, a.p), :], LD(0))


def _axis_pairs(a):
    """Per (dof i, offset e): the Gauss points of the support of i (N, Wd), their validity, values of i (N, Wd, 2), of the
    partner i + e - p (N, 2p + 1, Wd, 2), the number of points of the support intersection (N, 2p + 1)."""
    Wd = (a.p + 1) * a.q
    i = np.arange(a.N)
    h = a.mslo[:, None] * a.q + np.arange(Wd)[None, :]
    valid = h < a.mshi[:, None] * a.q
    h = np.where(valid, h, 0)
    vi = np.where(valid[..., None], _dofval(a, i[:, None], h), LD(0))
    j = i[:, None] + np.arange(-a.p, a.p + 1)[None, :]
    vj = np.where(valid[:, None, :, None], _dofval(a, j[:, :, None], h[:, None, :]), LD(0))
    jc = np.clip(j, 0, a.N - 1)
    n = np.maximum(np.minimum(a.mshi[:, None], a.mshi[jc]) - np.maximum(a.mslo[:, None], a.mslo[jc]), 0) * a.q
    n = np.where((j >= 0) & (j < a.N), n, 0)
    last = np.minimum(a.mshi[:, None], a.mshi[jc]) * a.q - 1                    # last point of the intersection
    return h, vi, vj, n, last


def assemble2d(axes, F, kind, Fmag=None, mutate=None):
    """(val, mag, npts), each [i0, e, i1, d]: entry of row (i0, i1), column (i0 + e - p0, i1 + d - p1) of the whole patch.

    F: fields (NF, G0, G1) of the whole patch; Fmag: fields to take the magnitude with (default |F|).  mutate: 'swap_T12' (the
    axis-1 factors of terms 1 and 2 exchanged), 'drop1' (the last Gauss point of every axis-1 overlap missing)."""
    a0, a1 = axes
    terms = em.terms_of(2, kind)
    if mutate == 'swap_T12' and kind == 'stiffness':
        (f1, u1, v1), (f2, u2, v2) = terms[1], terms[2]
        terms[1], terms[2] = (f1, (u1[0], u2[1]), (v1[0], v2[1])), (f2, (u2[0], u1[1]), (v2[0], v1[1]))
    F = np.asarray(F).astype(LD)
    Fm = abs(F) if Fmag is None else np.asarray(Fmag).astype(LD)
    h0, vi0, vj0, n0, _ = _axis_pairs(a0)
    h1, vi1, vj1, n1, last1 = _axis_pairs(a1)
    if mutate == 'drop1':
        vj1 = np.where((h1[:, None, :] == last1[:, :, None])[..., None], LD(0), vj1)
    val = mag = LD(0)
    for t, us, vs in terms:
        # axis 0: K[i0, e, g1] = sum_w (u * v)[i0, e, w] * F_t[h0[i0, w], g1]
        pr0 = vj0[..., us[0]] * vi0[:, None, :, vs[0]]                          # (N0, E, W0)
        K = np.einsum('iew,iwg->ieg', pr0, F[t][h0])
        Km = np.einsum('iew,iwg->ieg', abs(pr0), Fm[t][h0])
        pr1 = vj1[..., us[1]] * vi1[:, None, :, vs[1]]                          # (N1, D, W1)
        Kg, Kmg = K[:, :, h1], Km[:, :, h1]                                     # (N0, E, N1, W1)
        val = val + np.einsum('iekw,kdw->iekd', Kg, pr1)
        mag = mag + np.einsum('iekw,kdw->iekd', Kmg, abs(pr1))
    return val, mag, n0[:, :, None, None] * n1[None, None, :, :]


def csr_order(axes, row0=None):
    """Index arrays (i0, e, i1, d) of the CSR values of the dof planes row0[0] .. row0[1] - 1 (all rows without) in the
    canonical order: rows (i0, i1), per row the columns j0 of axis 0, then j1 of axis 1."""
    a0, a1 = axes
    lo, hi = (0, a0.N) if row0 is None else row0
    out = [[], [], [], []]
    for i0 in range(lo, hi):
        e = np.arange(a0.jlo[i0], a0.jhi[i0]) - i0 + a0.p
        for i1 in range(a1.N):
            d = np.arange(a1.jlo[i1], a1.jhi[i1]) - i1 + a1.p
            E, Dd = np.meshgrid(e, d, indexing='ij')
            out[0].append(np.full(E.size, i0)); out[1].append(E.ravel())
            out[2].append(np.full(E.size, i1)); out[3].append(Dd.ravel())
    return tuple(np.concatenate(o) for o in out)


def single2d_bound(kind, mag, npts, magF):
    return (npts + C_SINGLE2D[kind]) * U * mag + magF

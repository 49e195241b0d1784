"""Host model of the device saddle-point solver (csrc/solve_saddle.hip): plain NumPy / SciPy, no GPU, no library load.

* the transposed tables ``ilo | ihi | rpt`` and the transposed layout of a pair matrix, built from ``jlo / jhi / rp`` as
  igx_solver_create_saddle and k_pair_transpose build them;
* the preconditioned MINRES recurrence in float64 in the device's order (alfa = v.(K v) - (beta / oldb) v.r1), with the device's
  stopping rule phi_k <= tol phi_0, its freeze after the last update and the mean projection of the pressure right-hand side;
* the block-diagonal preconditioner diag(F, .., F, scale M_p^-1) from 1D matrices formed on the host.
"""
import numpy as np
import scipy.linalg
import scipy.sparse

EPS = 2.220446049250313e-16


# ---------------------------------------------------------------------------------------------
# layouts
def transposed_tables(jlo, jhi, ncols):
    """(ilo, ihi, rpt) of one axis: the rows [ilo[j], ihi[j]) that hold column j, from the column ranges [jlo[i], jhi[i]) of the
    rows; supports are monotone along an axis, so they are a range (asserted)."""
    jlo, jhi = np.asarray(jlo, dtype=np.int64), np.asarray(jhi, dtype=np.int64)
    ilo, ihi = np.zeros(ncols, dtype=np.int64), np.zeros(ncols, dtype=np.int64)
    for j in range(ncols):
        rows = np.nonzero((jlo <= j) & (j < jhi))[0]
        if rows.size:
            assert rows[-1] - rows[0] + 1 == rows.size
            ilo[j], ihi[j] = rows[0], rows[-1] + 1
    return ilo, ihi, np.concatenate(([0], np.cumsum(ihi - ilo)))


def _rowptr(rp, S, c, i):
    """igx_rowptr3 for any dimension: sum_k (prod_{m<k} c_m) rp_k[i_k] (prod_{m>k} S_m)."""
    out, lead = 0, 1
    for k in range(len(rp)):
        out += lead * int(rp[k][i[k]]) * int(np.prod(S[k + 1:], dtype=np.int64))
        lead *= int(c[k])
    return out


def box_layout(lo, hi, ncols):
    """Canonical CSR ``(indptr, indices)`` of the product pattern: row (i_0, ..) holds the columns prod_k [lo_k[i_k], hi_k[i_k]),
    ravelled by `ncols`, in lexicographic order."""
    nrows = [len(l) for l in lo]
    indptr, indices = [0], []
    for i in np.ndindex(*nrows):
        axes = [np.arange(lo[k][i[k]], hi[k][i[k]]) for k in range(len(lo))]
        cols = np.ravel_multi_index(np.meshgrid(*axes, indexing='ij'), ncols).ravel() if all(a.size for a in axes) else np.zeros(0, int)
        indices.append(cols)
        indptr.append(indptr[-1] + cols.size)
    return np.array(indptr, dtype=np.int64), np.concatenate(indices).astype(np.int64)


def transposed_layout(jlo, jhi, ntrial):
    """Of the pair matrix B with the per-axis column ranges jlo / jhi (rows: test dofs, columns: `ntrial` trial dofs per axis):
    ``(indptr, indices, perm)`` -- the layout of B^T in the pair layout of the swapped spaces, and for every entry of B^T the
    position of its value in the data of B (found from rp and jlo as k_pair_transpose finds it)."""
    d = len(jlo)
    ntest = [len(l) for l in jlo]
    tabs = [transposed_tables(jlo[k], jhi[k], ntrial[k]) for k in range(d)]
    ilo, ihi = [t[0] for t in tabs], [t[1] for t in tabs]
    indptr, indices = box_layout(ilo, ihi, ntest)
    rp = [np.concatenate(([0], np.cumsum(np.asarray(jhi[k]) - np.asarray(jlo[k])))) for k in range(d)]
    S = [int(r[-1]) for r in rp]
    perm = np.empty(indices.size, dtype=np.int64)
    e = 0
    for j in np.ndindex(*ntrial):
        J = int(np.ravel_multi_index(j, ntrial))
        for I in indices[indptr[J]:indptr[J + 1]]:
            i = np.unravel_index(int(I), ntest)
            c = [int(jhi[k][i[k]] - jlo[k][i[k]]) for k in range(d)]
            off = 0
            for k in range(d):
                off = off * c[k] + (j[k] - int(jlo[k][i[k]]))
            perm[e] = _rowptr(rp, S, c, i) + off
            e += 1
    return indptr, indices, perm


# ---------------------------------------------------------------------------------------------
# the preconditioner
def _dense(M):
    return M.toarray() if scipy.sparse.issparse(M) else np.asarray(M, dtype=np.float64)


def kron_inverse(mats, lo, hi, stiff):
    """apply(x): the fast-diagonalization inverse on the box lo[k] <= i_k < hi[k]; mats[k] = (K_k, M_k) 1D matrices.  `stiff`:
    the inverse of sum_k M_0 (x) .. K_k .. (x) M_{d-1}, else of (x) M_k."""
    U, lam = [], []
    for (K, M), a, b in zip(mats, lo, hi):
        M = _dense(M)[a:b, a:b]
        w, V = scipy.linalg.eigh(_dense(K)[a:b, a:b], M) if stiff else scipy.linalg.eigh(M)
        U.append(V)
        lam.append(w)
    d = len(U)
    shape = tuple(len(l) for l in lam)
    if stiff:
        D = sum(np.reshape(lam[k], [-1 if m == k else 1 for m in range(d)]) for k in range(d)) + np.zeros(shape)
    else:
        D = np.ones(shape)
        for k in range(d):
            D = D * np.reshape(lam[k], [-1 if m == k else 1 for m in range(d)])

    def contract(T, mats_):
        for k in range(d):
            T = np.moveaxis(np.tensordot(mats_[k], T, axes=(1, k)), 0, k)
        return T

    def apply(x):
        T = contract(np.asarray(x).reshape(shape), [u.T for u in U]) / D
        return contract(T, U).ravel()
    return apply


def block_preconditioner(ndofs_u, ndofs_p, nc, free, mats_u, mats_p, scale=1.0, viscosity=1.0):
    """apply(r) of diag(F, .., F, scale M_p^-1) for masked r: F the fast diagonalization of `viscosity` times the parametric
    Laplacian on the free box of every velocity component (all of the boundary fixed), the pressure part on the whole pressure
    space, applied to the masked vector and masked again."""
    Nu, Np = int(np.prod(ndofs_u)), int(np.prod(ndofs_p))
    lo_u, hi_u = [1] * len(ndofs_u), [n - 1 for n in ndofs_u]
    F = kron_inverse(mats_u, lo_u, hi_u, True)
    S = kron_inverse(mats_p, [0] * len(ndofs_p), list(ndofs_p), False)
    box = tuple(slice(a, b) for a, b in zip(lo_u, hi_u))
    fp = free[nc * Nu:]

    def apply(r):
        z = np.zeros_like(r)
        for c in range(nc):
            zc = np.zeros(ndofs_u)
            zc[box] = (F(r[c * Nu:(c + 1) * Nu].reshape(ndofs_u)[box]) / viscosity).reshape(zc[box].shape)
            z[c * Nu:(c + 1) * Nu] = zc.ravel()
        z[nc * Nu:] = np.where(fp, scale * S(np.where(fp, r[nc * Nu:], 0.0)), 0.0)
        return z
    return apply


# ---------------------------------------------------------------------------------------------
# MINRES in the device's order
def minres(K, P, r0, tol, maxiter, x0=None):
    """Preconditioned MINRES on K x = r0 (K: callable, symmetric; P: callable, symmetric positive definite) as
    solve_minres / k_fin_minres run it.  Returns (x, iterations, converged, breakdown, phi history)."""
    n = r0.size
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64)
    r1 = np.array(r0, dtype=np.float64)
    r2 = r1.copy()
    y = P(r1)
    a = float(r1 @ y)
    if not np.isfinite(a):
        return x, 0, False, 'nonfinite', []
    if a < 0:
        return x, 0, False, 'indefinite_precond', []
    beta1 = beta = phibar = np.sqrt(a)
    stop = tol * beta1
    hist = [phibar]
    if beta1 == 0.0:
        return x, 0, True, None, hist
    oldb = dbar = epsln = 0.0
    cs, sn = -1.0, 0.0
    w1, w2 = np.zeros(n), np.zeros(n)
    v = y / beta
    vr = 0.0
    it = 0
    while it < maxiter:
        y = K(v)
        vKv = float(v @ y)
        alfa = vKv - (beta / oldb) * vr if it >= 1 else vKv
        if not np.isfinite(alfa):
            return x, it, False, 'nonfinite', hist
        c1 = beta / oldb if it >= 1 else 0.0
        rn = (y - c1 * r1) - (alfa / beta) * r2
        r1, r2 = r2, rn
        y = P(r2)
        a = float(r2 @ y)
        if not np.isfinite(a):
            return x, it, False, 'nonfinite', hist
        if a < 0:
            return x, it, False, 'indefinite_precond', hist
        oldb, beta = beta, np.sqrt(a)
        oldeps = epsln
        delta = cs * dbar + sn * alfa
        gbar = sn * dbar - cs * alfa
        epsln = sn * beta
        dbar = -cs * beta
        gamma = max(np.sqrt(gbar * gbar + beta * beta), EPS)
        cs, sn = gbar / gamma, beta / gamma
        phi, phibar = cs * phibar, sn * phibar
        if not (np.isfinite(phi) and np.isfinite(phibar)):
            return x, it, False, 'nonfinite', hist
        it += 1
        hist.append(abs(phibar))
        wn = ((v - oldeps * w1) - delta * w2) * (1.0 / gamma)
        w1, w2 = w2, wn
        x = x + phi * wn
        if abs(phibar) <= stop or beta == 0.0:
            return x, it, abs(phibar) <= stop, None, hist
        v = y * (1.0 / beta)
        vr = float(v @ r1)
    return x, it, False, None, hist


def solve(A, B, nc, bcs, b=None, P=None, tol=1e-8, maxiter=1000, project=False):
    """The saddle solve of the device on host matrices: A (nc Nu x nc Nu), B (Np x nc Nu), bcs = (indices, values) in the
    nc Nu + Np numbering.  Returns (u, info) with u the full vector (Dirichlet values included), info = dict(iterations,
    converged, breakdown, relres, rhs_mean, rhs_norm)."""
    K = scipy.sparse.bmat([[A, B.T], [B, None]], format='csr')
    n = K.shape[0]
    nv = A.shape[0]
    free = np.ones(n, dtype=bool)
    free[np.asarray(bcs[0], dtype=np.int64)] = False
    g = np.zeros(n)
    g[np.asarray(bcs[0], dtype=np.int64)] = bcs[1]
    b = np.zeros(n) if b is None else np.asarray(b, dtype=np.float64)

    def proj(r):
        if project:
            r = r.copy()
            r[nv:] -= np.where(free[nv:], r[nv:].sum() / (n - nv), 0.0)
        return r
    r_raw = np.where(free, b - K @ g, 0.0)
    mean, norm = r_raw[nv:].sum() / (n - nv), np.linalg.norm(r_raw[nv:])
    r0 = proj(r_raw)
    Kop = lambda x: np.where(free, K @ x, 0.0)
    Pop = (lambda r: r.copy()) if P is None else P
    x, it, conv, brk, hist = minres(Kop, Pop, r0, tol, maxiter)
    res = proj(np.where(free, b - K @ (g + x), 0.0))
    info = dict(iterations=it, converged=conv, breakdown=brk, relres=float(np.linalg.norm(res) / np.linalg.norm(r0)),
                rhs_mean=float(mean), rhs_norm=float(norm), phi=hist)
    return x + g, info


def normalise_pressure(u, nv, how):
    """The pressure part of u shifted: 'first' -- its first coefficient 0 (the notebook's pinned dof); 'mean' -- zero mean."""
    u = u.copy()
    u[nv:] -= u[nv] if how == 'first' else u[nv:].mean()
    return u

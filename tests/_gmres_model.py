"""Host model of the device GMRES on saddle-point systems (csrc/solve_gmres.hip): plain NumPy / SciPy, no GPU, no library load.

* right-preconditioned restarted GMRES in float64 in the device's order: z = P v_j, w = K z, classical Gram-Schmidt twice (the
  coefficients of both passes added), the stored Givens rotations applied to the new column, the stop |g_{j+1}| <= tol ||r_0||,
  the lucky breakdown h_{j+1,j} = 0, the back substitution and x += P (V y) at the end of a cycle, the residual formed again with
  a product at a restart, and the freeze after the stop;
* the block upper-triangular preconditioner [[F, B^T], [0, -S]]^-1 built from the block-diagonal one of _saddle_model.py (whose
  pieces are imported, not copied) and the masked B^T.
The mean projection of the pressure right-hand side is sm.solve's, restated in `solve` below because it is local to that function.
"""
import numpy as np
import scipy.sparse

from _saddle_model import block_preconditioner, kron_inverse, normalise_pressure  # noqa: F401  (re-exported for the cases)


def triangular_preconditioner(P, B, free, nv):
    """apply(r) of the solve with [[F, B^T], [0, -S]] from the block-diagonal apply P = diag(F^-1, S^-1) (masked r in, masked z
    out): z_p = -S^-1 r_p, z_u = F^-1 (r_u - R B^T z_p)."""
    BT = scipy.sparse.csr_matrix(B).T.tocsr()
    fu = free[:nv]

    def apply(r):
        rp = np.zeros_like(r)
        rp[nv:] = r[nv:]
        zp = -P(rp)[nv:]
        t = np.zeros_like(r)
        t[:nv] = np.where(fu, r[:nv] - BT @ zp, 0.0)
        z = P(t)
        z[nv:] = zp
        return z
    return apply


def gmres(K, P, rhs, tol, maxiter, restart, x0=None):
    """Right-preconditioned GMRES(restart) on K x = rhs (K, P: callables) as solve_gmres / k_gm_fin run it.  Returns
    (x, iterations, restarts, converged, breakdown, history of |g|)."""
    n = rhs.size
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64)
    r = np.array(rhs, dtype=np.float64) if x0 is None else rhs - K(x)
    beta = float(np.sqrt(r @ r))
    if not np.isfinite(beta):
        return x, 0, 0, False, 'nonfinite', []
    stop = tol * beta
    hist = [beta]
    if beta == 0.0:
        return x, 0, 0, True, None, hist
    it = restarts = 0
    conv = False
    while True:
        V = [r * (1.0 / beta)]
        g = [beta]
        cs, sn, R = [], [], []
        last = False
        j = 0
        while j < restart and it < maxiter:
            w = K(P(V[j]))
            h = np.zeros(j + 1)
            for _ in range(2):
                hp = np.array([float(v @ w) for v in V])
                for k in range(j + 1):
                    w = w - hp[k] * V[k]
                h += hp
            nn = float(w @ w)
            hn = np.sqrt(nn)
            if not (np.isfinite(nn) and np.isfinite(h).all()):
                return x, it, restarts, False, 'nonfinite', hist
            for i in range(j):
                t = cs[i] * h[i] + sn[i] * h[i + 1]
                h[i + 1] = cs[i] * h[i + 1] - sn[i] * h[i]
                h[i] = t
            rr = np.sqrt(h[j] * h[j] + hn * hn)
            if rr == 0.0:
                last = True
                break
            c, s = h[j] / rr, hn / rr
            gn, gj = -s * g[j], c * g[j]
            if not (np.isfinite(gn) and np.isfinite(gj) and np.isfinite(rr)):
                return x, it, restarts, False, 'nonfinite', hist
            cs.append(c)
            sn.append(s)
            h[j] = rr
            R.append(h.copy())
            g[j] = gj
            g.append(gn)
            it += 1
            j += 1
            hist.append(abs(gn))
            if abs(gn) <= stop or hn == 0.0:
                last = conv = True
                break
            V.append(w * (1.0 / hn))
        y = np.zeros(j)
        for i in range(j - 1, -1, -1):
            t = g[i]
            for k in range(i + 1, j):
                t -= R[k][i] * y[k]
            y[i] = t / R[i][i]
        if not np.isfinite(y).all():
            return x, it, restarts, False, 'nonfinite', hist
        t = np.zeros(n)
        for k in range(j):
            t = t + y[k] * V[k]
        x = x + P(t)
        if last or it >= maxiter:
            break
        restarts += 1
        r = rhs - K(x)
        beta = float(np.sqrt(r @ r))
        if not np.isfinite(beta):
            return x, it, restarts, False, 'nonfinite', hist
        if beta <= stop:
            conv = True
            break
    return x, it, restarts, conv, None, hist


def solve(A, B, nc, bcs, b=None, P=None, tol=1e-8, maxiter=1000, restart=40, project=False, triangular=False):
    """The device's GMRES solve on host matrices: A (nc Nu x nc Nu, need not be symmetric), B (Np x nc Nu), bcs = (indices,
    values) in the nc Nu + Np numbering, P the block-diagonal preconditioner (masked r -> masked z) or None; `triangular`: its
    block upper-triangular form.  Returns (u, info) as _saddle_model.solve, with `restarts`."""
    K = scipy.sparse.bmat([[A, scipy.sparse.csr_matrix(B).T], [B, None]], format='csr')
    n, nv = K.shape[0], A.shape[0]
    idx = np.asarray(bcs[0], dtype=np.int64)
    free = np.ones(n, dtype=bool)
    free[idx] = False
    g = np.zeros(n)
    g[idx] = bcs[1]
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
    Pop = (lambda r: r.copy()) if P is None else (triangular_preconditioner(P, B, free, nv) if triangular else P)
    x, it, restarts, conv, brk, hist = gmres(Kop, Pop, r0, tol, maxiter, restart)
    res = proj(np.where(free, b - K @ (g + x), 0.0))
    info = dict(iterations=it, restarts=restarts, converged=conv, breakdown=brk,
                relres=float(np.linalg.norm(res) / np.linalg.norm(r0)), rhs_mean=float(mean), rhs_norm=float(norm), g=hist)
    return x + g, info

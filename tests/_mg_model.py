"""Numpy model of the multigrid preconditioner of MultipatchSystem, shared by the CPU and GPU tests:
the first-fit colouring restated in Python, Gauss-Seidel sweeps in colour order, the global prolongation
W^-1 sum_p X_pf (P_0 (x) P_1 [(x) P_2]) X_pc^T, the V-cycle with a dense inverse on the coarsest level, and PCG.  Needs no device:
the matrices of the levels are handed in."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from pyiga_amd import bspline, solvers


def first_fit(indptr, indices, free=None):
    """Colour of every row (-1 where not free): rows in ascending order take the smallest colour none of their coloured
    neighbours has.  The Python restatement of igx_csr_colouring."""
    n = len(indptr) - 1
    colour = -np.ones(n, dtype=np.int64)
    for i in range(n):
        if free is not None and not free[i]:
            continue
        nb = indices[indptr[i]:indptr[i + 1]]
        used = set(colour[nb[nb != i]].tolist())
        c = 0
        while c in used:
            c += 1
        colour[i] = c
    return colour


def colour_order(colour):
    """The free dofs sorted by (colour, index)."""
    fr = np.flatnonzero(colour >= 0)
    return fr[np.argsort(colour[fr], kind='stable')]


def coarsen(MP):
    """The multipatch of MP's patches over coarsened knot vectors, joined as MP."""
    return MP.replay_joins([(tuple(solvers.coarsen_knots(kv) for kv in kvs), geo) for kvs, geo in MP.patches])


def patch_prolongation(kvs_c, kvs_f):
    P = None
    for kc, kf in zip(kvs_c, kvs_f):
        P1 = bspline.prolongation(kc, kf)
        P = P1 if P is None else sp.kron(P, P1, format='csr')
    return sp.csr_matrix(P)


def global_prolongation(MPf, MPc):
    """(W^-1 sum_p X_pf P_p X_pc^T, the patch terms X_pf P_p X_pc^T, the multiplicities W) on all dofs."""
    terms, mult = [], np.zeros(MPf.numdofs)
    for p in range(MPf.numpatches):
        Xf, Xc = MPf.patch_to_global(p), MPc.patch_to_global(p)
        terms.append(sp.csr_matrix(Xf @ patch_prolongation(MPc.patches[p][0], MPf.patches[p][0]) @ Xc.T))
        mult += np.asarray(Xf.sum(axis=1)).ravel()
    return sp.csr_matrix(sp.diags(1.0 / mult) @ sum(terms)), terms, mult


def side_dofs(MP, sides):
    """Global dofs of the patch sides [(patch, axis, side), ...]."""
    from pyiga_amd.multipatch import slice_indices
    out = [MP.patch_to_global_idx(p)[slice_indices(ax, 0 if sd == 0 else -1, tuple(kv.numdofs for kv in MP.patches[p][0]), ravel=True)]
           for p, ax, sd in sides]
    return np.unique(np.concatenate(out)) if out else np.zeros(0, dtype=np.int64)


def gauss_seidel(A, x, b, order, sweep='forward'):
    """Sequential Gauss-Seidel over the rows `order` (backward: reversed; symmetric: both), in place on a copy."""
    A = sp.csr_matrix(A)
    x = np.array(x, dtype=float)
    ip, ix, d = A.indptr, A.indices, A.data
    diag = A.diagonal()
    seqs = {'forward': [order], 'backward': [order[::-1]], 'symmetric': [order, order[::-1]]}[sweep]
    for seq in seqs:
        for i in seq:
            if diag[i] == 0:
                continue
            s = d[ip[i]:ip[i + 1]] @ x[ix[ip[i]:ip[i + 1]]] - diag[i] * x[i]
            x[i] = (b[i] - s) / diag[i]
    return x


class Model:
    """The V-cycle on the matrices `As` (all dofs of every level, the finest first), the multipatches `MPs` and the fixed dofs
    `fixed` of every level.  Vectors are over the free dofs of the finest level in ascending order."""

    def __init__(self, As, MPs, fixed, smooth_steps=1, colours=None):
        self.nu = smooth_steps
        self.levels = []
        for l, (A, MP, fx) in enumerate(zip(As, MPs, fixed)):
            A = sp.csr_matrix(A)
            A.sort_indices()
            free = np.ones(MP.numdofs, dtype=bool)
            free[np.asarray(fx, dtype=np.int64)] = False
            fr = np.flatnonzero(free)
            col = first_fit(A.indptr, A.indices, free) if colours is None else colours[l]
            order = colour_order(col)
            pos = np.empty(MP.numdofs, dtype=np.int64)
            pos[fr] = np.arange(fr.size)
            Af = A[fr][:, fr].tocsr()
            perm = pos[order]                            # the colour order within the free vector
            Ap = Af[perm][:, perm].tocsr()
            self.levels.append(dict(A=A, Af=Af, fr=fr, perm=perm, inv=np.argsort(perm), colour=col, ncol=int(col.max()) + 1 if fr.size else 0,
                                    DL=sp.tril(Ap, format='csr'), DU=sp.triu(Ap, format='csr'), Ap=Ap, MP=MP))
        for a, b in zip(self.levels[:-1], self.levels[1:]):
            Pfull, _, _ = global_prolongation(a['MP'], b['MP'])
            a['Pfull'] = Pfull
            a['P'] = Pfull[a['fr']][:, b['fr']].tocsr()
        last = self.levels[-1]
        inv = np.linalg.inv(last['Af'].toarray()) if last['fr'].size else np.zeros((0, 0))
        last['Ainv'] = 0.5 * (inv + inv.T)

    def _smooth(self, L, x, b, lower):
        p = L['perm']
        xp, bp = x[p], b[p]
        xp = xp + spla.spsolve_triangular(L['DL'] if lower else L['DU'], bp - L['Ap'] @ xp, lower=lower)
        out = np.empty_like(x)
        out[p] = xp
        return out

    def vcycle(self, b, l=0):
        L = self.levels[l]
        if l == len(self.levels) - 1:
            return L['Ainv'] @ b
        x = np.zeros_like(b)
        for _ in range(self.nu):
            x = self._smooth(L, x, b, True)
        x = x + L['P'] @ self.vcycle(L['P'].T @ (b - L['Af'] @ x), l + 1)
        for _ in range(self.nu):
            x = self._smooth(L, x, b, False)
        return x

    def apply_full(self, r):
        """The V-cycle on a vector of all dofs of the finest level (fixed entries ignored / 0)."""
        L = self.levels[0]
        z = np.zeros(L['MP'].numdofs)
        z[L['fr']] = self.vcycle(np.asarray(r, dtype=float)[L['fr']])
        return z


def pcg(A, b, M, tol=1e-8, maxiter=5000):
    """(x, iterations) of preconditioned CG from x0 = 0 to ||r|| <= tol ||b||."""
    x = np.zeros_like(b)
    r = b.copy()
    z = M(r)
    p = z.copy()
    rz = r @ z
    b0 = np.linalg.norm(b)
    for it in range(1, maxiter + 1):
        q = A @ p
        a = rz / (p @ q)
        x += a * p
        r -= a * q
        if np.linalg.norm(r) <= tol * b0:
            return x, it
        z = M(r)
        rz2 = r @ z
        p = z + (rz2 / rz) * p
        rz = rz2
    return x, maxiter


def oracle_levels(orc, make, geos, p, n, nlev, sides):
    """(As, MPs, fixed) of `nlev` levels of the hand-joined domain make(p=, n=) with the oracle's stiffness matrices per patch
    (`geos`: the oracle's geometry of every patch), summed through MP.patch_to_global; `sides`: [(patch, bdspec), ...] fixed."""
    import _mpsolve_model as M
    As, MPs, fixed = [], [], []
    for k in range(nlev):
        MP = make(p=p, n=n >> k)
        okv = orc.make_knots(p, 0.0, 1.0, n >> k)
        A = None
        for q in range(MP.numpatches):
            X = MP.patch_to_global(q)
            T = X @ orc.assemble('stiffness', (okv, okv), geos[q]) @ X.T
            A = T if A is None else A + T
        As.append(sp.csr_matrix(A))
        MPs.append(MP)
        fixed.append(M.fixed_dofs(MP, sides))
    return As, MPs, fixed

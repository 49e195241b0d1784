"""Host model of the local multigrid (tests/test_hmg_cpu.py, tests/test_hmg_gpu.py, tests/test_hmg_kernels_gpu.py): a numpy
restatement of the reference's cycle (pyiga/solvers.py:174-283) with the sweep order as a parameter, a long-double triple
product, and a Python first-fit colouring.  Nothing here touches the device or the library.
"""
import numpy as np
import scipy.linalg
import scipy.sparse

LD = np.longdouble


def csr(A):
    A = scipy.sparse.csr_matrix(A)
    A.sort_indices()
    return A


def structural_pattern(A, P):
    """0/1 CSR of the structural pattern of P^T A P (stored entries of A and P; nothing lost to cancellation)."""
    A, P = csr(A), csr(P)
    one = lambda M: scipy.sparse.csr_matrix((np.ones(M.nnz, dtype=np.int64), M.indices, M.indptr), shape=M.shape)   # noqa: E731
    C = csr(one(P).T @ one(A) @ one(P))
    C.data[:] = 1
    return C


def rap_longdouble(A, P, pattern=None):
    """P^T A P summed in long double, entry by entry of the structural pattern (or `pattern`), rounded once to double.  Returns
    CSR on that pattern: positions without a term hold an explicit 0.0."""
    A, P = csr(A), csr(P)
    pat = structural_pattern(A, P) if pattern is None else csr(pattern)
    PT = csr(P.T)
    nc = P.shape[1]
    # rows of P^T A as dicts of long doubles, then their products with the columns of P
    vals = np.zeros(pat.nnz)
    Pcols = [dict(zip(PT.indices[PT.indptr[j]:PT.indptr[j + 1]].tolist(), PT.data[PT.indptr[j]:PT.indptr[j + 1]].astype(LD))) for j in range(nc)]
    for i in range(nc):
        row = {}
        for a in range(PT.indptr[i], PT.indptr[i + 1]):
            k, w = PT.indices[a], LD(PT.data[a])
            for q in range(A.indptr[k], A.indptr[k + 1]):
                m = A.indices[q]
                row[m] = row.get(m, LD(0)) + w * LD(A.data[q])
        for e in range(pat.indptr[i], pat.indptr[i + 1]):
            col = Pcols[pat.indices[e]]
            small, big = (col, row) if len(col) < len(row) else (row, col)
            s = LD(0)
            for m in sorted(small):
                if m in big:
                    s += small[m] * big[m]
            vals[e] = float(s)
    return scipy.sparse.csr_matrix((vals, pat.indices, pat.indptr), shape=(nc, nc))


def spmv_longdouble(M, x, y=None):
    M = csr(M)
    out = np.zeros(M.shape[0], dtype=LD) if y is None else np.asarray(y, dtype=LD).copy()
    xl = np.asarray(x, dtype=LD)
    for i in range(M.shape[0]):
        s = LD(0)
        for k in range(M.indptr[i], M.indptr[i + 1]):
            s += LD(M.data[k]) * xl[M.indices[k]]
        out[i] += s
    return out.astype(np.float64)


def galerkin_chain(A, Ps, exact=True):
    """The level matrices, coarsest first: A_{l-1} = P_l^T A_l P_l (long double per entry, or scipy's double product)."""
    As = [csr(A)]
    for P in reversed(Ps):
        As.append(rap_longdouble(As[-1], P) if exact else csr(P.T @ As[-1] @ P))
    As.reverse()
    return As


def first_fit(A, ind):
    """First-fit colouring in ascending index order over the pattern of `A` restricted to the set `ind`: ``(colour, ncolours)``,
    colour -1 outside the set."""
    A = csr(A)
    colour = np.full(A.shape[0], -1, dtype=np.int64)
    members = np.zeros(A.shape[0], dtype=bool)
    members[np.asarray(ind, dtype=np.int64)] = True
    nc = 0
    for i in np.flatnonzero(members):
        used = {colour[j] for j in A.indices[A.indptr[i]:A.indptr[i + 1]] if j != i and colour[j] >= 0}
        c = 0
        while c in used:
            c += 1
        colour[i] = c
        nc = max(nc, c + 1)
    return colour, nc


def colour_order(A, ind):
    """The set `ind` sorted by (colour, index), and the number of colours."""
    colour, nc = first_fit(A, ind)
    rows = np.flatnonzero(colour >= 0)
    return rows[np.argsort(colour[rows], kind='stable')], nc


def gauss_seidel(A, x, b, order):
    """One sweep over the rows `order`, in that order, in place (pyiga/relaxation_cy.pyx: gauss_seidel_indexed)."""
    ip, ix, v = A.indptr, A.indices, A.data
    for i in order:
        seg = slice(ip[i], ip[i + 1])
        cols, vals = ix[seg], v[seg]
        off = cols != i
        x[i] = (b[i] - vals[off] @ x[cols[off]]) / vals[~off][0]


class Model:
    """The cycle on the level matrices `As` (coarsest first) with the prolongations `Ps` and, per level, the rows the smoother
    visits in the order it visits them (`orders`; level 0: the dofs of the direct solve)."""

    def __init__(self, As, Ps, orders, smoother='gs', smooth_steps=2):
        assert smoother in ('gs', 'forward_gs', 'backward_gs', 'symmetric_gs')
        self.As, self.Ps = [csr(A) for A in As], [csr(P) for P in Ps]
        self.orders = [np.asarray(o, dtype=np.int64) for o in orders]
        self.smoother, self.steps = smoother, smooth_steps
        i0 = self.orders[0]
        self.inv0 = scipy.linalg.inv(self.As[0][i0][:, i0].toarray()) if i0.size else np.zeros((0, 0))

    def _smooth(self, lv, x, f, post):
        A, o = self.As[lv], self.orders[lv]
        for _ in range(self.steps):
            if self.smoother == 'symmetric_gs':
                gauss_seidel(A, x, f, o)
                gauss_seidel(A, x, f, o[::-1])
            else:
                back = self.smoother == 'backward_gs' or (self.smoother == 'gs' and post)
                gauss_seidel(A, x, f, o[::-1] if back else o)

    def step(self, lv, x, f):
        x1 = np.array(x, dtype=np.float64)
        if lv == 0:
            i0 = self.orders[0]
            x1[i0] = self.inv0 @ f[i0]
            return x1
        P, A = self.Ps[lv - 1], self.As[lv]
        self._smooth(lv, x1, f, False)
        rc = P.T @ (f - A @ x1)
        x1 += P @ self.step(lv - 1, np.zeros_like(rc), rc)
        self._smooth(lv, x1, f, True)
        return x1

    def cycle(self, f, x=None):
        f = np.asarray(f, dtype=np.float64)
        return self.step(len(self.As) - 1, np.zeros_like(f) if x is None else x, f)

    def iterate(self, f, free, tol, maxiter=500):
        """``(iterates, ratios)`` of x <- cycle(x) from zero until the residual over `free` has dropped by `tol`."""
        A = self.As[-1]
        free = np.asarray(free, dtype=np.int64)
        res0 = np.linalg.norm(f[free])
        x = np.zeros_like(f)
        xs, ratios = [], []
        while len(ratios) < maxiter:
            x = self.cycle(f, x)
            xs.append(x)
            ratios.append(np.linalg.norm((f - A @ x)[free]) / res0)
            if ratios[-1] < tol:
                break
        return xs, ratios

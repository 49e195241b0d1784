"""The operations of ``solvers.lobpcg_loop`` on numpy arrays: the host model of the device eigen-solver.

A plain helper module (no GPU needed): tests/test_eig_cpu.py runs the controller on it with the oracle's matrices,
tests/test_eig_gpu.py compares the device solve with it.  Blocks are full-length ``(n, m)`` arrays that vanish on the fixed
dofs, as on the device; K and M are scipy CSR matrices of all dofs.
"""
import numpy as np
import scipy.linalg
import scipy.sparse


class NumpyOps:
    def __init__(self, K, M, fixed, X0, precond=None):
        self.K, self.M = scipy.sparse.csr_matrix(K), scipy.sparse.csr_matrix(M)
        self.n = self.K.shape[0]
        self.free = np.ones(self.n, dtype=bool)
        self.free[np.asarray(fixed, dtype=np.int64)] = False
        self.X0 = np.array(X0, dtype=np.float64)
        self.precond_fn = precond                     # (n, m) -> (n, m) on masked blocks, or None
        self.b = {}

    def _mask(self, A):
        return np.where(self.free[:, None], A, 0.0)

    def start(self):
        self.b = {'X': self._mask(self.X0)}

    def products(self, name):
        self.b['K' + name] = self._mask(self.K @ self.b[name])
        self.b['M' + name] = self._mask(self.M @ self.b[name])

    def gram(self, A, B):
        return np.hstack([self.b[a] for a in A]).T @ np.hstack([self.b[c] for c in B])

    def combine(self, updates, triple):
        new = {}
        for dst, srcs, coeffs in updates:
            for pre in (('', 'K', 'M') if triple else ('',)):
                new[pre + dst] = sum(self.b[pre + s] @ np.asarray(c) for s, c in zip(srcs, coeffs))
        self.b.update(new)

    def residuals(self, lam):
        R = self._mask(self.b['KX'] - self.b['MX'] * np.asarray(lam)[None, :])
        self.b['R'] = R
        return np.sqrt((R * R).sum(axis=0)), np.sqrt((self.b['KX'] ** 2).sum(axis=0))

    def precond(self, src, dst):
        r = self.b[src]
        self.b[dst] = self._mask(r if self.precond_fn is None else self.precond_fn(r))


def kron_precond(U, lam, box, ndofs):
    """The fast-diagonalization inverse of the parametric Laplacian on the free box ``box = (lo, hi)`` of the tensor index space
    `ndofs`, from the per-axis factors of ``solvers.fastdiag_factors``: a function of full-length blocks."""
    lo, hi = box
    d = len(ndofs)
    sl = tuple(slice(a, b) for a, b in zip(lo, hi))
    D = lam[0]
    for l in lam[1:]:
        D = np.add.outer(D, l)

    def apply(R):
        m = R.shape[1]
        T = R.reshape(tuple(ndofs) + (m,))[sl]
        for k in range(d):
            T = np.moveaxis(np.tensordot(U[k].T, T, axes=(1, k)), 0, k)
        T = T / D[..., None]
        for k in range(d):
            T = np.moveaxis(np.tensordot(U[k], T, axes=(1, k)), 0, k)
        Z = np.zeros(tuple(ndofs) + (m,))
        Z[sl] = T
        return Z.reshape(-1, m)
    return apply


def dense_eigh(K, M, fixed):
    """``(lam, V, free)``: every eigenpair of the restricted pencil by dense ``eigh`` (V M-orthonormal, free dofs only)."""
    n = K.shape[0]
    free = np.setdiff1d(np.arange(n), np.asarray(fixed, dtype=np.int64))
    Kf = scipy.sparse.csr_matrix(K)[free][:, free].toarray()
    Mf = scipy.sparse.csr_matrix(M)[free][:, free].toarray()
    lam, V = scipy.linalg.eigh(Kf, Mf)
    return lam, V, free


def boundary_dofs(ndofs):
    """The dofs on every side of the tensor index space `ndofs` (sorted)."""
    idx = np.arange(int(np.prod(ndofs))).reshape(ndofs)
    on = np.zeros(ndofs, dtype=bool)
    for k, n in enumerate(ndofs):
        s = [slice(None)] * len(ndofs)
        for e in (0, n - 1):
            s[k] = e
            on[tuple(s)] = True
    return np.sort(idx[on])


def start_block(n, m, seed):
    return np.random.default_rng(seed).standard_normal((n, m))

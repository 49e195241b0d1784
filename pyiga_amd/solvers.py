"""Solvers (names and contracts of ``pyiga.solvers``, pyiga/solvers.py:17-42) and the device-resident Dirichlet problem of one
patch.

``fastdiag_solver(KM)``: the fast diagonalization solver of Sangalli and Tani.  The generalized eigenproblems of the small 1D
pairs ``(K_k, M_k)`` are solved on the host (setup); the application ``(x)U_k . D^-1 . (x)U_k^T`` runs on the device.

``PatchSystem(kvs, geo, rhs, bcs, kind)``: assembles the mass or stiffness matrix of a patch on the device and solves the
Dirichlet problem there by preconditioned CG (``igx_solver_*``, pyiga_amd/csrc/solve.hip).  The matrix never leaves the
device; only the solution vector comes back.  What the reference does with ``RestrictedLinearSystem`` and ``make_solver`` /
``cg`` on a host matrix.
"""
import ctypes as C

import numpy as np
import scipy.linalg
import scipy.sparse
import scipy.sparse.linalg

from . import _lib
from . import assemblers
from .operators import DeviceArray, DeviceKron, _dense


class KronDiagOperator(scipy.sparse.linalg.LinearOperator):
    """``(U_0 (x) .. (x) U_{d-1}) . D^-1 . (U_0 (x) ..)^T`` with D built from the per-axis eigenvalues `lam` as a sum
    (``lam_mode = IGX_KRON_SUM``) or a product (``IGX_KRON_PRODUCT``); applied on the device.  Trailing batch columns are
    supported by matmat."""

    def __init__(self, U, lam, lam_mode, device=None):
        self.U = [np.ascontiguousarray(u, dtype=np.float64) for u in U]
        self.lam = [np.ascontiguousarray(l, dtype=np.float64) for l in lam]
        self.lam_mode = lam_mode
        self.device = device
        self._dev = None
        n = int(np.prod([u.shape[0] for u in self.U]))
        scipy.sparse.linalg.LinearOperator.__init__(self, dtype=np.dtype(np.float64), shape=(n, n))

    def _ops(self):
        if self._dev is None:
            right = DeviceKron([u.T for u in self.U], lam=self.lam, lam_mode=self.lam_mode, device=self.device)
            left = DeviceKron(self.U, device=self.device)
            self._dev = (right, left)
        return self._dev

    def _matmat(self, X):
        right, left = self._ops()
        X = np.ascontiguousarray(X, dtype=np.float64)
        batch = X.shape[1]
        d_x = DeviceArray.from_host(right.ctx, X)
        d_t = DeviceArray(right.ctx, X.size)
        right.apply_d(d_x, d_t, batch)
        left.apply_d(d_t, d_x, batch)
        return d_x.download().reshape(-1, batch)

    def _matvec(self, x):
        return self._matmat(np.reshape(x, (-1, 1)))[:, 0]

    def _transpose(self):
        return self

    def _adjoint(self):
        return self


def fastdiag_solver(KM):
    """The fast diagonalization solver as described in [Sangalli, Tani 2016].

    `KM`: a sequence of length `d` (1 to 3) of pairs of symmetric matrices ``(K_i, M_i)``.  Returns a ``LinearOperator`` that
    realizes the inverse of ``sum_i M_0 (x) .. (x) K_i (x) .. (x) M_{d-1}``.  The eigenproblems are solved on the host; the
    operator is applied on the device."""
    EV = [scipy.linalg.eigh(_dense(K), _dense(M)) for (K, M) in KM]
    return KronDiagOperator([U for (_, U) in EV], [lam for (lam, _) in EV], _lib.IGX_KRON_SUM)


def dirichlet_box(ndofs, indices):
    """If the dof set `indices` is exactly a union of whole sides of the tensor-product index space `ndofs`, the box of the free
    dofs as ``(lo, hi)`` tuples (``lo[k] <= i_k < hi[k]``); else None."""
    ndofs = tuple(int(n) for n in ndofs)
    fixed = np.zeros(ndofs, dtype=bool)
    idx = np.asarray(indices, dtype=np.int64).ravel()
    if idx.size and (idx.min() < 0 or idx.max() >= fixed.size):
        return None
    fixed.ravel()[idx] = True
    lo, hi = [], []
    for k, n in enumerate(ndofs):
        first = np.take(fixed, 0, axis=k).all()
        last = np.take(fixed, n - 1, axis=k).all()
        lo.append(1 if first else 0)
        hi.append(n - 1 if last else n)
        if lo[-1] >= hi[-1]:
            return None
    box = np.ones(ndofs, dtype=bool)
    box[tuple(slice(a, b) for a, b in zip(lo, hi))] = False
    if not np.array_equal(box, fixed):
        return None
    return tuple(lo), tuple(hi)


class PatchSystem:
    """The Dirichlet problem ``A u = b`` with ``u = g`` on the dofs of `bcs`, for the mass or stiffness matrix of one patch,
    assembled and solved on the device.

    `rhs`: the load vector (any shape with ``prod(ndofs)`` entries), or a function of the physical coordinates whose load vector
    is then formed with ``assemble.inner_products``.  `bcs`: ``(indices, values)`` as ``compute_dirichlet_bcs`` returns them, or
    None.  ``solve(...)`` returns the completed full vector and leaves the solver's statistics in ``info``.
    """

    def __init__(self, kvs, geo, rhs, bcs=None, kind='stiffness', device=None):
        self.kvs = tuple(kvs)
        self.kind = kind
        if kind not in _lib.KINDS:
            raise ValueError('unknown kind %r' % (kind,))
        self.patch = assemblers.DevicePatch(self.kvs, geo, device=device)
        self.ndofs = self.patch.ndofs
        self.n = int(np.prod(self.ndofs))
        if kind in ('mass', 'stiffness'):
            self.patch.assemble(kind, to_host=False)            # the values stay on the device
        if callable(rhs):
            from . import assemble
            rhs = assemble.inner_products(self.kvs, rhs, f_physical=True, geo=geo)
        self.b = np.ascontiguousarray(rhs, dtype=np.float64).ravel()
        if self.b.size != self.n:
            raise ValueError('right-hand side has %d entries, the space %d' % (self.b.size, self.n))
        if bcs is None:
            idx, vals = np.zeros(0, dtype=np.int64), np.zeros(0)
        else:
            idx = np.asarray(bcs[0], dtype=np.int64).ravel()
            vals = np.broadcast_to(np.asarray(bcs[1], dtype=np.float64), idx.shape)
            idx, first = np.unique(idx, return_index=True)    # (a repeated dof keeps its first value, as combine_bcs)
            vals = vals[first]
        self.bc_indices, self.bc_values = idx, np.ascontiguousarray(vals)
        self.box = dirichlet_box(self.ndofs, idx)
        self._precond = None
        self.info = None
        h = C.c_void_p()
        _lib.check(_lib.load().igx_solver_create(self.patch.handle, _lib.KINDS[kind],
                                                 idx.ctypes.data_as(C.POINTER(C.c_int64)), idx.size, C.byref(h)),
                   'igx_solver_create')
        self.handle = h.value

    def close(self):
        if getattr(self, 'handle', None):
            _lib.load().igx_solver_destroy(self.handle)
            self.handle = None
        if getattr(self, 'patch', None) is not None:
            self.patch.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _kron_factors(self):
        """Per-axis eigenvectors and eigenvalues of the 1D Dirichlet matrices of the free range."""
        from .assemble import bsp_mass_1d, bsp_stiffness_1d
        lo, hi = self.box
        U, lam = [], []
        for kv, a, b in zip(self.kvs, lo, hi):
            M = bsp_mass_1d(kv)[a:b, a:b].toarray()
            if self.kind == 'stiffness':
                K = bsp_stiffness_1d(kv)[a:b, a:b].toarray()
                w, V = scipy.linalg.eigh(K, M)
            else:
                w, V = scipy.linalg.eigh(M)
            U.append(np.ascontiguousarray(V))
            lam.append(np.ascontiguousarray(w))
        return U, lam, (_lib.IGX_KRON_SUM if self.kind == 'stiffness' else _lib.IGX_KRON_PRODUCT)

    def set_precond(self, precond):
        key = precond if precond is not None else 'none'
        if key not in _lib.PRECONDS:
            raise ValueError('unknown preconditioner %r' % (precond,))
        if key == self._precond:
            return
        lib = _lib.load()
        if key == 'kron':
            if self.box is None:
                raise ValueError("precond='kron' needs the Dirichlet dofs to be a union of whole sides of the patch")
            U, lam, mode = self._kron_factors()
            lo = (C.c_int32 * 3)(*self.box[0])
            hi = (C.c_int32 * 3)(*self.box[1])
            Up = (_lib._dp * 3)(*[_lib.dptr(u) for u in U])
            Lp = (_lib._dp * 3)(*[_lib.dptr(l) for l in lam])
            _lib.check(lib.igx_solver_set_precond(self.handle, _lib.IGX_PRECOND_KRON, lo, hi, Up, Lp, mode), 'igx_solver_set_precond')
        else:
            _lib.check(lib.igx_solver_set_precond(self.handle, _lib.PRECONDS[key], None, None, None, None, 0), 'igx_solver_set_precond')
        self._precond = key

    def solve(self, tol=1e-8, maxiter=1000, precond='kron', x0=None, check_every=1, timed=False):
        """CG to ``||r|| <= tol * ||R (b - A ext(g))||``; returns the full solution vector (the Dirichlet values included)."""
        self.set_precond(precond)
        u = np.empty(self.n)
        x0a = None if x0 is None else np.ascontiguousarray(x0, dtype=np.float64).ravel()
        if x0a is not None and x0a.size != self.n:
            raise ValueError('x0 has the wrong size')
        info = _lib.SolveInfo()
        _lib.check(_lib.load().igx_solver_solve(self.handle, _lib.dptr(self.b), _lib.dptr(self.bc_values),
                                                None if x0a is None else _lib.dptr(x0a), float(tol), int(maxiter),
                                                int(check_every), 1 if timed else 0, _lib.dptr(u), C.byref(info)),
                   'igx_solver_solve')
        self.info = dict(info.as_dict(), converged=bool(info.converged), precond=self._precond)
        return u

    def spmv(self, x):
        """``R A R^T x`` on the device (full-length vectors in and out)."""
        x = np.ascontiguousarray(x, dtype=np.float64).ravel()
        d_x = DeviceArray.from_host(self.patch.ctx, x)
        d_y = DeviceArray(self.patch.ctx, self.n)
        _lib.check(_lib.load().igx_solver_spmv_d(self.handle, d_x.ptr, d_y.ptr), 'igx_solver_spmv_d')
        return d_y.download()

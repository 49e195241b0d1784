"""Linear operators whose application runs on the device (the part of ``pyiga.operators`` the solvers use,
pyiga/operators.py:60-86).

``KroneckerOperator(*ops)`` applies ``ops[0] (x) ops[1] [(x) ops[2]]`` with ``igx_kron_apply_d``: one contraction per axis
through LDS tiles (pyiga_amd/csrc/solve.hip).  Factors may be dense arrays or scipy sparse matrices (densified; the factors
are the small 1D matrices of a tensor-product space) and may be rectangular.  There is no host fallback.
"""
import ctypes as C

import numpy as np
import scipy.sparse
import scipy.sparse.linalg

from . import _lib


def _dense(A):
    if scipy.sparse.issparse(A):
        A = A.toarray()
    elif isinstance(A, scipy.sparse.linalg.LinearOperator):
        A = A @ np.eye(A.shape[1])
    return np.ascontiguousarray(A, dtype=np.float64)


class DeviceArray:
    """A float64 buffer in device memory (igx_dev_alloc), freed with the object."""

    def __init__(self, ctx, n):
        self.ctx, self.n = ctx, int(n)
        self.ptr = _lib.load().igx_dev_alloc(ctx.handle, max(1, self.n) * 8)
        if not self.ptr:
            raise _lib.IgxError('igx_dev_alloc failed: ' + _lib.last_error())

    @classmethod
    def from_host(cls, ctx, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        d = cls(ctx, a.size)
        d.upload(a)
        return d

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert a.size == self.n
        _lib.check(_lib.load().igx_dev_upload(self.ctx.handle, self.ptr, a.ctypes.data, a.nbytes), 'igx_dev_upload')

    def download(self):
        out = np.empty(self.n)
        _lib.check(_lib.load().igx_dev_download(self.ctx.handle, out.ctypes.data, self.ptr, out.nbytes), 'igx_dev_download')
        return out

    def free(self):
        if getattr(self, 'ptr', None) and getattr(self.ctx, 'handle', None):
            _lib.load().igx_dev_free(self.ctx.handle, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceKron:
    """Dense factors resident on the device, applied as ``y = D^-1 (B_0 (x) .. (x) B_{d-1}) x`` to tensors with a trailing
    batch axis.  `lam` / `lam_mode`: the optional diagonal D of ``igx_kron_desc``."""

    def __init__(self, factors, lam=None, lam_mode=0, device=None):
        self.factors = [_dense(B) for B in factors]
        assert 1 <= len(self.factors) <= 3, 'the device Kronecker product takes 1 to 3 factors'
        self.ctx = _lib.context(device)
        self.m = tuple(B.shape[0] for B in self.factors)
        self.n = tuple(B.shape[1] for B in self.factors)
        self._B = [DeviceArray.from_host(self.ctx, B) for B in self.factors]
        self.lam_mode = int(lam_mode)
        self._lam = [DeviceArray.from_host(self.ctx, l) for l in lam] if lam_mode else []

    def desc(self, batch):
        d = _lib.KronDesc()
        d.dim = len(self.factors)
        for k, B in enumerate(self._B):
            d.m[k], d.n[k], d.d_B[k] = self.m[k], self.n[k], B.ptr
            if self.lam_mode:
                d.d_lam[k] = self._lam[k].ptr
        d.batch = int(batch)
        for off_name, st_name, ext in (('x_off', 'x_stride', self.n), ('y_off', 'y_stride', self.m)):
            st = getattr(d, st_name)
            st[3] = 1
            s = int(batch)
            for k in reversed(range(3)):
                st[k] = s
                s *= ext[k] if k < len(ext) else 1
            setattr(d, off_name, 0)
        d.lam_mode = self.lam_mode
        return d

    def apply_d(self, d_x, d_y, batch=1):
        """Device buffers in, device buffer out (C order, batch axis last)."""
        d = self.desc(batch)
        _lib.check(_lib.load().igx_kron_apply_d(self.ctx.handle, C.byref(d), d_x.ptr, d_y.ptr, None, 0), 'igx_kron_apply_d')

    def apply(self, X):
        """X: host array (prod n, batch) -> host array (prod m, batch)."""
        X = np.ascontiguousarray(X, dtype=np.float64)
        batch = X.shape[1]
        d_x = DeviceArray.from_host(self.ctx, X)
        d_y = DeviceArray(self.ctx, int(np.prod(self.m)) * batch)
        self.apply_d(d_x, d_y, batch)
        return d_y.download().reshape(-1, batch)


class KroneckerOperator(scipy.sparse.linalg.LinearOperator):
    """A :class:`LinearOperator` that applies the Kronecker product of the given factors (1 to 3 of them) on the device."""

    def __init__(self, *ops):
        self.ops = ops
        sz = int(np.prod([A.shape[1] for A in ops]))
        sz_out = int(np.prod([A.shape[0] for A in ops]))
        self._dev = None
        scipy.sparse.linalg.LinearOperator.__init__(self, dtype=np.dtype(np.float64), shape=(sz_out, sz))

    def _kron(self):
        if self._dev is None:
            self._dev = DeviceKron(self.ops)
        return self._dev

    def _matvec(self, x):
        return self._kron().apply(np.reshape(x, (-1, 1)))[:, 0]

    def _matmat(self, X):
        return self._kron().apply(X)

    def _transpose(self):
        return KroneckerOperator(*(B.T for B in self.ops))

    def _adjoint(self):
        return KroneckerOperator(*(B.conj().T for B in self.ops))

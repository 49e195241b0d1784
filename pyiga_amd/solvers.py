"""Solvers (names and contracts of ``pyiga.solvers``, pyiga/solvers.py:17-42) and the device-resident Dirichlet problem of one
patch.

``fastdiag_solver(KM)``: the fast diagonalization solver of Sangalli and Tani.  The generalized eigenproblems of the small 1D
pairs ``(K_k, M_k)`` are solved on the host (setup); the application ``(x)U_k . D^-1 . (x)U_k^T`` runs on the device.

``PatchSystem(kvs, geo, rhs, bcs, kind)``: assembles the mass or stiffness matrix of a patch on the device and solves the
Dirichlet problem there by preconditioned CG (``igx_solver_*``, pyiga_amd/csrc/solve.hip).  The matrix never leaves the
device; only the solution vector comes back.  What the reference does with ``RestrictedLinearSystem`` and ``make_solver`` /
``cg`` on a host matrix.

``MultipatchSystem(MP, problem, rhs, bcs)``: the same for the global system of a ``Multipatch``.  The sums
``sum_p X_p A_p X_p^T`` and ``sum_p X_p b_p`` are formed on the device and solved there (CSR SpMV over the global pattern;
Jacobi, an additive Schwarz preconditioner of one fast-diagonalization solve per patch, or a geometric multigrid V-cycle with
coloured Gauss-Seidel smoothing, ``precond='mg'``); only the Dirichlet values go up and only the solution comes down.
``coarsen_knots``, ``fixed_sides`` and ``first_fit_colouring`` are the host pieces of the multigrid set-up.

``FormSystem(problem, kvs, rhs, bcs, args)``: the Dirichlet problem of any form whose values the device assembles (general form
strings, the convection-diffusion form, ...), solved there by right-preconditioned BiCGStab -- what the reference does with
``assemble.assemble`` + ``RestrictedLinearSystem`` + ``make_solver`` (a direct LU) on the host.  ``method='bicgstab'`` also
lets ``PatchSystem`` and ``MultipatchSystem`` solve by BiCGStab; ``MultipatchSystem`` then accepts non-symmetric forms.

``VectorFormSystem(problem, kvs, rhs, bcs, bfuns=[('u', nc), ('v', nc)], geo=geo)``: the same for vector-valued forms (linear
elasticity, grad-div, ...): the nc x nc scalar blocks are assembled on the device and stay there; a block SpMV and a
block-diagonal fast-diagonalization preconditioner serve CG or BiCGStab.

``MultipatchVectorSystem(MP, problem, rhs, bcs, bfuns=[('u', nc), ('v', nc)])``: vector-valued forms on a multipatch (elasticity
on a multi-patch solid): the nc x nc blocks are summed over the one global pattern and solved with one block CSR SpMV per
product, Jacobi or a block-diagonal additive Schwarz preconditioner.

``ParabolicSystem(kvs, geo, rhs, bcs, problem=None)``: the heat equation ``M u' = f - K u`` (or any device-valued form as K) of
one patch, integrated on the device by a DIRK scheme with constant steps (``integrate``; the reference's ``crank_nicolson``,
``sdirk3``, ..., pyiga/solvers.py:366-473).  Every stage solves with ``C = M + tau gamma K``; M, K and C stay on the device, and
only the saved states come down.  ``dirk_tableau(name)`` gives the tableaux of the named schemes.
``integrate_adaptive`` chooses the step from the embedded rule of ``sdirk21``, ``dirk34``, ``esdirk23``, ``esdirk34``
(``embedded_tableau``) or of the Rosenbrock methods ``ros3p``, ``ros3pw``, ``rowdaind2``, ``rodasp``, ``rosi2p1``
(``rosenbrock_tableau``; pyiga/solvers.py:475-534, 684-939): the error estimate, its norm and the mass solve run on the device,
the accept/reject controller on the host.

``EigenSystem(kvs, geo, bcs)``, ``MultipatchEigenSystem(MP, bcs)`` and ``VectorEigenSystem(problem, kvs, bcs, bfuns=[('u', nc),
('v', nc)], geo=geo)``: the lowest eigenpairs of ``K x = lam M x`` on one patch, on a multipatch, and for a vector-valued form
(elastic vibration, ``M`` the same mass matrix for every component), by block LOBPCG (``lobpcg_loop``) with the matrices, the
blocks and the preconditioner on the device.

``SaddlePointSystem((kvs_u, kvs_p), geo, bcs)`` and ``OseenSystem((kvs_u, kvs_p), geo, bcs, viscosity=nu, w=wind)``: the Stokes
system ``[[A, B^T], [B, 0]]`` by preconditioned MINRES, and the Oseen system -- the same with a frozen-wind convection term in the
velocity block -- by right-preconditioned restarted GMRES with a block-diagonal or block-triangular preconditioner.

``solve_hmultigrid(hs, A, f, ...)``, ``local_mg_step(...)`` and ``HierarchicalSystem(hs, problem, rhs, geo=geo)``: the local
multigrid of the reference for hierarchical (HB / THB) spline spaces (pyiga/solvers.py:174-324) with the level matrices, the
transfers and the coloured Gauss-Seidel sweeps on the device (``HMultigrid``, csrc/hmg.hip), as a stationary iteration or as the
preconditioner of CG.
"""
import ctypes as C
import math
import re
import warnings

import numpy as np
import scipy.linalg
import scipy.sparse
import scipy.sparse.linalg

from . import _lib
from . import assemblers
from . import boundary_terms as _bt
from .boundary_terms import BoundaryTerm
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


def _check_method(method):
    if method not in _lib.METHODS:
        raise ValueError("unknown method %r: 'cg' or 'bicgstab'" % (method,))


def _bcs_arrays(bcs):
    """Sorted unique fixed dofs and their values (a repeated dof keeps its first value, as combine_bcs)."""
    if bcs is None:
        return np.zeros(0, dtype=np.int64), np.zeros(0)
    idx = np.asarray(bcs[0], dtype=np.int64).ravel()
    vals = np.broadcast_to(np.asarray(bcs[1], dtype=np.float64), idx.shape)
    idx, first = np.unique(idx, return_index=True)
    return idx, np.ascontiguousarray(vals[first])


def fastdiag_factors(kvs, lo, hi, stiff, mats1d=None):
    """Per axis of the box ``lo[k] <= i_k < hi[k]`` the eigenvectors ``U_k`` and eigenvalues ``lam_k`` of the 1D matrices on the
    box range, and the ``IGX_KRON_*`` mode of the fast-diagonalization inverse: ``eigh(K_k, M_k)`` with ``IGX_KRON_SUM`` if
    `stiff`, else ``eigh(M_k)`` with ``IGX_KRON_PRODUCT``.  `mats1d(kv)`: ``(K, M)`` of a knot vector (default: the device's
    ``bsp_stiffness_1d`` / ``bsp_mass_1d``; K is not used, and may be None, unless `stiff`)."""
    if mats1d is None:
        from .assemble import bsp_mass_1d, bsp_stiffness_1d

        def mats1d(kv):
            return (bsp_stiffness_1d(kv) if stiff else None), bsp_mass_1d(kv)
    U, lam = [], []
    for kv, a, b in zip(kvs, lo, hi):
        K, M = mats1d(kv)
        M = _dense(M)[a:b, a:b]
        w, V = scipy.linalg.eigh(_dense(K)[a:b, a:b], M) if stiff else scipy.linalg.eigh(M)
        U.append(np.ascontiguousarray(V))
        lam.append(np.ascontiguousarray(w))
    return U, lam, (_lib.IGX_KRON_SUM if stiff else _lib.IGX_KRON_PRODUCT)


def _box_args(lo, hi, U, lam):
    """The ctypes arrays ``(box_lo, box_hi, U, lam)`` of ``igx_solver_set_precond`` and its kin: three slots per box (one box, or
    the boxes of all patches one after the other), an absent factor (None) a null pointer.  The caller keeps the NumPy arrays
    alive over the call."""
    n = max(3, len(lo))
    ptrs = lambda arrays: (_lib._dp * n)(*[None if a is None else _lib.dptr(a) for a in arrays])
    return (C.c_int32 * n)(*lo), (C.c_int32 * n)(*hi), ptrs(U), ptrs(lam)


def _schwarz_args(boxes, U, lam):
    """``_box_args`` of the boxes and factors of all patches (``schwarz_boxes``, ``schwarz_factors``): three slots per patch, the
    slots of a missing third axis 0 / null."""
    slots = lambda per_patch, fill: [v[k] if k < len(v) else fill for v in per_patch for k in range(3)]
    return _box_args(slots([b[0] for b in boxes], 0), slots([b[1] for b in boxes], 0), slots(U, None), slots(lam, None))


class _DeviceSystem:
    """What the device-resident Dirichlet problems share: the solver handle (``igx_solver_*``) and its lifecycle, the method, the
    preconditioner, the solve and the solver's SpMV and preconditioner alone.

    A subclass sets ``PRECONDS`` (preconditioner names -> ``IGX_PRECOND_*``), ``_ctx`` (the context of the device vectors) and
    ``n``, creates the handle with ``_attach``, and implements ``_set_factors(handle)`` (the preconditioner ``FACTORED`` that
    needs a host set-up).  ``_drop_owner()`` is what ``close()`` releases besides the handle: the ``patch``, unless it is the
    caller's (``_own_patch`` False); a system that owns something else overrides it.  ``_factors_set``: the set-up is done once
    and kept (else it runs whenever ``FACTORED`` is chosen)."""
    PRECONDS = _lib.PRECONDS
    FACTORED = 'kron'
    handle = None
    _factors_set = False
    _own_patch = True

    def _attach(self, create, args, bcs, method, initial):
        """The device solver made by `create` (``igx_solver_create*``, leading arguments `args`) with the fixed dofs of `bcs`;
        its method is `initial`, then `method`."""
        self.bc_indices, self.bc_values = _bcs_arrays(bcs)
        idx = self.bc_indices
        self._precond = None
        self.info = None
        h = C.c_void_p()
        _lib.check(getattr(_lib.load(), create)(*args, idx.ctypes.data_as(C.POINTER(C.c_int64)), idx.size, C.byref(h)), create)
        self.handle = h.value
        self.method = initial
        self.set_method(method)

    def _live(self):
        if not self.handle:
            raise _lib.IgxError('%s: the solver was closed (that of a MultipatchSystem also when its Multipatch is closed or '
                                're-joined)' % type(self).__name__)
        return self.handle

    def set_method(self, method):
        """'cg' or 'bicgstab' for the following solves.  CG on a matrix that is not known to be symmetric positive definite
        raises IgxError (IGX_ERR_UNSUPPORTED)."""
        _check_method(method)
        if method != self.method:
            _lib.check(_lib.load().igx_solver_set_method(self._live(), _lib.METHODS[method]), 'igx_solver_set_method')
            self.method = method

    def set_precond(self, precond):
        key = precond if precond is not None else 'none'
        if key not in self.PRECONDS:
            raise ValueError('unknown preconditioner %r' % (precond,))
        h = self._live()
        if key == self._precond:
            return
        if key == self.FACTORED and not self._factors_set:
            self._set_factors(h)
        else:
            _lib.check(_lib.load().igx_solver_set_precond(h, self.PRECONDS[key], None, None, None, None, 0), 'igx_solver_set_precond')
        self._precond = key

    def _drop_owner(self):
        if getattr(self, 'patch', None) is not None and self._own_patch:
            self.patch.close()
        self.patch = None

    def _release(self):
        if self.handle:
            _lib.load().igx_solver_destroy(self.handle)
            self.handle = None

    def close(self):
        self._release()
        self._drop_owner()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _solve(self, b, tol, maxiter, precond, x0, check_every, timed):
        """The solve with the host right-hand side `b`, or with the vector the device holds (multipatch sums) if None."""
        self.set_precond(precond)
        u = np.empty(self.n)
        x0a = None if x0 is None else np.ascontiguousarray(x0, dtype=np.float64).ravel()
        if x0a is not None and x0a.size != self.n:
            raise ValueError('x0 has the wrong size')
        ba = None if b is None else np.ascontiguousarray(b, dtype=np.float64).ravel()
        if ba is not None and ba.size != self.n:
            raise ValueError('b has the wrong size')
        lib = _lib.load()
        info = _lib.SolveInfo()
        _lib.check(lib.igx_solver_solve(self._live(), None if ba is None else _lib.dptr(ba), _lib.dptr(self.bc_values),
                                        None if x0a is None else _lib.dptr(x0a), float(tol), int(maxiter), int(check_every),
                                        1 if timed else 0, _lib.dptr(u), C.byref(info)),
                   'igx_solver_solve')
        reason = lib.igx_solver_last_breakdown(self.handle)
        self.info = dict(info.as_dict(), converged=bool(info.converged), precond=self._precond, method=self.method,
                         breakdown=_lib.BREAKDOWNS.get(reason, reason))
        return u

    def _device_op(self, fn, what, x):
        x = np.ascontiguousarray(x, dtype=np.float64).ravel()
        if x.size != self.n:
            raise ValueError('vector of %d entries, the system has %d' % (x.size, self.n))
        h = self._live()
        d_x = DeviceArray.from_host(self._ctx, x)
        d_y = DeviceArray(self._ctx, self.n)
        _lib.check(fn(h, d_x.ptr, d_y.ptr), what)
        return d_y.download()

    def spmv(self, x):
        """``R A R^T x`` on the device (vectors of all dofs in and out)."""
        return self._device_op(_lib.load().igx_solver_spmv_d, 'igx_solver_spmv_d', x)

    def apply_precond(self, r, precond=None):
        """``z = P r`` on the device (vectors of all dofs in and out) with the preconditioner of the last solve, or `precond`
        (a name of ``PRECONDS``, or None) if given."""
        if precond is not None:
            self.set_precond(precond)
        return self._device_op(_lib.load().igx_solver_precond_d, 'igx_solver_precond_d', r)


class _PatchErrorNorms:
    """``error_norms`` of the one-patch systems: they have ``self.patch`` and ``self.kvs``."""

    def error_norms(self, u, exact=None, grad_exact=None, elementwise=False):
        """``(l2, h1)`` of ``u_h - exact`` for a solution `u` of this system (host dofs, a scalar ``BSplineFunc`` or a
        ``DeviceArray``), `exact` and `grad_exact` functions of the physical coordinates: ``approx.error_norms`` on the system's
        own patch, so the geometry is not set up a second time."""
        from . import approx
        if self.patch is None:
            raise _lib.IgxError('%s: the system was closed' % type(self).__name__)
        return approx.error_norms(self.kvs, self.patch.geo, u, exact, grad_exact, elementwise=elementwise, patch=self.patch)


class PatchSystem(_PatchErrorNorms, _DeviceSystem):
    """The Dirichlet problem ``A u = b`` with ``u = g`` on the dofs of `bcs`, for the mass or stiffness matrix of one patch,
    assembled and solved on the device.

    `rhs`: the load vector (any shape with ``prod(ndofs)`` entries), or a function of the physical coordinates whose load vector
    is then formed with ``assemble.inner_products``.  `bcs`: ``(indices, values)`` as ``compute_dirichlet_bcs`` returns them, or
    None.  `boundary_terms`: ``BoundaryTerm`` objects (Robin / impedance matrices and Neumann / Robin loads on sides of the
    patch): the face matrices are added on the device to the values the patch holds there, the face loads to the load vector
    (DESIGN.md section 29); a fixed dof on such a side keeps its Dirichlet value.  ``solve(...)`` returns the completed full
    vector and leaves the solver's statistics in ``info``.  ``spmv(x)`` (``R A R^T x``) and ``apply_precond(r)`` (``z = P r``)
    run the solver's SpMV and preconditioner alone on the device.
    """
    _terms = None                             # boundary_terms.PatchTerms of the system, or None
    _sigma = 0.0                              # 1^T R 1 of its boundary matrices (the shift of the pure-Robin Kronecker preconditioner)

    def __init__(self, kvs, geo, rhs, bcs=None, kind='stiffness', device=None, method='cg', boundary_terms=None):
        self.kvs = tuple(kvs)
        self.kind = kind
        if kind not in _lib.KINDS:
            raise ValueError('unknown kind %r' % (kind,))
        _check_method(method)
        self._set_terms(boundary_terms, geo, method)
        self.patch = assemblers.DevicePatch(self.kvs, geo, device=device)
        self.ndofs = self.patch.ndofs
        self.n = int(np.prod(self.ndofs))
        if kind in ('mass', 'stiffness'):
            self.patch.assemble(kind, to_host=False)            # the values stay on the device
            self._add_term_matrices()
        if callable(rhs):
            from . import assemble
            rhs = assemble.inner_products(self.kvs, rhs, f_physical=True, geo=geo)
        self._create(rhs, bcs, 'igx_solver_create', 'cg', method)

    def _set_terms(self, boundary_terms, geo, method):
        """The boundary terms, checked and set up on the host (ValueError before any device work)."""
        terms = _bt.check_terms(boundary_terms, len(self.kvs), method=method, who=type(self).__name__)
        if terms:
            self._terms = _bt.PatchTerms(self.kvs, geo, terms, method=method, who=type(self).__name__)
            self._sigma = self._terms.sigma()

    def _add_term_matrices(self):
        """The face matrices added to the values the patch holds on the device: after the assembly, before the solver is made."""
        if self._terms is not None:
            self._terms.add_matrices(self.patch.add_face)

    def _create(self, rhs, bcs, create, initial, method):
        """Right-hand side, Dirichlet data and the device solver (igx_solver_create or igx_solver_create_general)."""
        self.b = np.ascontiguousarray(rhs, dtype=np.float64).ravel()
        if self.b.size != self.n:
            raise ValueError('right-hand side has %d entries, the space %d' % (self.b.size, self.n))
        if self._terms is not None:
            try:
                if self._terms.has_rhs:
                    self.b = self._terms.add_loads(self.b.copy())
            finally:
                self._terms.close()                               # (the face patches: their values have been added)
        self._ctx = self.patch.ctx
        self._attach(create, (self.patch.handle, _lib.KINDS[self.kind]), bcs, method, initial)
        self.box = dirichlet_box(self.ndofs, self.bc_indices)

    def _kron_factors(self):
        """Per-axis eigenvectors and eigenvalues of the 1D Dirichlet matrices of the free range.  With boundary matrices and no
        fixed dof at all (pure Robin) the stiffness-like kinds get ``lam_k + s / d``, ``s = 1^T R 1 / |parametric domain|`` the
        Rayleigh quotient of the boundary matrices on the constant: the constant mode (``sum lam_k = 0``) stays invertible."""
        stiff = self.kind != 'mass'                           # (any other form: the parametric Laplacian of the free box)
        U, lam, mode = fastdiag_factors(self.kvs, self.box[0], self.box[1], stiff)
        if stiff and self._terms is not None and self._terms.has_matrix and self.bc_indices.size == 0:
            shift = _bt.kron_shift(self.kvs, self._sigma)
            lam = [l + shift for l in lam]
        return U, lam, mode

    def _set_factors(self, h):
        if self.box is None:
            raise ValueError("precond='kron' needs the Dirichlet dofs to be a union of whole sides of the patch")
        U, lam, mode = self._kron_factors()
        lo, hi, Up, Lp = _box_args(self.box[0], self.box[1], U, lam)
        _lib.check(_lib.load().igx_solver_set_precond(h, _lib.IGX_PRECOND_KRON, lo, hi, Up, Lp, mode), 'igx_solver_set_precond')

    def solve(self, tol=1e-8, maxiter=1000, precond='kron', x0=None, check_every=1, timed=False):
        """CG (or BiCGStab, see ``method``) to ``||r|| <= tol * ||R (b - A ext(g))||``; returns the full solution vector (the
        Dirichlet values included)."""
        return self._solve(self.b, tol, maxiter, precond, x0, check_every, timed)


_HOST_VALUED = ("FormSystem solves forms whose matrix values the device assembles and keeps; %s leaves its values on the "
                "host.  Solve it on the device through a one-patch multipatch instead: "
                "MultipatchSystem(Multipatch([(kvs, geo)]), problem, rhs, bcs, method='bicgstab')")


def _check_device_form(problem, kvs, args):
    """ValueError, before any device work, for a problem whose values would not stay on the device: vector-valued / boundary /
    surface forms (FormAssembler), forms with second or parametric derivatives (parametric jet forms, assembled in passes),
    functionals, and assembler classes or objects of other kinds."""
    from . import assemble, forms
    from .assemblers import _DeviceAssembler, _ParametricFormAssembler
    if isinstance(problem, str):
        geo = args.get('geo')
        if geo is None:
            raise ValueError("required input parameter 'geo' missing")
        if getattr(geo, 'dim', len(kvs)) != len(kvs):
            raise ValueError(_HOST_VALUED % 'a surface form')
        if re.search(r'\bds\b', problem):
            raise ValueError(_HOST_VALUED % 'a boundary form')
        if assemble._KNOWN_FORMS.get(assemble._normalise_form(problem)) is not None:
            return
        try:
            if forms.arity(problem) != 2:
                raise ValueError('FormSystem needs a bilinear form, not a linear functional: %r' % (problem,))
        except NotImplementedError as e:
            raise ValueError('FormSystem: %s' % e)
        # the class of the form decided on one host point (inputs that cannot be evaluated there are left to the assembler)
        d = len(kvs)
        try:
            forms.coefficient_table(problem, (1,) * d, np.full((1,) * d + (d,), 0.5), dict(args))
        except NotImplementedError:
            raise ValueError(_HOST_VALUED % 'a form with second or parametric derivatives (a parametric jet form)')
        except Exception:
            pass
        return
    cls = problem if isinstance(problem, type) else type(problem)
    if not issubclass(cls, _DeviceAssembler) or issubclass(cls, _ParametricFormAssembler):
        raise ValueError(_HOST_VALUED % cls.__name__)


class FormSystem(PatchSystem):
    """The Dirichlet problem ``A u = b``, ``u = g`` on the dofs of `bcs`, for the matrix of `problem` on one patch, assembled and
    solved on the device by BiCGStab (``method='bicgstab'``; 'cg' for a symmetric positive definite kind).

    `problem`: anything ``assemble.instantiate_assembler`` turns into a device assembler (a form string such as the
    convection-diffusion form of the reference's notebook, an assembler class or object); `args` / `kwargs`: its inputs,
    ``geo`` among them.  Forms whose values stay on the host (vector-valued, boundary or surface forms, second or parametric
    derivatives) raise ValueError.  `rhs`: a vector, a scalar, a function of the physical coordinates (``inner_products``) or
    a linear form string (``'f*v*dx'``).  `boundary_terms`: as for ``PatchSystem``.  ``solve()`` uses the Kronecker preconditioner of the parametric Laplacian on the free
    box when the Dirichlet dofs are whole sides, else Jacobi.
    """

    def __init__(self, problem, kvs, rhs, bcs=None, args=None, method='bicgstab', boundary_terms=None, **kwargs):
        from . import assemble
        _check_method(method)
        args = dict(args or {})
        args.update(kwargs)
        self.kvs = tuple(kvs)
        _check_device_form(problem, self.kvs, args)
        self._set_terms(boundary_terms, args.get('geo'), method)
        self.assembler = assemble.instantiate_assembler(problem, self.kvs, args)
        self._own_patch = self.assembler is not problem
        self.patch = self.assembler.patch
        self.kind = self.assembler._kind
        self.ndofs = self.patch.ndofs
        self.n = int(np.prod(self.ndofs))
        self.patch.assemble(self.kind, to_host=False)            # the values stay on the device
        self._add_term_matrices()
        if isinstance(rhs, str):
            rhs = assemble.assemble(rhs, self.kvs, args=args)
        elif callable(rhs):
            rhs = assemble.inner_products(self.kvs, rhs, f_physical=True, geo=args['geo'])
        elif np.ndim(rhs) == 0:
            rhs = np.full(self.n, float(rhs))
        self._create(rhs, bcs, 'igx_solver_create_general', 'bicgstab', method)

    @property
    def default_precond(self):
        return 'kron' if self.box is not None else 'jacobi'

    def solve(self, tol=1e-8, maxiter=1000, precond='auto', x0=None, check_every=1, timed=False):
        """BiCGStab to ``||r|| <= tol * ||R (b - A ext(g))||``; returns the full solution vector.  `precond`: 'auto' (see the
        class), 'kron', 'jacobi' or None."""
        return self._solve(self.b, tol, maxiter, self.default_precond if precond == 'auto' else precond, x0, check_every, timed)


################################################################################
# Vector-valued Dirichlet problems of one patch on the device
################################################################################

def _vector_components(problem, kvs, args, bfuns, who='VectorFormSystem'):
    """The number of components of a vector-valued volume form that `who` (VectorFormSystem, MultipatchVectorSystem, ...) solves;
    ValueError, before any device work, for anything else (no ``geo``, a surface or boundary form, not bilinear, trial and test
    components that differ, a scalar form, more than three components)."""
    from . import tforms
    if not isinstance(problem, str):
        raise ValueError('%s needs a form string, not %r' % (who, problem))
    geo = args.get('geo')
    if geo is None:
        raise ValueError("required input parameter 'geo' missing")
    if getattr(geo, 'dim', len(kvs)) != len(kvs) or re.search(r'\bds\b', problem):
        raise ValueError('%s solves volume forms (dx), not surface or boundary forms: %r' % (who, problem))
    bf = tforms.normalise_bfuns(problem, bfuns)
    if any(space != 0 for _, _, space in bf):
        raise ValueError('%s: basis functions in different spaces (mixed systems are assembled, not solved, on the device)' % who)
    if len(bf) != 2:
        raise ValueError('%s needs a bilinear form (trial and test function), not arity %d: %r' % (who, len(bf), problem))
    (_, ncu, _), (_, ncv, _) = bf
    if ncu != ncv:
        raise ValueError('%s: trial and test functions have %d and %d components (mixed systems are not '
                         'supported)' % (who, ncu, ncv))
    if ncu == 1:
        raise ValueError('%s: %r is a scalar form: solve it with FormSystem' % (who, problem))
    if ncu not in (2, 3):
        raise ValueError('%s solves forms of 2 or 3 components, not %d' % (who, ncu))
    return ncu


def symmetric_block_tables(table, rtol=1e-13):
    """True if the coefficient tables of a vector-valued form (``table[p][q][r][s]``: test component p with jet r, trial component
    q with jet s; arrays on the Gauss grid or None) give a symmetric block matrix: ``C^{pq}_{rs} == C^{qp}_{sr}`` within `rtol`
    of the largest entry of all tables, a None only opposite a None."""
    nc = len(table)
    big = 0.0
    for row in table:
        for tab in row:
            for trow in tab:
                for e in trow:
                    if e is not None:
                        big = max(big, float(np.max(np.abs(e))))
    for p in range(nc):
        for q in range(nc):
            A, B = table[p][q], table[q][p]
            for r in range(len(A)):
                for s in range(len(A[r])):
                    a, b = A[r][s], B[s][r]
                    if (a is None) != (b is None):
                        return False
                    if a is not None and np.max(np.abs(np.asarray(a) - np.asarray(b))) > rtol * big:
                        return False
    return True


class _VectorBlocks:
    """What the device systems of a vector-valued form share (``VectorFormSystem``, ``VectorEigenSystem``): the hand-over of the
    nc x nc scalar blocks to a block solver, the free box of every component and the block-diagonal Kronecker factors.  They
    supply ``kvs``, ``ndofs``, ``N``, ``ncomp``, ``patch``, ``handle`` and ``bc_indices``."""

    def _take_blocks(self, table):
        """Every block of `table` that is not absent, assembled (IGX_FORM) and handed to the solver; ``present[p][q]``."""
        from .form_assemblers import _full_table
        lib = _lib.load()
        nc, d = self.ncomp, len(self.kvs)
        self.present = [[False] * nc for _ in range(nc)]
        for p in range(nc):
            for q in range(nc):
                tab = table[p][q]
                if all(e is None for row in tab for e in row):
                    continue                      # (an absent block: zero, never read)
                self.patch.set_form(_full_table(tab, d))
                self.patch.assemble('form', to_host=False)
                _lib.check(lib.igx_solver_take_block(self.handle, p, q), 'igx_solver_take_block')
                self.present[p][q] = True

    def _component_boxes(self):
        idx = self.bc_indices
        self.boxes = [dirichlet_box(self.ndofs, idx[(idx >= c * self.N) & (idx < (c + 1) * self.N)] - c * self.N)
                      for c in range(self.ncomp)]

    @property
    def default_precond(self):
        return 'kron' if all(b is not None for b in self.boxes) else 'jacobi'

    def kron_factors(self):
        """Per component ``(lo, hi, U, lam, mode)``: the fast diagonalization of the parametric Laplacian on its free box.  A
        component without a wholly fixed side gets ``sigma / d`` added to every ``lam_k`` (``sigma = min_k lam_k[1]``, as a
        floating Schwarz patch): the inverse stays symmetric positive definite."""
        out = []
        for c, box in enumerate(self.boxes):
            if box is None:
                raise ValueError("precond='kron' needs the Dirichlet dofs of every component to be a union of whole sides of the "
                                 "patch (component %d is not)" % c)
            lo, hi = box
            U, lam, mode = fastdiag_factors(self.kvs, lo, hi, True)
            floating = all(a == 0 for a in lo) and all(b == kv.numdofs for b, kv in zip(hi, self.kvs))
            if floating and all(len(l) > 1 for l in lam):
                sigma = min(l[1] for l in lam)
                lam = [l + sigma / len(lam) for l in lam]
            out.append((lo, hi, U, lam, mode))
        return out

    def _set_block_kron(self, h):
        """The factors of every component on the device (``igx_solver_set_block_kron``)."""
        lib = _lib.load()
        for c, (lo, hi, U, lam, mode) in enumerate(self.kron_factors()):
            lo_, hi_, Up, Lp = _box_args(lo, hi, U, lam)
            _lib.check(lib.igx_solver_set_block_kron(h, c, lo_, hi_, Up, Lp, mode), 'igx_solver_set_block_kron')


class VectorFormSystem(_VectorBlocks, _DeviceSystem):
    """The Dirichlet problem ``A u = b``, ``u = g`` on the dofs of `bcs`, for a vector-valued form (``bfuns=[('u', nc),
    ('v', nc)]``, nc = 2 or 3: linear elasticity, grad-div, ...) on one patch, assembled and solved on the device.

    The nc x nc scalar blocks ``A_pq`` are assembled one after the other (IGX_FORM) and handed to the block solver of
    ``igx_solver_create_block``; only the right-hand side goes up and the solution comes down.  Vectors have ``nc * N`` entries in
    the reference's 'blocked' layout (component-major, as ``assemble(..., layout='blocked')``).  `method`: 'auto' is CG when the
    coefficient tables are symmetric (``symmetric``), else BiCGStab; 'cg' on a non-symmetric form raises ValueError.  `rhs`: a
    vector of ``nc * N`` entries or of shape ``(nc,) + ndofs``, a scalar, or a linear form string in the test function.  `bcs`:
    ``(indices, values)`` in the blocked numbering, as ``compute_dirichlet_bcs`` gives them for a vector-valued ``dir_func``.
    ``solve()`` uses the block-diagonal Kronecker preconditioner (the fast diagonalization of the parametric Laplacian on each
    component's free box) when the Dirichlet dofs of every component are whole sides, else Jacobi.
    """

    def __init__(self, problem, kvs, rhs, bcs=None, args=None, bfuns=None, method='auto', **kwargs):
        from . import assemble
        from .form_assemblers import FormAssembler
        if method != 'auto':
            _check_method(method)
        args = dict(args or {})
        args.update(kwargs)
        self.kvs = tuple(kvs)
        nc = _vector_components(problem, self.kvs, args, bfuns)
        self.ncomp = nc
        self.assembler = FormAssembler(self.kvs, args['geo'], problem, bfuns=bfuns, inputs=args)
        self.patch = self.assembler.patch
        table = self.assembler._table
        self.symmetric = symmetric_block_tables(table)
        if method == 'auto':
            method = 'cg' if self.symmetric else 'bicgstab'
        elif method == 'cg' and not self.symmetric:
            raise ValueError('VectorFormSystem: CG needs a symmetric form; the coefficient tables of %r are not symmetric: '
                             "method='bicgstab'" % (problem,))
        self.ndofs = self.patch.ndofs
        self.N = int(np.prod(self.ndofs))
        self.n = nc * self.N
        if isinstance(rhs, str):
            test = _test_function_name(problem, bfuns)
            rhs = assemble.assemble(rhs, self.kvs, args=args, bfuns=[(test, nc)], layout='blocked')
        elif np.ndim(rhs) == 0:
            rhs = np.full(self.n, float(rhs))
        self.b = np.ascontiguousarray(rhs, dtype=np.float64).ravel()
        if self.b.size != self.n:
            raise ValueError('right-hand side has %d entries, the space %d x %d' % (self.b.size, nc, self.N))
        self._ctx = self.patch.ctx
        initial = 'cg' if self.symmetric else 'bicgstab'
        self._attach('igx_solver_create_block', (self.patch.handle, nc, 1 if self.symmetric else 0), bcs, method, initial)
        self._take_blocks(table)
        self._component_boxes()

    def _set_factors(self, h):
        self._set_block_kron(h)
        _lib.check(_lib.load().igx_solver_set_precond(h, _lib.IGX_PRECOND_KRON, None, None, None, None, 0), 'igx_solver_set_precond')
        self._factors_set = True

    def solve(self, tol=1e-8, maxiter=1000, precond='auto', x0=None, check_every=1, timed=False):
        """CG or BiCGStab (``method``) to ``||r|| <= tol * ||R (b - A ext(g))||``; returns the full blocked solution vector of
        ``nc * N`` entries (the Dirichlet values included).  `precond`: 'auto' (see the class), 'kron', 'jacobi' or None."""
        return self._solve(self.b, tol, maxiter, self.default_precond if precond == 'auto' else precond, x0, check_every, timed)


class SaddlePointSystem(_VectorBlocks, _DeviceSystem):
    """The Stokes-type saddle-point problem ``[[A, B^T], [B, 0]] (u, p) = (f, 0)``, ``(u, p) = g`` on the dofs of `bcs`, on one
    patch, assembled and solved on the device with preconditioned MINRES (the reference's solve-stokes notebook without its
    ``bmat`` and ``spsolve``).

    `kvs` = ``(kvs_u, kvs_p)``: the velocity space (every component) and the pressure space, e.g. a Taylor-Hood pair, on one
    mesh.  `a`: the velocity form in ``u`` and ``v`` (``ncomp`` components each), times `viscosity`; its coefficient tables must
    be symmetric.  `b`: the form over the two spaces in ``u`` (space 0) and ``p`` (space 1), assembled as
    ``form_assemblers.FormAssembler`` assembles forms over two spaces (its role rule and mesh checks apply).  Both are assembled
    on one ``DevicePatch`` over `kvs_u` whose Gauss rule has ``max(p over both spaces) + 1`` points per span -- the blocks of `a`
    are integrated with that rule too, not with the ``p_u + 1`` points ``assemble.assemble`` takes for `a` alone.
    Vectors have ``nc * N_u + N_p`` entries: the velocity components first, component-major, then the pressure (the notebook's
    ordering).  `bcs`: ``(indices, values)`` in that numbering.  `rhs`: a full vector, a linear form string in the velocity test
    function ``v``, or a scalar (every velocity entry); the pressure part of the latter two is 0.

    ``solve()`` returns the full vector; ``split(u)`` gives the coefficient arrays of velocity and pressure."""
    PRESSURES = ('auto', 'mean', None)
    METHOD = 'minres'

    def __init__(self, kvs, geo, bcs, rhs=0.0, a='inner(grad(u), grad(v)) * dx', b='div(u) * p * dx', ncomp=None, viscosity=1.0,
                 args=None, **inputs):
        from . import assemble, tforms
        from .form_assemblers import FormAssembler, _full_table, is_space_pair
        if not is_space_pair(kvs):
            raise ValueError('SaddlePointSystem needs kvs=(kvs_u, kvs_p): the velocity and the pressure space')
        self.kvs = tuple(kvs[0])
        self.kvs_p = tuple(kvs[1])
        d = len(self.kvs)
        nc = d if ncomp is None else int(ncomp)
        if nc not in (2, 3):
            raise ValueError('SaddlePointSystem solves systems of 2 or 3 velocity components, not %d' % nc)
        if not (viscosity > 0.0 and np.isfinite(viscosity)):
            raise ValueError('viscosity must be positive')
        self.ncomp, self.viscosity = nc, float(viscosity)
        self.ndofs = tuple(int(kv.numdofs) for kv in self.kvs)
        self.ndofs_p = tuple(int(kv.numdofs) for kv in self.kvs_p)
        self.N, self.Np = int(np.prod(self.ndofs)), int(np.prod(self.ndofs_p))
        self.n = nc * self.N + self.Np
        idx, _ = _bcs_arrays(bcs)
        if idx.size and (idx.min() < 0 or idx.max() >= self.n):
            raise ValueError('bcs: dof %d outside of the %d x %d + %d unknowns' % (idx.max() if idx.max() >= self.n else idx.min(),
                                                                                  nc, self.N, self.Np))
        args = dict(args or {})
        args.update(inputs)
        fargs = {k: v for k, v in args.items() if k != 'geo'}
        bf_a, bf_b = [('u', nc), ('v', nc)], [('u', nc, 0), ('p', 1, 1)]
        # (the structure of the tables at one point, before anything exists on the device; the values are checked below)
        _, _, t1, _ = tforms.evaluate(a, (1,) * d, np.zeros((1,) * d + (d,)), fargs, bf_a)
        if not symmetric_block_tables(t1):
            raise ValueError('SaddlePointSystem: the coefficient tables of a=%r are not symmetric; non-symmetric velocity forms '
                             '(Oseen, Navier-Stokes: BiCGStab or GMRES on the saddle-point matrix) are not supported' % (a,))
        self.asm_b = FormAssembler((self.kvs, self.kvs_p), geo, b, bfuns=bf_b, inputs=fargs)
        self.patch, self.pair = self.asm_b.patch, self.asm_b.pair
        try:                                   # (from here on a patch exists on the device: close() on any failure)
            if self.pair is None:
                raise ValueError('SaddlePointSystem: b=%r does not couple the two spaces' % (b,))
            self.asm_a = FormAssembler(self.kvs, geo, a, bfuns=bf_a, inputs=fargs, patch=self.patch)
            table = self.asm_a._table
            if not symmetric_block_tables(table):
                raise ValueError('SaddlePointSystem: the coefficient tables of a=%r are not symmetric; non-symmetric velocity '
                                 'forms (Oseen, Navier-Stokes: BiCGStab or GMRES on the saddle-point matrix) are not '
                                 'supported' % (a,))
            if self.viscosity != 1.0:
                table = [[[[None if e is None else self.viscosity * np.asarray(e, dtype=np.float64) for e in row] for row in tab]
                          for tab in trow] for trow in table]
            table = self._velocity_tables(table, geo, fargs)
            if isinstance(rhs, str):
                f = assemble.assemble(rhs, self.kvs, args=dict(fargs, geo=geo), bfuns=[('v', nc)], layout='blocked')
                rhs = np.concatenate((np.asarray(f, dtype=np.float64).ravel(), np.zeros(self.Np)))
            elif np.ndim(rhs) == 0:
                rhs = np.concatenate((np.full(nc * self.N, float(rhs)), np.zeros(self.Np)))
            self.b = np.ascontiguousarray(rhs, dtype=np.float64).ravel()
            if self.b.size != self.n:
                raise ValueError('right-hand side has %d entries, the system %d x %d + %d' % (self.b.size, nc, self.N, self.Np))
            self._ctx = self.patch.ctx
            self.method = self.METHOD
            self._attach('igx_solver_create_saddle', (self.patch.handle, self.pair.handle, nc), bcs, self.METHOD, self.METHOD)
            self._take_blocks(table)
            lib = _lib.load()
            for q in range(nc):
                self.patch.set_form(_full_table(self.asm_b._table[0][q], d))
                self.pair.assemble('form', to_host=False)
                _lib.check(lib.igx_solver_take_pair_block(self.handle, self.pair.handle, q), 'igx_solver_take_pair_block')
        except Exception:
            self.close()
            raise
        self._component_boxes()
        pidx = self.bc_indices[self.bc_indices >= nc * self.N] - nc * self.N
        self.pressure_fixed = pidx
        self.enclosed = pidx.size == 0 and all(box is not None and all(a_ == 1 for a_ in box[0]) and
                                               all(b_ == n_ - 1 for b_, n_ in zip(box[1], self.ndofs)) for box in self.boxes)
        self._velocity_factors_set = False

    def _velocity_tables(self, table, geo, fargs):
        """The coefficient tables of the velocity block from the (scaled) tables of `a`: those themselves."""
        return table

    def set_method(self, method):
        """'minres' is the only method of a saddle-point system; 'cg' and 'bicgstab' raise IgxError (IGX_ERR_UNSUPPORTED)."""
        if method not in _lib.SADDLE_METHODS:
            raise ValueError("unknown method %r: 'minres'" % (method,))
        if method != self.method:
            _lib.check(_lib.load().igx_solver_set_method(self._live(), _lib.SADDLE_METHODS[method]), 'igx_solver_set_method')
            self.method = method

    def _drop_owner(self):
        if getattr(self, 'pair', None) is not None:
            self.pair.close()
        self.pair = None
        _DeviceSystem._drop_owner(self)

    def kron_factors(self):
        """As ``_VectorBlocks.kron_factors``, of `viscosity` times the parametric Laplacian."""
        return [(lo, hi, U, [self.viscosity * l for l in lam], mode) for lo, hi, U, lam, mode in _VectorBlocks.kron_factors(self)]

    def schur_factors(self):
        """``(lo, hi, U, lam, mode)`` of the pressure part ``(x) M_k^-1``: on the whole pressure space, or on the free box when the
        fixed pressure dofs are whole sides."""
        box = dirichlet_box(self.ndofs_p, self.pressure_fixed)
        lo, hi = box if box is not None else ((0,) * len(self.ndofs_p), self.ndofs_p)
        return (lo, hi) + fastdiag_factors(self.kvs_p, lo, hi, False)

    def _set_schur(self, h, key):
        lib = _lib.load()
        if key == 'kron':
            lo, hi, U, lam, mode = self.schur_factors()
            lo_, hi_, Up, Lp = _box_args(lo, hi, U, lam)
            _lib.check(lib.igx_solver_set_saddle_schur(h, _lib.IGX_PRECOND_KRON, lo_, hi_, Up, Lp, mode, None, self.viscosity),
                       'igx_solver_set_saddle_schur')
        else:                                  # the inverse diagonal of (x) M_k
            from .assemble import bsp_mass_1d
            diag = np.ones(1)
            for kv in self.kvs_p:
                diag = np.multiply.outer(diag, _dense(bsp_mass_1d(kv)).diagonal()).ravel()
            dinv = np.ascontiguousarray(1.0 / diag)
            _lib.check(lib.igx_solver_set_saddle_schur(h, _lib.IGX_PRECOND_JACOBI, None, None, None, None, 0, _lib.dptr(dinv),
                                                       self.viscosity), 'igx_solver_set_saddle_schur')

    def set_precond(self, precond):
        """'kron': ``diag(F_0, .., F_{nc-1}, viscosity (x) M_k^-1)`` with ``F_c`` the fast diagonalization of `viscosity` times the
        parametric Laplacian on the free box of component c; 'jacobi': the inverse diagonals of the ``A_cc`` and of the pressure
        mass matrix; None."""
        key = precond if precond is not None else 'none'
        if key not in self.PRECONDS:
            raise ValueError('unknown preconditioner %r' % (precond,))
        h = self._live()
        if key == self._precond:
            return
        if key == 'kron' and not self._velocity_factors_set:
            self._set_block_kron(h)
            self._velocity_factors_set = True
        if key != 'none':
            self._set_schur(h, key)
        _lib.check(_lib.load().igx_solver_set_precond(h, self.PRECONDS[key], None, None, None, None, 0), 'igx_solver_set_precond')
        self._precond = key

    def solve(self, tol=1e-8, maxiter=1000, precond='auto', pressure='auto', x0=None, check_every=1, timed=False):
        """Preconditioned MINRES to ``phi_k <= tol * phi_0`` (MINRES's estimate of ``sqrt(r^T P r)``); returns the full vector
        (Dirichlet values included).  ``info['relres']`` is the true relative residual from one more product, ``info['breakdown']``
        None, 'nonfinite' or 'indefinite_precond'.

        `precond`: 'auto' ('kron' when the Dirichlet dofs of every velocity component are whole sides, else 'jacobi'), 'kron',
        'jacobi' or None.  `pressure`: when every velocity component is fixed on the whole boundary and no pressure dof is, the
        matrix is singular with the constant pressure (all coefficients 1) as its kernel; 'auto' and 'mean' then remove the
        mean of the lifted pressure right-hand side (warning if it exceeds 1e-10 of its norm: the data is incompatible), solve
        unpinned and shift the pressure so that its first coefficient ('auto', the notebook's normalisation) or its coefficient
        mean ('mean') is 0.  None does nothing of this: an outflow boundary, or a pinned dof in `bcs`."""
        if pressure not in self.PRESSURES:
            raise ValueError("unknown pressure %r: 'auto', 'mean' or None" % (pressure,))
        if precond != 'auto' and (precond if precond is not None else 'none') not in self.PRECONDS:
            raise ValueError('unknown preconditioner %r' % (precond,))
        h = self._live()
        lib = _lib.load()
        project = pressure is not None and self.enclosed
        _lib.check(lib.igx_solver_saddle_projection(h, 1 if project else 0, None, None), 'igx_solver_saddle_projection')
        u = self._solve(self.b, tol, maxiter, self.default_precond if precond == 'auto' else precond, x0, check_every, timed)
        if project:
            mean, norm = C.c_double(), C.c_double()
            _lib.check(lib.igx_solver_saddle_projection(h, -1, C.byref(mean), C.byref(norm)), 'igx_solver_saddle_projection')
            self.info.update(rhs_mean=mean.value, rhs_norm=norm.value)
            if abs(mean.value) > 1e-10 * norm.value:
                import warnings
                warnings.warn('SaddlePointSystem: the pressure right-hand side has mean %.3e against a norm of %.3e: the data is '
                              'not compatible with an enclosed flow; its mean was removed' % (mean.value, norm.value))
            nv = self.ncomp * self.N
            u[nv:] -= u[nv] if pressure == 'auto' else u[nv:].mean()
        return u

    def split(self, u):
        """``(U, P)``: the velocity coefficients of shape ``ndofs_u + (nc,)`` and the pressure coefficients of shape ``ndofs_p``,
        ready for ``BSplineFunc(kvs_u, U)`` and ``BSplineFunc(kvs_p, P)``."""
        u = np.asarray(u)
        nv = self.ncomp * self.N
        U = np.stack([u[c * self.N:(c + 1) * self.N].reshape(self.ndofs) for c in range(self.ncomp)], axis=-1)
        return U, u[nv:].reshape(self.ndofs_p)


def add_block_tables(ta, tb):
    """The entry-wise sum of two coefficient tables of a vector-valued form (``table[p][q][r][s]``: arrays on one Gauss grid or
    None); a None entry is zero, an entry absent in both stays None."""
    def add(x, y):
        if x is None:
            return y
        if y is None:
            return x
        return np.asarray(x, dtype=np.float64) + np.asarray(y, dtype=np.float64)
    return [[[[add(x, y) for x, y in zip(ra, rb)] for ra, rb in zip(xa, xb)] for xa, xb in zip(pa, pb)] for pa, pb in zip(ta, tb)]


def _check_convection(convection, kvs_u, kvs_p, nc, fargs):
    """ValueError, before any device work, unless `convection` is None or a bilinear volume form in ``u`` and ``v`` of `nc`
    components each.  The form is evaluated at one point: inputs given as arrays over the Gauss grid enter with their first
    value, callables with their value at the origin."""
    from . import tforms
    if convection is None:
        return
    if not isinstance(convection, str):
        raise ValueError('OseenSystem: convection must be a form string or None, not %r' % (convection,))
    if re.search(r'\bds\b', convection):
        raise ValueError('OseenSystem: the convection term is a volume form (dx), not a surface or boundary form: %r' % (convection,))
    d = len(kvs_u)
    nqp = max(kv.p for kv in tuple(kvs_u) + tuple(kvs_p)) + 1
    G = tuple(int(kv.numspans) * nqp for kv in kvs_u)
    point = {}
    for name, val in fargs.items():
        if not callable(val) and np.ndim(val) >= d and np.shape(val)[:d] == G:
            val = np.asarray(val, dtype=np.float64)[(0,) * d][(None,) * d]
        point[name] = val
    try:
        arity, measure, table, ncs = tforms.evaluate(convection, (1,) * d, np.zeros((1,) * d + (d,)), point, [('u', nc), ('v', nc)])
    except Exception as e:
        raise ValueError('OseenSystem: convection=%r is not a bilinear volume form in u and v of %d components each: %s'
                         % (convection, nc, e))
    if arity != 2 or measure != 'dx' or tuple(ncs) != (nc, nc) or len(table) != nc or any(len(row) != nc for row in table):
        raise ValueError('OseenSystem: convection=%r is not a bilinear volume form (dx) in u and v of %d components each'
                         % (convection, nc))


class OseenSystem(SaddlePointSystem):
    """The Oseen problem ``[[nu A + N, B^T], [B, 0]] (u, p) = (f, 0)`` on one patch -- the linear system of every step of the
    reference's solve-navier-stokes notebook, ``Re^-1 A_grad + A_linconv(vel)`` with the wind frozen -- assembled and solved on
    the device with right-preconditioned restarted GMRES.

    Everything is ``SaddlePointSystem``'s except the velocity block, `viscosity` times the (symmetric) form `a` plus the form
    `convection` in ``u`` and ``v``, which is not scaled and need not be symmetric, and the Krylov method.  `convection` is
    evaluated on the same Gauss grid as `a` and `b`, and its coefficient tables are added to those of `a` before the blocks are
    assembled; its inputs (the wind ``w``) are what vector-valued forms accept: a callable of the physical coordinates that
    returns a tuple, or an array over the Gauss grid with a trailing component axis.  ``convection=None``: the Stokes system,
    solved by GMRES.  `restart`: the length of a GMRES cycle (1 to 128), the default of ``solve``."""
    METHOD = 'gmres'
    MAX_RESTART = 128

    def __init__(self, kvs, geo, bcs, rhs=0.0, convection='grad(u).dot(w).dot(v) * dx', a='inner(grad(u), grad(v)) * dx',
                 b='div(u) * p * dx', ncomp=None, viscosity=1.0, restart=40, args=None, **inputs):
        from .form_assemblers import is_space_pair
        if not is_space_pair(kvs):
            raise ValueError('OseenSystem needs kvs=(kvs_u, kvs_p): the velocity and the pressure space')
        self.restart = self._check_restart(restart)
        nc = len(kvs[0]) if ncomp is None else int(ncomp)
        fargs = dict(args or {})
        fargs.update(inputs)
        fargs.pop('geo', None)
        if nc in (2, 3):                           # (any other count: the parent's refusal)
            _check_convection(convection, kvs[0], kvs[1], nc, fargs)
        self.convection = convection
        SaddlePointSystem.__init__(self, kvs, geo, bcs, rhs=rhs, a=a, b=b, ncomp=ncomp, viscosity=viscosity, args=args, **inputs)

    @classmethod
    def _check_restart(cls, restart):
        if not (isinstance(restart, (int, np.integer)) and 1 <= restart <= cls.MAX_RESTART):
            raise ValueError('restart must be an integer from 1 to %d, not %r' % (cls.MAX_RESTART, restart))
        return int(restart)

    def _velocity_tables(self, table, geo, fargs):
        """`viscosity` times the tables of `a` (given) plus those of the convection form on the same patch."""
        from .form_assemblers import FormAssembler
        self._geo, self._fargs, self._visc_table = geo, dict(fargs), table       # (kept for update())
        if self.convection is None:
            return table
        asm = FormAssembler(self.kvs, geo, self.convection, bfuns=[('u', self.ncomp), ('v', self.ncomp)], inputs=fargs, patch=self.patch)
        return add_block_tables(table, asm._table)

    # -- the convection blocks of a live system replaced
    WIND_FORM = 'grad(u).dot(w).dot(v) * dx'
    _d_atab = _d_wind = _phases = None

    def _replace_blocks(self, table):
        """``_take_blocks`` on a live solver: every block of `table` that is not absent is assembled and replaces the solver's
        (``igx_solver_replace_block``: the buffers change hands, nothing is allocated after the first replacement)."""
        from .form_assemblers import _full_table
        lib = _lib.load()
        nc, d = self.ncomp, len(self.kvs)
        for p in range(nc):
            for q in range(nc):
                tab = table[p][q]
                if all(e is None for row in tab for e in row):
                    if self.present[p][q]:             # (only an off-diagonal block can be: the diagonal ones carry `a`)
                        _lib.check(lib.igx_solver_hide_block(self.handle, p, q, 1), 'igx_solver_hide_block')
                    continue
                self.patch.set_form(_full_table(tab, d))
                self.patch.assemble('form', to_host=False)
                _lib.check(lib.igx_solver_replace_block(self.handle, p, q), 'igx_solver_replace_block')
                self.present[p][q] = True

    def _gauss_shape(self):
        return tuple(int(self.patch.info.ngauss[k]) for k in range(len(self.kvs)))

    def _device_a_tables(self):
        """The unscaled tables of `a` on the device, uploaded once: ``[p][q]`` a 4x4 table of device pointers, or None."""
        if self._d_atab is None:
            nc, d, G = self.ncomp, len(self.kvs), self._gauss_shape()
            out = [[None] * nc for _ in range(nc)]
            for p in range(nc):
                for q in range(nc):
                    tab = self.asm_a._table[p][q]
                    where = [(r, s) for r in range(d + 1) for s in range(d + 1) if tab[r][s] is not None]
                    if not where:
                        continue
                    ptrs = self.patch.upload_fields([np.broadcast_to(np.asarray(tab[r][s], dtype=np.float64), G) for r, s in where],
                                                    buf='_d_atab_%d%d' % (p, q))
                    out[p][q] = [[None] * 4 for _ in range(4)]
                    for (r, s), ptr in zip(where, ptrs):
                        out[p][q][r][s] = ptr
            self._d_atab = out
        return self._d_atab

    def _velocity_dofs(self, w):
        """The component-major velocity dofs (``nc * N`` entries) of `w`: a full solution vector, its velocity part, or a
        coefficient array of shape ``ndofs + (nc,)``; None if `w` is none of these."""
        if callable(w):
            return None
        w = np.asarray(w, dtype=np.float64)
        nv = self.ncomp * self.N
        if w.ndim == 1 and w.size in (self.n, nv):
            return np.ascontiguousarray(w[:nv])
        if w.shape == self.ndofs + (self.ncomp,) and w.shape != self._gauss_shape() + (self.ncomp,):
            return np.ascontiguousarray(np.moveaxis(w, -1, 0)).ravel()
        return None

    def _wind_blocks(self, d_u, newton=False, want_grad=None, evaluate=True):
        """The blocks of ``viscosity a + (w . grad) u v`` -- with `newton` also ``+ (u . grad) w v`` -- for the wind with the
        device dofs `d_u`, assembled and replaced: one fused evaluation of the wind (igx_patch_eval_vspline_d; with the gradient
        if `want_grad`, default `newton`; not `evaluate`: the arrays of the last evaluation serve again), the tables formed on
        the device (igx_patch_set_form_sum_d).  Returns the number of blocks assembled; with ``self._phases`` a list, the device
        ms of the evaluation and of the assemblies are noted there."""
        lib = _lib.load()
        nc, d = self.ncomp, len(self.kvs)
        if nc != d:
            raise ValueError('a wind given by its dofs needs as many velocity components as dimensions')
        atab = self._device_a_tables()
        timed = self._phases is not None
        if evaluate:
            self._wind = self.patch.eval_vspline(d_u, nc, want_grad=newton if want_grad is None else want_grad)
            if timed:
                self._phases.append(dict(wind_ms=self.patch.timing()['total_ms']))
        vals, grads = self._wind
        count, asm_ms = 0, 0.0
        for p in range(nc):
            for q in range(nc):
                if p != q and not newton:
                    continue
                b = [[None] * 4 for _ in range(4)]
                if p == q:
                    for j in range(d):
                        b[0][1 + j] = vals[j]                     # (w . grad u_p) v_p: trial jet 1 + j, coefficient w_j
                if newton:
                    b[0][0] = grads[p][q]                         # (u_q d w_p / d x_q) v_p
                self.patch.set_form_sum_resident(atab[p][q], self.viscosity, b)
                self.patch.assemble('form', to_host=False)
                if timed:
                    asm_ms += self.patch.timing()['total_ms']
                _lib.check(lib.igx_solver_replace_block(self.handle, p, q), 'igx_solver_replace_block')
                self.present[p][q] = True
                count += 1
        if not newton:                                            # Newton blocks of an earlier step must not enter a Picard matrix
            for p in range(nc):
                for q in range(nc):
                    if p != q and self.present[p][q]:
                        if atab[p][q] is not None:
                            self.patch.set_form_sum_resident(atab[p][q], self.viscosity, None)
                            self.patch.assemble('form', to_host=False)
                            _lib.check(lib.igx_solver_replace_block(self.handle, p, q), 'igx_solver_replace_block')
                            count += 1
                        else:
                            _lib.check(lib.igx_solver_hide_block(self.handle, p, q, 1), 'igx_solver_hide_block')
        if timed:
            self._phases.append(dict(assembly_ms=asm_ms, blocks=count))
        return count

    def update(self, **inputs):
        """Replaces the convection blocks of the live system by those of new inputs of the convection form, usually
        ``update(w=...)``; ``solve()`` afterwards behaves as on a system constructed with them.  ``B``, ``B^T``, the
        preconditioner factors and every buffer stay (a selected Jacobi preconditioner takes the new diagonals).

        A callable or an array over the Gauss grid goes through the host tables, exactly as the constructor does.  ``w`` given as
        a full solution vector (or its velocity part) or as a coefficient array of shape ``ndofs + (nc,)`` -- a spline of the
        velocity space, e.g. the solution of a previous solve -- is evaluated and turned into tables on the device; that needs
        the default convection form."""
        from .form_assemblers import FormAssembler
        self._live()
        if self.convection is None:
            raise ValueError('OseenSystem.update: the system was made without a convection form')
        dofs = self._velocity_dofs(inputs['w']) if set(inputs) == {'w'} else None
        if dofs is not None:
            if self.convection != self.WIND_FORM:
                raise ValueError('OseenSystem.update: a wind given by its dofs needs convection=%r' % (self.WIND_FORM,))
            if self._d_wind is None:
                self._d_wind = DeviceArray(self._ctx, self.ncomp * self.N)
            self._d_wind.upload(dofs)
            self._wind_blocks(self._d_wind.ptr)
            return
        fargs = dict(self._fargs, **inputs)
        _check_convection(self.convection, self.kvs, self.kvs_p, self.ncomp, fargs)
        asm = FormAssembler(self.kvs, self._geo, self.convection, bfuns=[('u', self.ncomp), ('v', self.ncomp)], inputs=fargs, patch=self.patch)
        self._replace_blocks(add_block_tables(self._visc_table, asm._table))
        self._fargs = fargs

    def _drop_owner(self):
        if self._d_wind is not None:
            self._d_wind.free()
            self._d_wind = None
        SaddlePointSystem._drop_owner(self)

    def set_method(self, method):
        """'gmres' is the only method of an Oseen system."""
        if method != 'gmres':
            raise ValueError("unknown method %r: 'gmres'" % (method,))
        self.method = method

    def _select(self, precond, triangular, restart):
        """GMRES(restart) with the triangular or the block-diagonal form of the preconditioner `precond` selected on the device."""
        key = self.default_precond if precond == 'auto' else precond
        tri = bool(triangular) and key is not None
        _lib.check(_lib.load().igx_solver_set_gmres(self._live(), int(restart), 1 if tri else 0), 'igx_solver_set_gmres')
        return tri

    def solve(self, tol=1e-8, maxiter=1000, precond='auto', triangular=True, pressure='auto', x0=None, check_every=1, timed=False,
              restart=None):
        """Right-preconditioned GMRES(`restart`, default the system's) to ``|g_k| <= tol * ||r_0||``, GMRES's own residual norm;
        returns the full vector (Dirichlet values included).  `precond` and `pressure` as ``SaddlePointSystem.solve``;
        `triangular`: the block upper-triangular form ``[[F, B^T], [0, -S]]^-1`` of the preconditioner instead of the
        block-diagonal one (ignored for ``precond=None``).  ``info['iterations']`` counts Arnoldi steps, ``info['restarts']`` the
        cycles after the first, ``info['relres']`` is the true relative residual, ``info['breakdown']`` None or 'nonfinite'."""
        restart = self.restart if restart is None else self._check_restart(restart)
        if precond != 'auto' and (precond if precond is not None else 'none') not in self.PRECONDS:
            raise ValueError('unknown preconditioner %r' % (precond,))
        tri = self._select(precond, triangular, restart)
        u = SaddlePointSystem.solve(self, tol=tol, maxiter=maxiter, precond=precond, pressure=pressure, x0=x0, check_every=check_every,
                                    timed=timed)
        self.info.update(restarts=int(_lib.load().igx_solver_gmres_restarts(self.handle)), restart=restart, triangular=tri)
        return u

    def apply_precond(self, r, precond=None, triangular=True):
        """``z = P r`` on the device, as ``solve`` applies it: the triangular form when `triangular` (and a preconditioner is
        selected)."""
        if precond is not None:
            self.set_precond(precond)
        self._select(self._precond if self._precond != 'none' else None, triangular, self.restart)
        return self._device_op(_lib.load().igx_solver_precond_d, 'igx_solver_precond_d', r)


def _test_function_name(problem, bfuns):
    """The name of the test function of the bilinear form `problem` (the last of its basis functions)."""
    from . import tforms
    return tforms.normalise_bfuns(problem, bfuns)[-1][0]


################################################################################
# Multi-patch Dirichlet problems on the device
################################################################################

def schwarz_boxes(shapes, maps, fixed):
    """The box of every patch for the Schwarz preconditioner: ``[(lo, hi), ...]`` with ``lo[k] <= i_k < hi[k]``.

    `shapes`: dofs per axis of each patch; `maps`: the local-to-global index of each patch (``patch_to_global_idx``); `fixed`:
    the fixed global dofs.  Axis k of patch p drops its first index if the whole side ``(k, 0)`` of the patch is fixed and its
    last index if the whole side ``(k, 1)`` is.  Other fixed local dofs stay in the box (the device masks them)."""
    nglobal = max([int(np.max(m)) + 1 for m in maps if len(m)] + [0])
    fixed = np.asarray(fixed, dtype=np.int64).ravel()
    mask = np.zeros(max(nglobal, int(fixed.max()) + 1 if fixed.size else 0), dtype=bool)
    mask[fixed] = True
    boxes = []
    for shape, l2g in zip(shapes, maps):
        shape = tuple(int(n) for n in shape)
        loc = mask[np.asarray(l2g, dtype=np.int64)].reshape(shape)
        lo, hi = [], []
        for k, n in enumerate(shape):
            a = 1 if np.take(loc, 0, axis=k).all() else 0
            b = n - 1 if np.take(loc, n - 1, axis=k).all() else n
            lo.append(a)
            hi.append(max(a, b))
        boxes.append((tuple(lo), tuple(hi)))
    return boxes


def schwarz_factors(kvs_list, boxes, kind='stiffness', mats1d=None):
    """Per patch and axis the eigenvectors ``U`` and eigenvalues ``lam`` of the 1D matrices on the box range, and the
    ``IGX_KRON_*`` mode: ``eigh(K_k, M_k)`` with ``IGX_KRON_SUM`` for stiffness, ``eigh(M_k)`` with ``IGX_KRON_PRODUCT`` for
    mass (as :class:`PatchSystem`).  A floating stiffness patch -- no wholly fixed side, ``sum lam`` has a zero -- gets
    ``sigma / d`` added to every ``lam_k``, ``sigma = min_k lam_k[1]``: the inverse of the fast diagonalization of
    ``K + sigma M``, symmetric positive definite.  `mats1d(kv)`: ``(K, M)`` of a knot vector (default: the device's
    ``bsp_stiffness_1d`` / ``bsp_mass_1d``)."""
    if kind not in ('mass', 'stiffness'):
        raise ValueError('the Schwarz preconditioner has a Kronecker set-up for mass and stiffness only, not %r' % (kind,))
    U, lam, mode = [], [], None
    for kvs, (lo, hi) in zip(kvs_list, boxes):
        Up, Lp, mode = fastdiag_factors(kvs, lo, hi, kind == 'stiffness', mats1d)
        floating = all(a == 0 for a in lo) and all(b == kv.numdofs for b, kv in zip(hi, kvs))
        if kind == 'stiffness' and floating and all(len(l) > 1 for l in Lp):
            sigma = min(l[1] for l in Lp)
            Lp = [l + sigma / len(Lp) for l in Lp]
        U.append(Up)
        lam.append(Lp)
    return U, lam, mode


def coarsen_knots(kv):
    """The knot vector of `kv` without every second interior mesh point (the first, third, ... of them, with all their copies):
    its space is nested in that of `kv`, and ``coarsen_knots(kv.refine()) == kv``.  ValueError if the number of spans is odd or
    below 2."""
    from . import bspline
    ns = kv.numspans
    if ns < 2 or ns % 2:
        raise ValueError('a knot vector of %d spans cannot be coarsened (an even number >= 2 is needed)' % ns)
    return bspline.KnotVector(kv.kv[~np.isin(kv.kv, kv.mesh[1:-1:2])], kv.p)


def fixed_sides(kvs_list, maps, fixed):
    """The patch sides ``[(patch, axis, side), ...]`` all of whose dofs are in `fixed` (global dofs; `maps`: the local-to-global
    index of each patch).  ValueError, naming the first offending dof, unless `fixed` is exactly the union of these sides."""
    from .multipatch import slice_indices
    fixed = np.unique(np.asarray(fixed, dtype=np.int64).ravel())
    nglobal = max([int(np.max(m)) + 1 for m in maps if len(m)] + [int(fixed.max()) + 1 if fixed.size else 0])
    mask = np.zeros(nglobal, dtype=bool)
    mask[fixed] = True
    covered = np.zeros(nglobal, dtype=bool)
    sides = []
    for p, (kvs, l2g) in enumerate(zip(kvs_list, maps)):
        shape = tuple(kv.numdofs for kv in kvs)
        l2g = np.asarray(l2g, dtype=np.int64)
        for ax in range(len(shape)):
            for side in (0, 1):
                g = l2g[slice_indices(ax, 0 if side == 0 else -1, shape, ravel=True)]
                if mask[g].all():
                    sides.append((p, ax, side))
                    covered[g] = True
    rest = np.flatnonzero(mask & ~covered)
    if rest.size:
        raise ValueError('the multigrid preconditioner needs the fixed dofs to be a union of whole patch sides: dof %d is fixed '
                         'and lies on no wholly fixed side' % int(rest[0]))
    return sides


def first_fit_colouring(indptr, indices, free=None):
    """``(colour, ncolours)`` of the first-fit colouring of the CSR pattern under the mask `free` (``igx_csr_colouring``: host code
    of the library, no device): rows in ascending order take the smallest colour none of their coloured neighbours has; -1 on
    the rows that are not free."""
    indptr = np.ascontiguousarray(indptr, dtype=np.int32)
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    n = indptr.size - 1
    fm = None if free is None else np.ascontiguousarray(free, dtype=np.uint8)
    if fm is not None and fm.size != n:
        raise ValueError('the mask has %d entries, the pattern %d rows' % (fm.size, n))
    colour = np.empty(n, dtype=np.int32)
    nc = C.c_int32(0)
    _lib.check(_lib.load().igx_csr_colouring(n, indptr.ctypes.data_as(C.POINTER(C.c_int32)), indices.ctypes.data_as(C.POINTER(C.c_int32)),
                                             None if fm is None else fm.ctypes.data_as(C.POINTER(C.c_uint8)),
                                             colour.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(nc)), 'igx_csr_colouring')
    return colour, int(nc.value)


MG_BLOCK_ROWS = 1024        # a level of at most this many free dofs runs every sweep in one launch of one block


class _MultipatchMultigrid:
    """The geometric multigrid hierarchy of a system on a multipatch (DESIGN.md sections 17 and 37): built, inspected and dropped
    here for ``MultipatchSystem`` (and through it ``MultipatchEigenSystem``) and ``MultipatchVectorSystem``.  ``_mg`` is None or
    ``dict(systems=[self, coarser, ...], smooth_steps=, info=[mg_info entry per level])``.

    A class supplies ``MP`` and what differs between the systems: ``_refuse_multigrid()`` (ValueError when the system cannot have
    a hierarchy, before any work), ``_mg_fixed_sides(kvs, maps)``, ``_level_system(MPc, bcs)``, ``_set_smoother(smooth_steps,
    ...)``, and the names ``_MG_COARSE`` / ``_MG_INVERSE`` / ``_MG_ORDER_KEY``."""

    _mg = None
    _MG_COARSE, _MG_INVERSE = 'igx_solver_set_mg_coarse', 'igx_solver_set_mg_inverse'      # the C calls of a level's links
    _MG_ORDER_KEY = 'free'                    # the mg_info entry that counts what the smoother colours (``mg_colour_order``)

    def _drop_owner(self):
        self._drop_multigrid()
        MP = getattr(self, 'MP', None)
        if MP is not None:
            MP._solvers.discard(self)

    def _drop_multigrid(self):
        mg, self._mg = self._mg, None
        if mg:
            for S in mg['systems'][1:]:
                S.close()
                S.MP.close()
            if self._precond == 'mg':
                self._precond = None

    def set_method(self, method):
        if method == 'bicgstab' and getattr(self, '_precond', None) == 'mg':
            raise ValueError("precond='mg' serves method='cg' only")
        super().set_method(method)

    def _build_multigrid(self, levels, coarse, smooth_steps, coarse_max, *smoother_args):
        """``set_multigrid`` of every system: the coarse multipatches (coarsened and re-joined, or `coarse`) with the same patch
        sides fixed, their systems, then on the device every level's smoother (``S._set_smoother(smooth_steps,
        *smoother_args)``, the finest first), the links of every pair of levels and the dense inverse of the coarsest.  A
        failure closes every coarse level made so far and leaves the system without a hierarchy."""
        from . import bspline
        from .multipatch import slice_indices
        self._refuse_multigrid()
        self._live()
        MP = self.MP
        if not MP.injective:
            raise ValueError('the multigrid preconditioner needs injective local-to-global maps (two dofs of one patch share a '
                             'global dof)')
        smooth_steps = int(smooth_steps)
        if not 1 <= smooth_steps <= 16:
            raise ValueError('smooth_steps must be 1 .. 16')
        if levels is not None and int(levels) < 1:
            raise ValueError('levels must be >= 1')
        sides = self._mg_fixed_sides([kvs for kvs, _ in MP.patches], [MP.patch_to_global_idx(p) for p in range(MP.numpatches)])
        self._drop_multigrid()
        lib = _lib.load()
        systems, keep = [self], []                # (keep: the host tables stay referenced until the calls that read them are over)
        try:
            given = None if coarse is None else list(coarse)
            while True:
                S = systems[-1]
                nfree = S.n - S.bc_indices.size
                if given is not None:
                    if not given:
                        break
                    MPc = given.pop(0)
                    if MPc.numpatches != MP.numpatches:
                        raise ValueError('a coarse multipatch has %d patches, the system %d' % (MPc.numpatches, MP.numpatches))
                else:
                    if (levels is not None and len(systems) >= int(levels)) or (levels is None and nfree <= coarse_max):
                        break
                    try:
                        patches = [(tuple(coarsen_knots(kv) for kv in kvs), geo) for kvs, geo in S.MP.patches]
                    except ValueError:
                        break
                    MPc = MP.replay_joins(patches)
                # the sides of component c, fixed on the coarse multipatch: its scalar dofs numbered from c * Nc
                Nc = MPc.numdofs
                fixed = [c * Nc + MPc.patch_to_global_idx(p)[slice_indices(ax, 0 if side == 0 else -1,
                                                                           tuple(kv.numdofs for kv in MPc.patches[p][0]), ravel=True)]
                         for c, of_c in enumerate(sides) for p, ax, side in of_c]
                fixed = np.unique(np.concatenate(fixed)) if fixed else np.zeros(0, dtype=np.int64)
                try:
                    Sc = self._level_system(MPc, (fixed, np.zeros(fixed.size)))
                except Exception:
                    MPc.close()
                    raise
                systems.append(Sc)
            coarsest = systems[-1]
            m = coarsest.n - coarsest.bc_indices.size
            if m > coarse_max:
                raise ValueError('the coarsest level keeps %d free dofs, more than coarse_max = %d' % (m, coarse_max))
            info = [S._set_smoother(smooth_steps, *smoother_args) for S in systems]
            for F, Cs in zip(systems[:-1], systems[1:]):
                np_ = MP.numpatches
                Ps = []
                for (kf, _), (kc, _) in zip(F.MP.patches, Cs.MP.patches):
                    Ps += [np.ascontiguousarray(bspline.prolongation(c, f).toarray()) for c, f in zip(kc, kf)] + [None] * (3 - len(kf))
                keep.append(Ps)
                N = F.MP.numdofs                  # (the multiplicities are those of the scalar dofs, whatever the components)
                mult = np.zeros(N)
                for p in range(np_):
                    mult += np.bincount(F.MP.patch_to_global_idx(p), minlength=N)
                Pp = (_lib._dp * (3 * np_))(*[None if a is None else _lib.dptr(a) for a in Ps])
                _lib.check(getattr(lib, self._MG_COARSE)(F._live(), Cs._live(), Pp, _lib.dptr(mult)), self._MG_COARSE)
            # the coarsest matrix on its free dofs (blocked: of all components), inverted on the host
            A = coarsest.matrix()
            fr = np.setdiff1d(np.arange(coarsest.n), coarsest.bc_indices)
            inv = scipy.linalg.inv(A[fr][:, fr].toarray()) if fr.size else np.zeros((0, 0))
            inv = np.ascontiguousarray(0.5 * (inv + inv.T))
            _lib.check(getattr(lib, self._MG_INVERSE)(coarsest._live(), _lib.dptr(inv), fr.size), self._MG_INVERSE)
        except Exception:
            for S in systems[1:]:
                S.close()
                S.MP.close()
            raise
        self._mg = dict(systems=systems, smooth_steps=smooth_steps, info=info)
        if self._precond == 'mg':
            self._precond = None                  # (the device dropped it when the hierarchy changed)
        return self

    def _mg_solve_info(self, precond):
        """``levels`` and ``smooth_steps`` in ``info`` after a solve preconditioned with `precond` = 'mg'."""
        if precond == 'mg':
            self.info.update(levels=len(self._mg['systems']), smooth_steps=self._mg['smooth_steps'])

    def _mg_level(self, level):
        self._live()
        if self._mg is None:
            raise ValueError('no multigrid hierarchy yet: set_multigrid() or solve(precond=\'mg\') first')
        systems = self._mg['systems']
        if not 0 <= int(level) < len(systems):
            raise ValueError('level %r: the hierarchy has %d levels' % (level, len(systems)))
        return systems[int(level)]

    def mg_level(self, level):
        """The system of `level` of the hierarchy (0: this one): its ``MP``, ``bc_indices`` and ``matrix()``."""
        return self._mg_level(level)

    def mg_info(self):
        """Per level, the finest first: every patch's spans, dofs, free dofs, nonzeros, colours of the smoother, and whether a
        sweep is one launch of one block (``one_block``)."""
        self._mg_level(0)
        out = []
        for l, d in enumerate(self._mg['info']):
            inf = _lib.MgInfo()
            _lib.check(_lib.load().igx_solver_mg_info(self._live(), l, C.byref(inf)), 'igx_solver_mg_info')
            out.append(dict(d, one_block=bool(inf.one_block), dense_inverse=bool(inf.dense_inverse)))
        return out

    def mg_profile(self, r=None, reps=5):
        """Device milliseconds of the phases of one V-cycle (the mean of `reps` cycles on `r`, default all ones): per level the
        sweeps, the residual SpMV and the transfers; the coarsest level's dense product; the additions; the kernel launches."""
        self._mg_level(0)
        r = np.ones(self.n) if r is None else np.ascontiguousarray(r, dtype=np.float64).ravel()
        if r.size != self.n:
            raise ValueError('vector of %d entries, the system has %d' % (r.size, self.n))
        d_r = DeviceArray.from_host(self._ctx, r)
        d_z = DeviceArray(self._ctx, self.n)
        pf = _lib.MgProfile()
        _lib.check(_lib.load().igx_solver_mg_profile_d(self._live(), d_r.ptr, d_z.ptr, int(reps), C.byref(pf)), 'igx_solver_mg_profile_d')
        nl = len(self._mg['systems'])
        return dict(levels=int(pf.levels), launches=int(pf.launches), total_ms=pf.total_ms, coarse_ms=pf.coarse_ms, vector_ms=pf.vector_ms,
                    smooth_ms=list(pf.smooth_ms)[:nl], residual_ms=list(pf.residual_ms)[:nl], transfer_ms=list(pf.transfer_ms)[:nl])

    def mg_colour_order(self, level=0):
        """What the smoother of `level` colours -- the free dofs of a scalar system, the nodes with a free component of a
        vector-valued one -- in the order its forward sweep relaxes them: sorted by (colour, index)."""
        self._mg_level(level)
        inf = self._mg['info'][int(level)]
        rows = np.empty(inf[self._MG_ORDER_KEY], dtype=np.int32)
        offs = np.empty(inf['colours'] + 1, dtype=np.int32)
        _lib.check(_lib.load().igx_solver_mg_colours(self._live(), int(level), rows.ctypes.data_as(C.POINTER(C.c_int32)),
                                                     offs.ctypes.data_as(C.POINTER(C.c_int32))), 'igx_solver_mg_colours')
        return rows.astype(np.int64)

    def relax(self, x, b=None, sweep='forward', iterations=1, level=0):
        """`iterations` Gauss-Seidel sweeps of `level`'s smoother on ``R A R^T x = R b`` from `x` (vectors of all dofs of the level;
        `b` None: zero), on the device: 'forward' (colours ascending), 'backward' (descending) or 'symmetric' (one after the
        other) -- the reference's ``gauss_seidel(A, x, b, iterations, indices=mg_colour_order(level), sweep=sweep)``.  Returns
        the host vector; its fixed entries are 0."""
        if sweep not in ('forward', 'backward', 'symmetric'):
            raise ValueError('unknown sweep %r' % (sweep,))
        S = self._mg_level(level)
        x = np.ascontiguousarray(x, dtype=np.float64).ravel()
        b = np.zeros(S.n) if b is None else np.ascontiguousarray(b, dtype=np.float64).ravel()
        if x.size != S.n or b.size != S.n:
            raise ValueError('vectors of %d and %d entries, level %d has %d dofs' % (x.size, b.size, level, S.n))
        h = self._live()
        lib = _lib.load()
        d_x = DeviceArray.from_host(self._ctx, x)
        d_b = DeviceArray.from_host(self._ctx, b)
        for _ in range(int(iterations)):
            for back in {'forward': (0,), 'backward': (1,), 'symmetric': (0, 1)}[sweep]:
                _lib.check(lib.igx_solver_mg_relax_d(h, int(level), back, d_b.ptr, d_x.ptr), 'igx_solver_mg_relax_d')
        return d_x.download()

    def _transfer(self, fn, what, v, level, n_in, n_out):
        v = np.ascontiguousarray(v, dtype=np.float64).ravel()
        if v.size != n_in:
            raise ValueError('vector of %d entries, %d expected' % (v.size, n_in))
        d_in = DeviceArray.from_host(self._ctx, v)
        d_out = DeviceArray(self._ctx, n_out)
        _lib.check(fn(self._live(), int(level), d_in.ptr, d_out.ptr), what)
        return d_out.download()

    def prolong(self, xc, level=0):
        """``P xc`` on the device: from level ``level + 1`` to `level` (vectors of all dofs; fixed entries ignored / 0)."""
        F, Cs = self._mg_level(level), self._mg_level(level + 1)
        return self._transfer(_lib.load().igx_solver_mg_prolong_d, 'igx_solver_mg_prolong_d', xc, level, Cs.n, F.n)

    def restrict(self, r, level=0):
        """``P^T r`` on the device: from `level` to level ``level + 1``."""
        F, Cs = self._mg_level(level), self._mg_level(level + 1)
        return self._transfer(_lib.load().igx_solver_mg_restrict_d, 'igx_solver_mg_restrict_d', r, level, F.n, Cs.n)


class MultipatchSystem(_MultipatchMultigrid, _DeviceSystem):
    """The Dirichlet problem ``A u = b``, ``u = g`` on the dofs of `bcs`, of the global system of the multipatch `MP`, summed and
    solved on the device.

    `problem`, `rhs`, `args` / `kwargs`: as for ``MP.assemble_system`` (the same per-patch assemblies and scatters; the sums stay
    on the device).  With ``method='cg'`` (the default) the form must be symmetric: a form whose assembler declares
    ``_symmetric_form = False`` is refused.  ``method='bicgstab'`` solves any form; Schwarz then uses the stiffness factors.
    `bcs`: ``(indices, values)`` as ``MP.compute_dirichlet_bcs`` returns them, or None.  `boundary_terms`: ``BoundaryTerm``
    objects, each with its patch index (``patch=``); with a matrix form among them ``precond='mg'`` raises ValueError (the
    coarse levels would miss the boundary matrices).  ``solve(...)`` returns the completed
    global vector and leaves the solver's statistics in ``info``.  The system reads the sums `MP` holds: a later
    ``MP.assemble_system`` restarts them (a solve then raises), and ``MP.close()`` destroys the system's device solver.
    """

    PRECONDS = _lib.MP_PRECONDS
    FACTORED = 'schwarz'
    _inspect_symmetry = True                  # (False: the caller has shown the form to be symmetric before, as
                                              # MultipatchEigenSystem does for its own levels)

    def __init__(self, MP, problem, rhs, bcs=None, args=None, method='cg', boundary_terms=None, **kwargs):
        self.MP = MP
        _check_method(method)
        self._problem = (problem, rhs, dict(args or {}), dict(kwargs))
        kinds = []
        # boundary terms, set up on the host before any device work; their matrices are added to the
        # sums after the scatters, their loads to the patches' load vectors before theirs
        terms = MP._boundary_terms(boundary_terms, rhs, args, kwargs, method=method, who=type(self).__name__)
        self._matrix_terms = any(t.has_matrix for t in terms.values())

        def inspect(p, asm):
            if self._inspect_symmetry and method == 'cg' and not getattr(asm, '_symmetric_form', True):
                raise ValueError('MultipatchSystem solves by CG and needs a form known to be symmetric; the assembler of patch %d '
                                 '(%s) cannot show that its form is (general form strings never can).  Accepted: the built-in '
                                 "mass and stiffness forms ('u*v*dx', 'inner(grad(u),grad(v))*dx') and assemblers that do not "
                                 "declare _symmetric_form = False; any other form: method='bicgstab'" % (p, type(asm).__name__))
            kinds.append(getattr(asm, '_kind', None))
        h = MP._sum_system(problem, rhs, args, False, 'csr', 'blocked', kwargs, on_assembler=inspect, boundary_terms=terms)
        self.kind = kinds[0] if kinds and all(k == kinds[0] for k in kinds) else None
        self.n = MP.numdofs
        self._ctx = MP._ctx                       # (the context of the multipatch handle: device vectors of spmv / apply_precond)
        self._attach('igx_solver_create_multipatch', (h,), bcs, method, 'cg')
        MP._solvers.add(self)

    def error_norms(self, u, exact, grad_exact=None):
        """``Multipatch.error_norms`` of the system's multipatch for a global solution vector `u`."""
        return self.MP.error_norms(u, exact, grad_exact)

    # -- geometric multigrid: what _MultipatchMultigrid asks of a scalar system
    def set_precond(self, precond):
        if precond == 'mg':
            self._refuse_multigrid()
            self._live()
            if self._mg is None:
                self.set_multigrid()
        _DeviceSystem.set_precond(self, precond)

    _matrix_terms = False                     # the sums hold boundary matrices (boundary_terms with a matrix form)

    def _refuse_multigrid(self):
        if self.method != 'cg':
            raise ValueError("precond='mg' serves method='cg' only")
        if self._matrix_terms:
            raise ValueError("precond='mg' is not available with boundary terms that have a matrix form: the coarse levels assemble "
                             "`problem` again and would miss the boundary matrices (load-only terms are fine); use 'schwarz', "
                             "'jacobi' or None")

    def set_multigrid(self, levels=None, coarse=None, smooth_steps=1, coarse_max=2048, block_rows=None):
        """Sets up the hierarchy of ``precond='mg'``: a V-cycle with `smooth_steps` coloured Gauss-Seidel sweeps before (forward)
        and after (backward) the coarse correction, the coarsest level solved with a dense inverse.

        Every patch's knot vectors are coarsened with :func:`coarsen_knots` and the joins of the multipatch replayed, level after
        level, until there are `levels` of them (the finest included), a knot vector cannot be coarsened, or a level has at most
        `coarse_max` free dofs; `coarse`: the coarser multipatches ``[MP1, MP2, ...]`` instead (needed for a multipatch joined
        through bare ``join_dofs`` calls).  The same problem is assembled again on every coarse level, on the device, with the same
        patch sides fixed; the system owns the coarse multipatches and closes them with itself.  `block_rows`: levels of at most
        this many free dofs sweep in one launch of one block (default ``MG_BLOCK_ROWS``).  ValueError if the fixed dofs are not a
        union of whole patch sides, if a local-to-global map is not injective, with ``method='bicgstab'``, or if the coarsest
        level keeps more than `coarse_max` free dofs."""
        return self._build_multigrid(levels, coarse, smooth_steps, coarse_max, MG_BLOCK_ROWS if block_rows is None else int(block_rows))

    def _mg_fixed_sides(self, kvs, maps):
        """Per component (a scalar system has one) the wholly fixed patch sides, which stay fixed on every level."""
        return [fixed_sides(kvs, maps, self.bc_indices)]

    def _level_system(self, MPc, bcs):
        """The system of a coarse level of the hierarchy: the same problem on `MPc` with the fixed dofs `bcs`."""
        problem, rhs, args, kwargs = self._problem
        return MultipatchSystem(MPc, problem, rhs, bcs, args=args, **kwargs)

    def _set_smoother(self, smooth_steps, block_rows):
        """Colours the free dofs (first fit on the pattern) and hands the colours to the device; returns this level's entry of
        ``mg_info``."""
        indptr, indices = self.MP.pattern()
        free = np.ones(self.n, dtype=np.uint8)
        free[self.bc_indices] = 0
        colour, nc = first_fit_colouring(indptr, indices, free)
        _lib.check(_lib.load().igx_solver_set_mg_smoother(self._live(), colour.ctypes.data_as(C.POINTER(C.c_int32)), smooth_steps, block_rows),
                   'igx_solver_set_mg_smoother')
        return dict(spans=[tuple(kv.numspans for kv in kvs) for kvs, _ in self.MP.patches], dofs=self.n,
                    free=int(self.n - self.bc_indices.size), nnz=int(indices.size), colours=nc)

    def matrix(self):
        """The summed matrix the system solves with, downloaded: CSR over all dofs (fixed rows and columns included)."""
        self._live()
        indptr, indices = self.MP.pattern()
        data = np.empty(indices.shape[0])
        _lib.check(_lib.load().igx_multipatch_download(self.MP._device(), _lib.dptr(data), None), 'igx_multipatch_download')
        return scipy.sparse.csr_matrix((data, indices.copy(), indptr.copy()), shape=(self.n, self.n))

    def rhs(self):
        """The summed right-hand side on the device, downloaded (all dofs)."""
        self._live()
        b = np.empty(self.n)
        _lib.check(_lib.load().igx_multipatch_download(self.MP._device(), None, _lib.dptr(b)), 'igx_multipatch_download')
        return b

    def schwarz_setup(self):
        """Boxes, factors and mode of the Schwarz preconditioner (host set-up)."""
        MP = self.MP
        shapes = [tuple(kv.numdofs for kv in kvs) for kvs, _ in MP.patches]
        maps = [MP.patch_to_global_idx(p) for p in range(MP.numpatches)]
        boxes = schwarz_boxes(shapes, maps, self.bc_indices)
        kind = self.kind
        if self.method == 'bicgstab' and kind not in ('mass', 'stiffness'):
            kind = 'stiffness'                    # (a general form: the fast-diagonalization inverse of the Laplacian per patch)
        U, lam, mode = schwarz_factors([tuple(kvs) for kvs, _ in MP.patches], boxes, kind)
        return boxes, U, lam, mode

    def _set_factors(self, h):
        boxes, U, lam, mode = self.schwarz_setup()
        _lib.check(_lib.load().igx_solver_set_schwarz(h, *_schwarz_args(boxes, U, lam), mode), 'igx_solver_set_schwarz')
        self._factors_set = True

    def solve(self, tol=1e-8, maxiter=1000, precond='jacobi', x0=None, check_every=1, timed=False, b=None):
        """CG (or BiCGStab) to ``||r|| <= tol * ||R (b - A ext(g))||``; returns the global solution vector (the Dirichlet values included).
        The right-hand side is the summed vector on the device unless a host vector `b` is given.

        `precond`: 'jacobi' (default), 'schwarz', 'mg' or None.  Schwarz takes far fewer iterations, but each of them applies one
        fast-diagonalization solve per patch, a few small GEMMs that leave most of the device idle on 2D patches: on the 2D
        notebook domain (p = 3, n = 256) it takes 2.7x fewer iterations and 4x the time of Jacobi.  It pays in 3D and on
        ill-conditioned systems.

        'mg' (CG only) is one V-cycle of geometric multigrid (``set_multigrid``, called with its defaults if it was not): the
        iteration count does not grow with the refinement (21 to 23 on the notebook domain at p = 3 from n = 16 to 256, where
        Jacobi needs 1329 at n = 256), but a V-cycle is a few hundred short launches.  It wins on large systems (notebook domain
        n = 256: 28 ms against 95 ms with Jacobi; three cubes, p = 2, n = 64: 59 ms against 152 ms) and loses on small ones (notebook
        n = 64: 12 ms against 8 ms; three cubes n = 32: 37 ms against 13 ms), and its set-up (coarse assemblies, colouring, a dense
        inverse) takes 0.1 to 0.4 s on the host."""
        u = self._solve(b, tol, maxiter, precond, x0, check_every, timed)
        self._mg_solve_info(precond)
        return u


class MultipatchVectorSystem(_MultipatchMultigrid, _DeviceSystem):
    """The Dirichlet problem ``A u = b``, ``u = g`` on the dofs of `bcs`, for a vector-valued form (``bfuns=[('u', nc),
    ('v', nc)]``, nc = 2 or 3: linear elasticity, grad-div, ...) on the multipatch `MP`, summed and solved on the device
    (DESIGN.md section 28).

    Vectors have ``nc * MP.numdofs`` entries, component-major; every component uses the scalar numbering and joins of `MP`.
    Block (p, q) is ``sum_patch X A^patch_pq X^T``: the blocks are summed one after the other in the multipatch's device sums
    (every patch assembles its scalar block and scatters it) and copied into the block solver of
    ``igx_solver_create_multipatch_block``, which multiplies by all of them in one block SpMV over the global pattern.
    `method`: 'auto' is CG when the coefficient tables of every patch are symmetric (``symmetric``), else BiCGStab; 'cg' on a
    non-symmetric form raises ValueError.  `rhs`: a linear form string in the test function, a vector of ``nc * numdofs``
    entries, or a scalar.  `bcs`: ``(indices, values)`` in the blocked numbering, as ``MP.compute_dirichlet_bcs`` gives them for
    a vector-valued ``dir_func``.  Preconditioners: 'jacobi' (the default), 'schwarz', and 'mg' after ``set_multigrid()``
    (DESIGN.md section 37).

    Constructing the system restarts the sums of `MP`: a ``MultipatchSystem`` made over them before goes stale (its solves
    raise), as after ``MP.assemble_system``.  The system owns copies of its blocks, so a later ``MP.assemble_system`` does not
    disturb it; it reads the pattern of `MP`, and ``MP.close()`` destroys its device solver.
    """

    PRECONDS = _lib.MPVEC_PRECONDS
    FACTORED = 'schwarz'

    def __init__(self, MP, problem, rhs, bcs=None, bfuns=None, args=None, method='auto', **kwargs):
        if method != 'auto':
            _check_method(method)
        self.MP = MP
        args = dict(args or {})
        args.update(kwargs)
        self._problem = (problem, bfuns, dict(args))
        nc, asms, args = MP._vector_assemblers(problem, bfuns, args, 'MultipatchVectorSystem')
        try:
            self.ncomp = nc
            self.symmetric = all(symmetric_block_tables(a._table) for a in asms)
            if method == 'auto':
                method = 'cg' if self.symmetric else 'bicgstab'
            elif method == 'cg' and not self.symmetric:
                raise ValueError('MultipatchVectorSystem: CG needs a symmetric form; the coefficient tables of %r are not '
                                 "symmetric: method='bicgstab'" % (problem,))
            self.N = MP.numdofs
            self.n = nc * self.N
            self.b = MP._vector_rhs(rhs, _test_function_name(problem, bfuns), nc, args)
            h = MP._device()
            self._ctx = MP._ctx
            initial = 'cg' if self.symmetric else 'bicgstab'
            self._attach('igx_solver_create_multipatch_block', (h, nc, 1 if self.symmetric else 0), bcs, method, initial)
            MP._solvers.add(self)
            lib = _lib.load()
            self.present = MP._sum_vector_blocks(
                asms, nc, lambda p, q, _h: _lib.check(lib.igx_solver_take_multipatch_block(self.handle, p, q),
                                                      'igx_solver_take_multipatch_block'))
        finally:
            for a in asms:
                a.patch.close()

    def set_precond(self, precond):
        if precond == 'kron':
            raise ValueError('MultipatchVectorSystem has no %r preconditioner: \'jacobi\', \'schwarz\', \'mg\' or None' % (precond,))
        if precond == 'mg':
            if self.method != 'cg':
                raise ValueError("precond='mg' serves method='cg' only")
            self._live()
            if self._mg is None:
                raise ValueError("MultipatchVectorSystem: precond='mg' needs a hierarchy: call set_multigrid() first (it assembles "
                                 'every block again on every coarse level, so it is not done behind a solve)')
        _DeviceSystem.set_precond(self, precond)

    # -- geometric multigrid: what _MultipatchMultigrid asks of a system on blocked vectors
    _MG_COARSE, _MG_INVERSE = 'igx_solver_set_block_mg_coarse', 'igx_solver_set_block_mg_inverse'
    _MG_ORDER_KEY = 'nodes'

    def _refuse_multigrid(self):
        if self.method != 'cg' or not self.symmetric:
            raise ValueError("precond='mg' serves method='cg' on a symmetric form only")

    def _mg_fixed_sides(self, kvs, maps):
        """Per component its wholly fixed patch sides, which stay fixed on every level."""
        sides = []
        for c in range(self.ncomp):
            try:
                sides.append(fixed_sides(kvs, maps, self._component_fixed(c)))
            except ValueError as e:
                raise ValueError('component %d: %s' % (c, e)) from None
        return sides

    def _level_system(self, MPc, bcs):
        """The system of a coarse level of the hierarchy: the same form on `MPc` with a zero right-hand side."""
        problem, bfuns, args = self._problem
        return MultipatchVectorSystem(MPc, problem, 0.0, bcs, bfuns=bfuns, args=args, method='cg')

    def _component_fixed(self, c):
        """The fixed dofs of component `c` in the scalar numbering."""
        idx = self.bc_indices
        return idx[(idx >= c * self.N) & (idx < (c + 1) * self.N)] - c * self.N

    def _node_free(self):
        """Per node (scalar global dof): whether any of its components is free."""
        free = np.ones(self.n, dtype=bool)
        free[self.bc_indices] = False
        return free.reshape(self.ncomp, self.N).any(axis=0)

    def _set_smoother(self, smooth_steps):
        """Colours the nodes with a free component (first fit on the scalar pattern) and hands the colours to the device; returns
        this level's entry of ``mg_info``."""
        indptr, indices = self.MP.pattern()
        nodes = self._node_free()
        colour, ncol = first_fit_colouring(indptr, indices, nodes.astype(np.uint8))
        _lib.check(_lib.load().igx_solver_set_block_mg_smoother(self._live(), colour.ctypes.data_as(C.POINTER(C.c_int32)), int(smooth_steps)),
                   'igx_solver_set_block_mg_smoother')
        return dict(spans=[tuple(kv.numspans for kv in kvs) for kvs, _ in self.MP.patches], dofs=self.n,
                    free=int(self.n - self.bc_indices.size), nnz=int(indices.size) * sum(sum(row) for row in self.present),
                    colours=ncol, nodes=int(nodes.sum()))

    def set_multigrid(self, levels=None, coarse=None, smooth_steps=1, coarse_max=2048):
        """Sets up the hierarchy of ``precond='mg'``, as ``MultipatchSystem.set_multigrid`` does: a V-cycle with `smooth_steps`
        coloured node-block Gauss-Seidel sweeps before (forward) and after (backward) the coarse correction -- every node, a scalar
        dof with its ``nc`` components, solves its free components exactly from its ``nc x nc`` diagonal block --, the transfers
        of the scalar space applied per component, the coarsest level solved with a dense inverse.

        Every patch's knot vectors are coarsened with :func:`coarsen_knots` and the joins replayed, level after level, until there
        are `levels` of them (the finest included), a knot vector cannot be coarsened, or a level has at most `coarse_max` free
        dofs (blocked: all components); `coarse`: the coarser multipatches ``[MP1, MP2, ...]`` instead.  Every coarse level is a
        ``MultipatchVectorSystem`` of the same form with a zero right-hand side and the same patch sides fixed per component,
        assembled on the device (``nc^2`` blocks per patch and level: the set-up is an explicit call); the system owns the coarse
        levels and closes them with itself.  ValueError if the fixed dofs of a component are not a union of whole patch sides
        (the sides may differ between components), if a local-to-global map is not injective, with ``method='bicgstab'`` or a
        non-symmetric form, or if the coarsest level keeps more than `coarse_max` free dofs."""
        return self._build_multigrid(levels, coarse, smooth_steps, coarse_max)

    def schwarz_setup(self):
        """Per component ``(boxes, U, lam, mode)`` of the block-diagonal Schwarz preconditioner (host set-up): the boxes of
        ``schwarz_boxes`` on that component's fixed dofs and the stiffness factors of ``schwarz_factors`` (a floating patch of a
        component gets the ``sigma / d`` shift)."""
        MP = self.MP
        shapes = [tuple(kv.numdofs for kv in kvs) for kvs, _ in MP.patches]
        maps = [MP.patch_to_global_idx(p) for p in range(MP.numpatches)]
        kvs_list = [tuple(kvs) for kvs, _ in MP.patches]
        out = []
        for c in range(self.ncomp):
            boxes = schwarz_boxes(shapes, maps, self._component_fixed(c))
            U, lam, mode = schwarz_factors(kvs_list, boxes, 'stiffness')
            out.append((boxes, U, lam, mode))
        return out

    def _set_factors(self, h):
        lib = _lib.load()
        for c, (boxes, U, lam, mode) in enumerate(self.schwarz_setup()):
            _lib.check(lib.igx_solver_set_block_schwarz(h, c, *_schwarz_args(boxes, U, lam), mode), 'igx_solver_set_block_schwarz')
        _lib.check(lib.igx_solver_set_precond(h, _lib.IGX_PRECOND_SCHWARZ, None, None, None, None, 0), 'igx_solver_set_precond')
        self._factors_set = True

    def matrix(self):
        """The ``nc n x nc n`` matrix the system solves with (fixed rows and columns included), downloaded block by block from
        the solver: scipy CSR in the blocked layout.  An absent block has no entries; a present one keeps the whole pattern."""
        h = self._live()
        indptr, indices = self.MP.pattern()
        lib = _lib.load()
        N = self.N
        blocks = []
        for p in range(self.ncomp):
            row = []
            for q in range(self.ncomp):
                if not self.present[p][q]:
                    row.append(scipy.sparse.csr_matrix((N, N)))
                    continue
                data = np.empty(indices.shape[0])
                _lib.check(lib.igx_solver_download_multipatch_block(h, p, q, _lib.dptr(data)), 'igx_solver_download_multipatch_block')
                row.append(scipy.sparse.csr_matrix((data, indices.copy(), indptr.copy()), shape=(N, N)))
            blocks.append(row)
        return scipy.sparse.bmat(blocks, format='csr')

    def solve(self, tol=1e-8, maxiter=1000, precond='jacobi', x0=None, check_every=1, timed=False):
        """CG or BiCGStab (``method``) to ``||r|| <= tol * ||R (b - A ext(g))||``; returns the blocked global solution vector of
        ``nc * numdofs`` entries (the Dirichlet values included).  `precond`: 'jacobi' (the diagonals of the diagonal blocks),
        'schwarz' (per component the additive Schwarz preconditioner of ``MultipatchSystem``: one fast-diagonalization solve of
        the Laplacian per patch and component), 'mg' (CG only: one V-cycle of the hierarchy of ``set_multigrid()``, which must
        have been called -- ValueError otherwise; ``info`` then has ``levels`` and ``smooth_steps``) or None; 'kron' raises
        ValueError.  'mg' takes a few tens of iterations where Jacobi takes hundreds to thousands, each of them a V-cycle of a few
        hundred short launches."""
        u = self._solve(self.b, tol, maxiter, precond, x0, check_every, timed)
        self._mg_solve_info(precond)
        return u


################################################################################
# Parabolic problems of one patch on the device: DIRK time stepping
################################################################################

# Alexander (1977), three-stage SDIRK of order 3: gamma is the root in (1/6, 1/2) of 6 g^3 - 18 g^2 + 9 g - 1 = 0 (L-stability)
_SDIRK3_GAMMA = 0.43586652150845899942


def _tableau(name):
    if name == 'implicit_euler':
        return [[1.0],
                [1.0]]
    if name == 'crank_nicolson':
        return [[0.0, 0.0],
                [0.5, 0.5],
                [0.5, 0.5]]
    if name == 'sdirk3':
        g = _SDIRK3_GAMMA
        b2 = (6 * g * g - 20 * g + 5) / 4
        b1 = 1 - b2 - g
        return [[g, 0.0, 0.0],
                [(1 - g) / 2, g, 0.0],
                [b1, b2, g],
                [b1, b2, g]]
    if name == 'sdirk21':
        # Ellsiepen: two stages, order 2, alpha = 1 - 1/sqrt(2)
        a = 1 - math.sqrt(0.5)
        return [[a, 0.0],
                [1 - a, a],
                [1 - a, a]]
    if name == 'dirk34':
        # four stages, explicit first stage, gamma = 0.1558983899988677 (the coefficients the reference runs; see DESIGN.md
        # section 16: their weights sum to 1.0211)
        g = 0.1558983899988677
        a32, a42, a43 = 1.072486270734370, 0.7685298292769537, 0.09666483609791597
        return [[0.0, 0.0, 0.0, 0.0],
                [g, g, 0.0, 0.0],
                [1 - a32 - g, a32, g, 0.0],
                [0.0, a42, a43, g],
                [0.0, a42, a43, g]]
    if name == 'esdirk23':
        # Jorgensen, Kristensen, Thomsen (2018): three stages, order 2, gamma = 1 - 1/sqrt(2)
        g = 1 - math.sqrt(0.5)
        return [[0.0, 0.0, 0.0],
                [g, g, 0.0],
                [(1 - g) / 2, (1 - g) / 2, g],
                [(1 - g) / 2, (1 - g) / 2, g]]
    if name == 'esdirk34':
        # Jorgensen, Kristensen, Thomsen (2018): four stages, order 3, gamma the root of sdirk3
        g = _SDIRK3_GAMMA
        b = [0.10239940061991099768, -0.3768784522555561061, 0.83861253012718610911, g]
        return [[0.0, 0.0, 0.0, 0.0],
                [g, g, 0.0, 0.0],
                [0.14073777472470619619, -0.1083655513813208000, g, 0.0],
                b,
                b]
    return None


DIRK_SCHEMES = ('implicit_euler', 'crank_nicolson', 'sdirk3', 'sdirk21', 'dirk34', 'esdirk23', 'esdirk34')


ADAPTIVE_DIRK_SCHEMES = ('sdirk21', 'dirk34', 'esdirk23', 'esdirk34')
ROSENBROCK_SCHEMES = ('ros3p', 'ros3pw', 'rowdaind2', 'rodasp', 'rosi2p1')


def embedded_tableau(name):
    """``(A, err_order)`` of an embedded DIRK pair in the reference's layout: ``A`` of shape ``(s + 2, s)``, its first ``s + 1``
    rows the main rule of ``dirk_tableau(name)``, the last row the weights ``b_hat`` of the embedded rule; ``err_order`` the
    exponent of the step controller.  Schemes: ``ADAPTIVE_DIRK_SCHEMES``."""
    if name not in ADAPTIVE_DIRK_SCHEMES:
        raise ValueError('scheme %r has no embedded rule: one of %s' % (name, ', '.join(ADAPTIVE_DIRK_SCHEMES + ROSENBROCK_SCHEMES)))
    A = dirk_tableau(name)
    if name == 'sdirk21':
        ah = 2 - 5 / 4 * math.sqrt(2)
        b_hat, order = [1 - ah, ah], 1
    elif name == 'dirk34':
        b_hat, order = list(A[2]), 2                   # (the third stage row; its last weight is 0)
    elif name == 'esdirk23':
        g = A[1, 1]
        b_hat, order = [(6 * g - 1) / (12 * g), 1 / (12 * g * (1 - 2 * g)), (1 - 3 * g) / (3 * (1 - 2 * g))], 3
    else:
        b_hat, order = [0.15702489786032493710, 0.11733044137043884870, 0.61667803039212146434, 0.10896663037711474985], 4
    return np.vstack([A, b_hat]), order


def _rosenbrock(name):
    """(strict lower triangle of A, lower triangle of Gamma below the diagonal, gamma, b, b_hat, err_order), rows listed"""
    if name == 'ros3p':
        return ([[1.0], [1.0, 0.0]], [[-1.0], [-0.7886751347, -1.077350269]], 0.7886751347,
                [2 / 3, 0, 1 / 3], [1 / 3, 1 / 3, 1 / 3], 2)
    if name == 'ros3pw':
        return ([[1.5773502691896257e+00], [5.0000000000000000e-01, 0.0]],
                [[-1.5773502691896257e+00], [-6.7075317547305480e-01, -1.7075317547305482e-01]], 7.8867513459481287e-01,
                [1.0566243270259355e-01, 4.9038105676657971e-02, 8.4529946162074843e-01],
                [-1.7863279495408180e-01, 3.3333333333333333e-01, 8.4529946162074843e-01], 2)
    if name == 'rowdaind2':
        return ([[0.5], [0.28, 0.72], [0.28, 0.72, 0.0]],
                [[-1.121794871794876e-1], [2.54, -3.84], [29.0 / 75.0, -0.72, 1.0 / 30.0]], 0.3,
                [2.0 / 3.0, 0.0, 1.0 / 30.0, 0.3],
                [4.799002800355166e-1, 5.176203811215082e-1, 2.479338842975209e-3, 0.0], 2)
    if name == 'rosi2p1':
        return ([[5.0000000000000000e-1], [5.5729261836499822e-1, 1.9270738163500176e-1],
                 [-3.0084516445435860e-1, 1.8995581939026787e+0, -5.9871302944832006e-1]],
                [[-5.0000000000000000e-1], [-6.4492162993321323e-1, 6.3491801247597734e-2],
                 [9.3606009252719842e-3, -2.5462058718013519e-1, -3.2645441930944352e-1]], 4.3586652150845900e-1,
                [5.2900072579103834e-2, 1.3492662311920438e+0, -9.1013275270050265e-1, 5.0796644892935516e-1],
                [1.4974465479289098e-1, 7.0051069041421810e-1, 0.0, 1.4974465479289098e-1], 2)
    return None


def _lower(rows, s, diag=0.0):
    T = np.zeros((s, s))
    for i, row in enumerate(rows):
        T[i + 1, :len(row)] = row
    np.fill_diagonal(T, diag)
    return T


def rosenbrock_tableau(name):
    """``(A, Gamma, b, b_hat, err_order)`` of a Rosenbrock method as the reference runs it: ``A`` strictly lower triangular,
    ``Gamma`` lower triangular with the constant diagonal ``gamma``, the weights ``b`` and those of the embedded rule ``b_hat``.
    Schemes: ``ROSENBROCK_SCHEMES`` (Lang and Teleaga; RODASP of Steinebach).  For an affine right-hand side stage 2 of
    ``ros3p`` and ``ros3pw`` equals stage 1 and their estimate vanishes."""
    if name == 'rodasp':
        # given through B = A + Gamma, as in the literature
        gamma = 0.25
        A = _lower([[0.75], [8.6120400814152190E-2, 0.1238795991858478],
                    [0.7749345355073236, 0.1492651549508680, -0.2941996904581916],
                    [5.308746682646142, 1.330892140037269, -5.374137811655562, -0.2655010110278497],
                    [-1.764437648774483, -0.4747565572063027, 2.369691846915802, 0.6195023590649829, 0.25]], 6)
        b5 = [-1.764437648774483, -0.4747565572063027, 2.369691846915802, 0.6195023590649829]
        b6 = [-8.0368370789113464E-2, -5.6490613592447572E-2, 0.4882856300427991, 0.5057162114816189, -0.1071428571428569]
        B = _lower([[0.0], [-0.049392, -0.014112], [-0.4820494693877561, -0.1008795555555556, 0.9267290249433117], b5, b6], 6, gamma)
        return A, B - A, np.array(b6 + [gamma]), np.array(b5 + [gamma, 0.0]), 3
    t = _rosenbrock(name) if isinstance(name, str) else None
    if t is None:
        raise ValueError('unknown Rosenbrock scheme %r: one of %s' % (name, ', '.join(ROSENBROCK_SCHEMES)))
    a, g, gamma, b, b_hat, order = t
    s = len(b)
    return _lower(a, s), _lower(g, s, gamma), np.array(b, dtype=np.float64), np.array(b_hat, dtype=np.float64), order


def _stepper(scheme, need_estimate):
    """The scheme of a stepping session: dict(family, name, stages, A, Gamma, b, b_hat, err_order, gamma).  `scheme`: a name of
    DIRK_SCHEMES or ROSENBROCK_SCHEMES.  ValueError for an unknown name (as dirk_tableau) or, with `need_estimate`, for a scheme
    without an embedded rule."""
    if isinstance(scheme, str) and scheme in ROSENBROCK_SCHEMES:
        A, G, b, b_hat, order = rosenbrock_tableau(scheme)
        return dict(family=_lib.IGX_STEPPER_ROSENBROCK, name=scheme, stages=len(b), A=np.ascontiguousarray(A),
                    Gamma=np.ascontiguousarray(G), b=b, b_hat=b_hat, err_order=order, gamma=float(G[0, 0]))
    name, A, gamma = _scheme(scheme)
    if name in ADAPTIVE_DIRK_SCHEMES:
        E, order = embedded_tableau(name)
        b_hat = np.ascontiguousarray(E[-1])
    elif need_estimate:
        raise ValueError('scheme %r has no embedded rule to choose the step by (tol given): one of %s'
                         % (scheme if name is None else name, ', '.join(ADAPTIVE_DIRK_SCHEMES + ROSENBROCK_SCHEMES)))
    else:
        b_hat, order = None, None
    return dict(family=_lib.IGX_STEPPER_DIRK, name=name, stages=A.shape[1], A=np.ascontiguousarray(A), Gamma=None,
                b=np.ascontiguousarray(A[-1]), b_hat=b_hat, err_order=order, gamma=gamma)


def next_step(tau, r, converged, step_factor, err_order):
    """The reference's step controller (pyiga/solvers.py:505-531): ``(accepted, next tau)`` after an attempt with step `tau` whose
    error ratio is `r`.  ``r == 0`` counts as 1e-15; accepted iff ``r <= 1``; the step changes by
    ``min(5, max(0.2, step_factor r^(-1/err_order)))`` whether accepted or not.  An attempt whose solves did not converge is
    rejected and halves the step."""
    if not converged:
        return False, tau * 0.5
    if r == 0:
        r = 1e-15
    fac = step_factor * r ** (-1 / err_order)
    fac = min(5.0, max(0.2, fac))
    return bool(r <= 1), tau * fac


def dirk_tableau(name):
    """The tableau ``A`` of the named DIRK scheme in the reference's layout: shape ``(s + 1, s)``, the last row ``b`` (main rules:
    no embedded ``b_hat`` row).  Schemes: ``DIRK_SCHEMES``."""
    t = _tableau(name) if isinstance(name, str) else None
    if t is None:
        raise ValueError('unknown DIRK scheme %r: one of %s' % (name, ', '.join(DIRK_SCHEMES)))
    return np.array(t, dtype=np.float64)


def check_tableau(A):
    """``(A, gamma)`` for a tableau every implicit stage of which solves with one matrix ``M + tau gamma K``: shape ``(s + 1, s)``,
    ``1 <= s <= 6``, lower triangular, every nonzero diagonal entry one ``gamma > 0``, a zero diagonal only in row 0 (an explicit
    first stage), stiffly accurate (``b`` equals the last stage row).  ValueError otherwise (what ``igx_solver_set_dirk``
    refuses)."""
    A = np.array(A, dtype=np.float64)
    if A.ndim != 2 or A.shape[0] != A.shape[1] + 1 or not 1 <= A.shape[1] <= _lib.IGX_DIRK_MAX_STAGES:
        raise ValueError('a DIRK tableau has shape (s + 1, s) with 1 <= s <= %d, not %s' % (_lib.IGX_DIRK_MAX_STAGES, A.shape))
    s = A.shape[1]
    if not np.all(np.isfinite(A)):
        raise ValueError('the DIRK tableau has non-finite entries')
    if np.any(np.triu(A[:s], 1) != 0):
        raise ValueError('the DIRK tableau is not lower triangular')
    diag = np.diag(A[:s])
    if np.any(diag[1:] == 0):
        raise ValueError('the DIRK tableau has a zero diagonal past the first stage (only the first stage may be explicit)')
    nz = diag[diag != 0]
    if nz.size == 0 or np.any(nz <= 0):
        raise ValueError('the diagonal of the DIRK tableau must be positive (gamma > 0)')
    if np.any(nz != nz[0]):
        raise ValueError('the DIRK tableau has two diagonal values (%r): every stage must solve with one matrix' % (sorted(set(nz)),))
    if np.any(A[s] != A[s - 1]):
        raise ValueError('the DIRK tableau is not stiffly accurate (b differs from the last stage row); such schemes need a mass '
                         'solve per step and are not supported')
    return A, float(nz[0])


def _scheme(scheme):
    """(name or None, A, gamma) of a scheme name or tableau (ValueError as check_tableau)."""
    if isinstance(scheme, str):
        A, gamma = check_tableau(dirk_tableau(scheme))
        return scheme, A, gamma
    A, gamma = check_tableau(scheme)
    return None, A, gamma


def _form_kind(problem):
    """The device kind of `problem` as far as it is known before any device work (None: the built-in stiffness form)."""
    from . import assemble
    if problem is None:
        return 'stiffness'
    if isinstance(problem, str):
        return assemble._KNOWN_FORMS.get(assemble._normalise_form(problem)) or 'form'
    cls = problem if isinstance(problem, type) else type(problem)
    return getattr(cls, '_kind', None)


def _check_times(name, tau, t0, t_end, save_every):
    """``(tau, t0, t_end, save_every)`` of an integration as three floats and an int, or ValueError (`name`: what the caller
    calls its step)."""
    tau, t0, t_end = float(tau), float(t0), float(t_end)
    if not (tau > 0 and math.isfinite(tau)):
        raise ValueError('%s must be positive and finite, not %r' % (name, tau))
    if not t_end > t0:
        raise ValueError('t_end (%r) must be greater than t0 (%r)' % (t_end, t0))
    save_every = int(save_every)
    if save_every < 1:
        raise ValueError('save_every must be >= 1')
    return tau, t0, t_end, save_every


class ParabolicSystem(_PatchErrorNorms, _DeviceSystem):
    """The parabolic problem ``M u' = f - K u`` on the free dofs, ``u = g`` on the dofs of `bcs`, ``u(t0) = u0``, of one patch,
    integrated on the device by a DIRK scheme with constant steps (the reference's ``crank_nicolson``, ``sdirk3``, ``esdirk34``,
    ... on ``RestrictedLinearSystem`` matrices, pyiga/solvers.py:366-473).

    M is the mass matrix of the patch; K the stiffness matrix (`problem` None: the heat equation) or the matrix of any form that
    ``FormSystem`` accepts (`problem`, with `args` / `kwargs` its inputs); f and g do not depend on time.  Both matrices are
    assembled on the device and handed to the solver (``igx_solver_take_values``); ``C = M + tau gamma K`` is formed there.
    `rhs`: the load vector, a scalar, a function of the physical coordinates (``inner_products``) or a linear form string.
    `bcs`: ``(indices, values)`` as ``compute_dirichlet_bcs`` gives them, or None (pure Neumann).  `method`: 'auto' is CG for the
    built-in stiffness (and mass) form, else BiCGStab; 'cg' on any other form raises ValueError before any assembly.
    `boundary_terms`: ``BoundaryTerm`` objects (time-independent): their face matrices are added to K on the device before the
    solver takes it (convective cooling: ``K + R``), their face loads to f; M is untouched.

    ``integrate(...)`` returns ``(times, solutions)``; ``spmv(x)`` is ``R C R^T x`` and ``apply_precond(r)`` the preconditioner
    of C, for the scheme and step of ``set_scheme`` (or the last ``integrate``).
    """

    def __init__(self, kvs, geo, rhs, bcs=None, problem=None, args=None, method='auto', device=None, boundary_terms=None, **kwargs):
        from . import assemble
        if method != 'auto':
            _check_method(method)
        args = dict(args or {})
        args.update(kwargs)
        if geo is not None:
            args.setdefault('geo', geo)
        self.kvs = tuple(kvs)
        self.geo = geo
        if problem is not None:
            _check_device_form(problem, self.kvs, args)
        kind = _form_kind(problem)
        self.symmetric = kind in ('mass', 'stiffness')
        # boundary terms: K + R is the operator, the face loads join f; the mass matrix is untouched
        terms = _bt.check_terms(boundary_terms, len(self.kvs), method=None if method == 'auto' else method, who='ParabolicSystem')
        self._terms = _bt.PatchTerms(self.kvs, args.get('geo'), terms, method=None if method == 'auto' else method,
                                     who='ParabolicSystem') if terms else None
        if self._terms is not None and not self._terms.symmetric():
            self.symmetric = False                               # ('auto' then takes BiCGStab)
        if method == 'auto':
            method = 'cg' if self.symmetric else 'bicgstab'
        elif method == 'cg' and not self.symmetric:
            raise ValueError("ParabolicSystem: CG needs M + tau gamma K symmetric positive definite; %r is not known to be "
                             "symmetric: method='bicgstab'" % (problem,))
        self.ndofs = tuple(kv.numdofs for kv in self.kvs)
        self.n = int(np.prod(self.ndofs))
        if problem is None:
            self.patch = assemblers.DevicePatch(self.kvs, geo, device=device)
            self._own_patch = True
        else:
            self.assembler = assemble.instantiate_assembler(problem, self.kvs, args)
            self._own_patch = self.assembler is not problem
            self.patch = self.assembler.patch
            kind = self.assembler._kind
        self.kind = kind
        if isinstance(rhs, str):
            rhs = assemble.assemble(rhs, self.kvs, args=args)
        elif callable(rhs):
            rhs = assemble.inner_products(self.kvs, rhs, f_physical=True, geo=geo)
        elif np.ndim(rhs) == 0:
            rhs = np.full(self.n, float(rhs))
        self.b = np.ascontiguousarray(rhs, dtype=np.float64).ravel()
        if self.b.size != self.n:
            raise ValueError('right-hand side has %d entries, the space %d' % (self.b.size, self.n))
        if self._terms is not None and self._terms.has_rhs:
            self.b = self._terms.add_loads(self.b.copy())
        self._ctx = self.patch.ctx
        self._attach('igx_solver_create_parabolic', (self.patch.handle, _lib.KINDS[self.kind], 1 if self.symmetric else 0), bcs,
                     method, 'cg' if self.symmetric else 'bicgstab')
        self.box = dirichlet_box(self.ndofs, self.bc_indices)
        lib = _lib.load()
        self.patch.assemble(self.kind, to_host=False)            # the values stay on the device and change hands
        if self._terms is not None:                              # K + R: added before the solver takes the values
            try:
                self._terms.add_matrices(self.patch.add_face)
            finally:
                self._terms.close()
        _lib.check(lib.igx_solver_take_values(self.handle, _lib.IGX_ROLE_OPERATOR), 'igx_solver_take_values')
        self.patch.assemble('mass', to_host=False)
        _lib.check(lib.igx_solver_take_values(self.handle, _lib.IGX_ROLE_MASS), 'igx_solver_take_values')
        self._step = None                                        # (tau, tableau) of the C on the device
        self._eig = None
        self._step_precond = None                                # the preconditioner of the stepping session on the device

    @property
    def default_precond(self):
        return 'kron' if self.box is not None else 'jacobi'

    def set_scheme(self, scheme, tau):
        """Validates `scheme` (a name of ``DIRK_SCHEMES`` or a tableau) and `tau`, and forms ``C = M + tau gamma K`` on the device
        (once per step and tableau).  Returns the tableau."""
        _, A, gamma = _scheme(scheme)
        tau = float(tau)
        if not (tau > 0 and math.isfinite(tau)):
            raise ValueError('tau must be positive and finite, not %r' % (tau,))
        key = (tau, A.tobytes())
        if key != self._step:
            _lib.check(_lib.load().igx_solver_set_dirk(self._live(), A.shape[1], _lib.dptr(A), tau), 'igx_solver_set_dirk')
            self._step = key
            self._precond = None                                 # (the device reset it: Jacobi and Kronecker depend on C)
            self.tau, self.gamma = tau, gamma
        return A

    def kron_factors(self):
        """Per axis ``U_k`` and ``lam'_k = tau gamma lam_k + 1/d`` from ``eigh(K_k, M_k)`` on the free box: with
        ``IGX_KRON_SUM`` the fast-diagonalization inverse of the parametric ``M + tau gamma K`` (exact on the identity map of the
        unit square or cube; symmetric positive definite without any Dirichlet dof)."""
        if self.box is None:
            raise ValueError("precond='kron' needs the Dirichlet dofs to be a union of whole sides of the patch (or none)")
        if self._step is None:
            raise ValueError('no step yet: set_scheme(scheme, tau) or integrate(...) first')
        if self._eig is None:
            self._eig = fastdiag_factors(self.kvs, self.box[0], self.box[1], True)[:2]
        U, lam = self._eig
        d = len(self.kvs)
        return U, [self.tau * self.gamma * l + 1.0 / d for l in lam]

    def _set_factors(self, h):
        U, lam = self.kron_factors()
        lo, hi, Up, Lp = _box_args(self.box[0], self.box[1], U, lam)
        _lib.check(_lib.load().igx_solver_set_precond(h, _lib.IGX_PRECOND_KRON, lo, hi, Up, Lp, _lib.IGX_KRON_SUM),
                   'igx_solver_set_precond')

    def set_precond(self, precond):
        key = precond if precond is not None else 'none'
        if key in self.PRECONDS and key != self._precond:
            self._step_precond = None                            # (igx_solver_set_precond replaces the session's factors)
        _DeviceSystem.set_precond(self, precond)

    def integrate(self, u0, tau, t_end, scheme='sdirk3', t0=0.0, tol=1e-10, maxiter=1000, precond='auto', save_every=1,
                  check_every=1, timed=False):
        """``ceil((t_end - t0) / tau)`` steps of `scheme` (a name of ``DIRK_SCHEMES`` or a tableau) from `u0` (a vector, or a
        function of the physical coordinates: its L2 projection; its fixed entries are replaced by g).  Every stage solve runs
        to ``||r|| <= tol ||R (b_i - C ext(g))||`` with `precond` ('auto': 'kron' when the Dirichlet dofs are whole sides or
        absent, else 'jacobi'; 'kron', 'jacobi' or None).

        Returns ``(times, solutions)`` as the reference's constant-step methods: ``times[k] = t0 + k tau`` of the states kept
        (every `save_every`-th step and always the last; the last time may pass `t_end`), ``solutions`` the full vectors
        (Dirichlet values included), ``solutions[0] = u0``.  A stage solve that does not converge within `maxiter` iterations
        ends the integration: the states up to the last completed step are returned (a RuntimeWarning says so, and
        ``info['converged']`` is False).  ``info``: the fields of ``igx_dirk_info`` and the iterations of every stage.

        A name of ``ROSENBROCK_SCHEMES`` runs the constant-step Rosenbrock method (``integrate_adaptive`` with ``tol=None``)."""
        if isinstance(scheme, str) and scheme in ROSENBROCK_SCHEMES:
            return self.integrate_adaptive(u0, tau, t_end, None, scheme=scheme, t0=t0, solve_tol=tol, maxiter=maxiter,
                                           precond=precond, save_every=save_every, check_every=check_every, timed=timed)
        name, A, gamma = _scheme(scheme)
        tau, t0, t_end, save_every = _check_times('tau', tau, t0, t_end, save_every)
        key = self._check_precond(precond)
        nsteps = int(math.ceil((t_end - t0) / tau))
        h = self._live()
        x0 = self._start_vector(u0)
        self.set_scheme(A, tau)
        self.set_precond(key)
        s = A.shape[1]
        plan = [k for k in range(1, nsteps + 1) if k % save_every == 0 or k == nsteps]
        saved = np.empty((len(plan), self.n))
        iters = np.zeros((nsteps, s), dtype=np.int32)
        info = _lib.DirkInfo()
        _lib.check(_lib.load().igx_solver_dirk_run(h, _lib.dptr(self.b), _lib.dptr(self.bc_values), _lib.dptr(x0), nsteps,
                                                   save_every, float(tol), int(maxiter), int(check_every), 1 if timed else 0,
                                                   _lib.dptr(saved), iters.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(info)),
                   'igx_solver_dirk_run')
        steps, converged = int(info.steps), bool(info.converged)
        kept = [k for k in plan if k <= steps]
        if not converged and steps > 0 and (not kept or kept[-1] != steps):
            kept.append(steps)
        assert len(kept) == info.nsaved, (kept, info.nsaved)
        implicit = [i for i in range(s) if A[i, i] != 0]
        rows = iters[:steps + (0 if converged else 1), implicit]
        reason = _lib.load().igx_solver_last_breakdown(h)
        self.info = dict(info.as_dict(), converged=converged, nsteps=nsteps, scheme=name, tau=tau, gamma=gamma,
                         stage_iterations=rows, step_iterations=rows.sum(axis=1), precond=self._precond, method=self.method,
                         breakdown=_lib.BREAKDOWNS.get(reason, reason))
        if not converged:
            warnings.warn('ParabolicSystem.integrate: a stage solve of step %d did not converge within %d iterations; returning '
                          'the %d steps completed' % (steps + 1, maxiter, steps), RuntimeWarning, stacklevel=2)
        return [t0] + [t0 + k * tau for k in kept], [x0] + [saved[j] for j in range(len(kept))]

    def _check_precond(self, precond):
        key = self.default_precond if precond == 'auto' else precond
        if (key if key is not None else 'none') not in self.PRECONDS:
            raise ValueError('unknown preconditioner %r' % (precond,))
        if key == 'kron' and self.box is None:
            raise ValueError("precond='kron' needs the Dirichlet dofs to be a union of whole sides of the patch (or none)")
        return key if key is not None else 'none'

    def _start_vector(self, u0):
        """`u0` (a vector, or a function of the physical coordinates: its L2 projection) as a full vector of its own with g on
        the fixed dofs."""
        if callable(u0):
            from . import approx
            u0 = approx.project_L2(self.kvs, u0, f_physical=True, geo=self.geo)
        x0 = np.array(u0, dtype=np.float64).ravel()
        if x0.size != self.n:
            raise ValueError('u0 has %d entries, the space %d' % (x0.size, self.n))
        x0[self.bc_indices] = self.bc_values
        return x0

    def _set_step_precond(self, h, key):
        """The session's preconditioner: for 'kron' the factors U_k and the RAW eigenvalues go up once; the device rescales
        them per step and for the mass solve."""
        if self._step_precond == key:
            return
        lib = _lib.load()
        if key == 'kron':
            if self._eig is None:
                self._eig = fastdiag_factors(self.kvs, self.box[0], self.box[1], True)[:2]
            U, lam = self._eig
            lo, hi, Up, Lp = _box_args(self.box[0], self.box[1], U, lam)
            _lib.check(lib.igx_solver_set_step_precond(h, _lib.IGX_PRECOND_KRON, lo, hi, Up, Lp), 'igx_solver_set_step_precond')
        else:
            _lib.check(lib.igx_solver_set_step_precond(h, self.PRECONDS[key], None, None, None, None), 'igx_solver_set_step_precond')
        self._step_precond = key

    def begin_steps(self, u0, scheme, precond='auto', need_estimate=True):
        """Starts a stepping session (``igx_solver_set_stepper``, ``igx_solver_set_step_precond``, ``igx_solver_step_begin``) from
        `u0` with the scheme `scheme`; returns ``(stepper, x0)``.  ``attempt_step`` / ``accept_step`` / ``step_state`` then run
        it; ``integrate_adaptive`` is the driver built on them."""
        st = _stepper(scheme, need_estimate)
        key = self._check_precond(precond)
        h = self._live()
        x0 = self._start_vector(u0)
        lib = _lib.load()
        # the session forms its own C and preconditioner data: what set_scheme / set_precond left is void after it
        self._step = None
        self._precond = None
        opt = lambda a: None if a is None else _lib.dptr(a)
        _lib.check(lib.igx_solver_set_stepper(h, st['family'], st['stages'], _lib.dptr(st['A']), opt(st['Gamma']),
                                              _lib.dptr(st['b']), opt(st['b_hat'])), 'igx_solver_set_stepper')
        self._set_step_precond(h, key)
        _lib.check(lib.igx_solver_step_begin(h, _lib.dptr(self.b), _lib.dptr(self.bc_values), _lib.dptr(x0)), 'igx_solver_step_begin')
        return st, x0

    def attempt_step(self, tau, err_tol=0.0, solve_tol=1e-10, maxiter=1000, check_every=1, timed=False):
        """One attempt of the session with the step `tau` (``igx_solver_step_attempt``); returns the ``StepInfo``."""
        info = _lib.StepInfo()
        _lib.check(_lib.load().igx_solver_step_attempt(self._live(), float(tau), float(err_tol), float(solve_tol), int(maxiter),
                                                       int(check_every), 1 if timed else 0, C.byref(info)), 'igx_solver_step_attempt')
        return info

    def accept_step(self):
        _lib.check(_lib.load().igx_solver_step_accept(self._live()), 'igx_solver_step_accept')

    def step_state(self, candidate=False):
        """The state of the session, or the candidate of the last attempt, as a full vector."""
        out = np.empty(self.n)
        _lib.check(_lib.load().igx_solver_step_state(self._live(), _lib.IGX_STEP_CANDIDATE if candidate else _lib.IGX_STEP_STATE,
                                                     _lib.dptr(out)), 'igx_solver_step_state')
        return out

    def error_ratio(self, vectors, coef, x, tol, offset=0):
        """``|| (sum_k coef[k] vectors[k]) / (tol + tol |x|) ||_2 / sqrt(n_free)`` over the free dofs by ``k_err_norm`` alone
        (``igx_solver_error_ratio_d``; at most ``_lib.COMB_MAX`` vectors).  `offset`: every vector starts that many doubles into
        its device buffer (an odd number: no 16-byte alignment, the kernel's scalar path)."""
        coef = np.ascontiguousarray(coef, dtype=np.float64).ravel()
        if not 1 <= len(vectors) <= _lib.COMB_MAX or coef.size != len(vectors):
            raise ValueError('1 to %d vectors and as many coefficients' % _lib.COMB_MAX)
        h = self._live()
        offset = int(offset)
        host = [np.asarray(v, dtype=np.float64).ravel() for v in list(vectors) + [x]]
        if offset < 0 or any(v.size != self.n for v in host):
            raise ValueError('vectors of the wrong size')
        dev = [DeviceArray.from_host(self._ctx, np.concatenate([np.zeros(offset), v])) for v in host]
        at = [d.ptr + 8 * offset for d in dev]
        ptrs = (C.c_void_p * len(vectors))(*at[:-1])
        r = C.c_double()
        _lib.check(_lib.load().igx_solver_error_ratio_d(h, len(vectors), _lib.dptr(coef), ptrs, at[-1], float(tol),
                                                        C.byref(r)), 'igx_solver_error_ratio_d')
        return r.value

    def integrate_adaptive(self, u0, tau0, t_end, tol, scheme='esdirk23', t0=0.0, step_factor=0.9, solve_tol=1e-10, maxiter=1000,
                           precond='auto', save_every=1, max_attempts=10000, check_every=1, timed=False):
        """Integrates from `t0` until ``t >= t_end`` with steps chosen by the embedded rule of `scheme` (a name of
        ``ADAPTIVE_DIRK_SCHEMES`` or ``ROSENBROCK_SCHEMES``), as the reference's adaptive methods (pyiga/solvers.py:475-534): with
        ``d = tol + tol |x|`` and ``r = ||(x_est - x_new) / d||_2 / sqrt(n_free)`` an attempt is accepted iff ``r <= 1`` and the
        step changes by ``min(5, max(0.2, step_factor r^(-1/err_order)))`` after every attempt (``next_step``); an attempt one of
        whose solves does not converge within `maxiter` iterations is rejected and halves the step.  The last step may pass
        `t_end`.  ``tol=None``: constant steps of `tau0` (any name of ``DIRK_SCHEMES`` or ``ROSENBROCK_SCHEMES``).

        Every solve runs to ``||r|| <= solve_tol ||r0||``, ``r0`` the residual of its start value.  That is the right-hand side
        but for the DIRK stages, which start from the previous stage: they are solved for their increment (as the reference's
        Newton measures its ``rtol``), also with ``tol=None``, where ``integrate`` with the same scheme stops relative to the
        right-hand side.

        Returns ``(times, solutions)`` of the accepted steps kept (every `save_every`-th and always the last; ``solutions[0] =
        u0``).  At most `max_attempts` attempts are made: when they run out (or a constant step does not converge) the states so
        far are returned, a RuntimeWarning says so and ``info['converged']`` is False.  ``info``: per attempt ``tau``, ``r``,
        ``accepted``, ``stage_iterations``, ``mass_iterations``; the counts ``attempts``, ``rejections``, ``reformations``; the
        phase times (ms, summed; all but ``total_ms`` and ``axpby_ms`` need `timed`)."""
        tau0, t0, t_end, save_every = _check_times('tau0', tau0, t0, t_end, save_every)
        if tol is not None and not tol > 0:
            raise ValueError('tol must be positive (or None for constant steps), not %r' % (tol,))
        if not 0 < step_factor <= 1:
            raise ValueError('step_factor must lie in (0, 1], not %r' % (step_factor,))
        max_attempts = int(max_attempts)
        if max_attempts < 1:
            raise ValueError('max_attempts must be >= 1')
        st, x0 = self.begin_steps(u0, scheme, precond, need_estimate=tol is not None)
        times, sols = [t0], [x0]
        log = dict(tau=[], r=[], accepted=[], stage_iterations=[], mass_iterations=[])
        phases = dict.fromkeys(('axpby_ms', 'spmv_ms', 'combine_ms', 'solve_ms', 'mass_ms', 'err_ms', 'total_ms'), 0.0)
        reformations = accepted = 0
        last_kept = True
        nsteps = int(math.ceil((t_end - t0) / tau0)) if tol is None else None
        t, tau, converged, failed = t0, tau0, True, None
        while (accepted < nsteps) if tol is None else (t < t_end):
            if tol is not None and len(log['tau']) >= max_attempts:
                converged, failed = False, 'the %d attempts allowed ran out at t = %g' % (max_attempts, t)
                break
            info = self.attempt_step(tau, 0.0 if tol is None else tol, solve_tol, maxiter, check_every, timed)
            for k in phases:
                phases[k] += getattr(info, k)
            reformations += info.reformed
            ok = bool(info.converged)
            if tol is None:
                accept, tau_next, r = ok, tau, 0.0
            else:
                r = info.r if ok else float('nan')
                accept, tau_next = next_step(tau, info.r, ok, step_factor, st['err_order'])
            log['tau'].append(tau)
            log['r'].append(r)
            log['accepted'].append(accept)
            log['stage_iterations'].append(list(info.stage_iterations)[:st['stages']])
            log['mass_iterations'].append(info.mass_iterations)
            if tol is None and not ok:
                converged, failed = False, 'a solve of step %d did not converge within %d iterations' % (accepted + 1, maxiter)
                break
            if accept:
                self.accept_step()
                accepted += 1
                t = t0 + accepted * tau0 if tol is None else t + tau
                last_kept = accepted % save_every == 0
                if last_kept:
                    times.append(t)
                    sols.append(self.step_state())
            tau = tau_next
        if not last_kept:
            times.append(t)
            sols.append(self.step_state())
        reason = _lib.load().igx_solver_last_breakdown(self.handle)
        self.info = dict(phases, converged=converged, scheme=st['name'], gamma=st['gamma'], tol=tol, attempts=len(log['tau']),
                         rejections=len(log['tau']) - accepted, accepted_steps=accepted, reformations=reformations,
                         tau=np.array(log['tau']), r=np.array(log['r']), accepted=np.array(log['accepted'], dtype=bool),
                         stage_iterations=np.array(log['stage_iterations'], dtype=np.int32).reshape(-1, st['stages']),
                         mass_iterations=np.array(log['mass_iterations'], dtype=np.int32), precond=self._step_precond,
                         method=self.method, breakdown=_lib.BREAKDOWNS.get(reason, reason))
        if not converged:
            warnings.warn('ParabolicSystem.integrate_adaptive: %s; returning the %d steps completed' % (failed, accepted),
                          RuntimeWarning, stacklevel=2)
        return times, sols


################################################################################
# Nonlinear Dirichlet problems of one patch on the device: Newton's method
################################################################################

class NoConvergenceError(Exception):
    """An iteration stopped after its maximum number of steps (pyiga/solvers.py:329-333)."""

    def __init__(self, method, num_iter, last_iterate):
        super().__init__('%s: no convergence after %d iterations' % (method, num_iter))
        self.method = method
        self.num_iter = num_iter
        self.last_iterate = last_iterate


def newton_loop(residual_norm, form_jacobian, update, atol, rtol, maxiter, freeze_jac):
    """The bookkeeping of Newton's method as the reference does it (pyiga/solvers.py:335-361), on callbacks that act on the
    current iterate wherever it lives: ``residual_norm()`` evaluates F there and returns ``||R F||``, ``form_jacobian()`` forms J
    there, ``update()`` does ``x -= J^-1 F`` with the J formed last and returns the inner iterations.  The target is
    ``max(atol, rtol ||R F(x0)||)``, tested (``<``) before each step; J is formed again every `freeze_jac` steps.  Returns
    ``(converged, info)``, info = Newton steps, the residual norm before every step (and after the last), the inner iterations
    per step and the number of Jacobians formed."""
    if freeze_jac < 1:
        raise ValueError('freeze_jac must be at least 1')
    norms, inner, jacobians = [residual_norm()], [], 0
    target = max(atol, rtol * norms[0])
    converged = False
    for it in range(maxiter):
        if norms[-1] < target:
            converged = True
            break
        if it % freeze_jac == 0:
            form_jacobian()
            jacobians += 1
        inner.append(update())
        norms.append(residual_norm())
    return converged, dict(iterations=len(inner), residual_norms=norms, inner_iterations=inner, jacobians=jacobians, target=target)


def _symmetric_traced_table(table):
    """The test VectorFormSystem applies to sampled tables (symmetric_block_tables), on a traced one: entry (r, s) and entry
    (s, r) are the same expression text, a None only opposite a None."""
    n = len(table)
    return all(table[r][s] == table[s][r] for r in range(n) for s in range(n))


class NewtonSystem(PatchSystem):
    """The nonlinear Dirichlet problem ``F(x) = 0``, ``x = g`` on the dofs of `bcs`, on one patch, by Newton's method with the
    iterate, the residual and the Jacobian in device memory (the reference's idiom: ``F(x) = Assembler(residual,
    updatable=[unknown]).assemble(w=BSplineFunc(kvs, x))``, J likewise, ``RestrictedLinearSystem``, ``solvers.newton``).

    `residual`: an arity-1 form string in ``v`` and the unknown; `jacobian`: an arity-2 form string in ``u``, ``v`` and the
    unknown (named `unknown`, a scalar spline function of the patch's space: its value, and ``grad(unknown)``); other inputs as
    for ``assemble.assemble``.  The linear solves are CG when the traced coefficient table of the Jacobian is symmetric, else
    BiCGStab (`method`: 'auto', 'cg', 'bicgstab').  Residual and Jacobian run on two patches of the same space: the solver reads
    the Jacobian's patch, whose form is never anything but the Jacobian's.  Needs the run-time compiler (no host fallback)."""

    def __init__(self, kvs, geo, residual, jacobian, bcs, unknown='w', args=None, method='auto', **inputs):
        from . import bspline, forms
        inputs = dict(args or {}, **inputs)
        inputs.pop('geo', None)
        self.kvs = tuple(kvs)
        self.unknown = unknown
        d = len(self.kvs)
        if forms.arity(residual) != 1 or forms.arity(jacobian) != 2:
            raise ValueError('NewtonSystem: the residual is a linear functional in v, the Jacobian a bilinear form in u and v')
        if method not in ('auto', 'cg', 'bicgstab'):
            raise ValueError("unknown method %r: 'auto', 'cg' or 'bicgstab'" % (method,))
        self.ndofs = tuple(kv.numdofs for kv in self.kvs)
        self.n = int(np.prod(self.ndofs))
        w0 = bspline.BSplineFunc(self.kvs, np.zeros(self.ndofs))
        full = dict(inputs, geo=geo)
        full[unknown] = w0
        cls2 = assemblers.GeneralFormAssembler2D if d == 2 else assemblers.GeneralFormAssembler3D
        cls1 = assemblers.GeneralFunctionalAssembler2D if d == 2 else assemblers.GeneralFunctionalAssembler3D
        from .assemble import _check_spline_inputs
        _check_spline_inputs(residual, self.kvs, full, None, None, False)
        _check_spline_inputs(jacobian, self.kvs, full, None, None, False)
        self.patch = self.jac = self.res = self.d_x = None
        try:
            self.jac = cls2(self.kvs, geo, jacobian, inputs=full)
            self.assembler, self.patch, self.kind = self.jac, self.jac.patch, 'form'
            self.res = cls1(self.kvs, geo, residual, inputs=full, fields=self.jac.fields)
            self._want_grad = self.jac._slots.wants_gradient(unknown) or self.res._slots.wants_gradient(unknown)
            self.symmetric = _symmetric_traced_table(self.jac._exprs)
            if method == 'auto':
                method = 'cg' if self.symmetric else 'bicgstab'
            self._ctx = self.patch.ctx
            self.d_x = DeviceArray(self._ctx, self.n)
            self.patch.assemble('form', to_host=False)                # J(0): the solver is made over values of its kind
            self.b = np.zeros(self.n)
            self._attach('igx_solver_create_general', (self.patch.handle, _lib.KINDS['form']), bcs, 'bicgstab', 'bicgstab')
            if self.symmetric:
                _lib.check(_lib.load().igx_solver_declare_symmetric(self.handle), 'igx_solver_declare_symmetric')
            self.set_method(method)
        except BaseException:
            self._release()
            self._drop_owner()                                    # (nothing of a failed construction stays on the device)
            raise
        self.box = dirichlet_box(self.ndofs, self.bc_indices)

    def _drop_owner(self):
        for name in ('jac', 'res'):
            a = getattr(self, name, None)
            if a is not None and getattr(a, 'patch', None) is not None:
                a.patch.close()
            setattr(self, name, None)
        if getattr(self, 'd_x', None) is not None:
            self.d_x.free()
            self.d_x = None
        self.patch = None

    def _kron_factors(self):
        return fastdiag_factors(self.kvs, self.box[0], self.box[1], True)     # the parametric Laplacian of the free box

    @property
    def default_precond(self):
        return 'kron' if self.box is not None else 'jacobi'

    # -- the steps of one iteration, all on the device
    def _start(self, x0):
        x = np.zeros(self.n) if x0 is None else np.array(x0, dtype=np.float64).ravel()
        if x.size != self.n:
            raise ValueError('x0 has the wrong size')
        x[self.bc_indices] = self.bc_values
        self.d_x.upload(x)

    _phases = None                    # solve(timed=True): device ms of the phases, one dict per evaluation / formation / solve

    def _note(self, **ms):
        if self._phases is not None:
            self._phases.append(ms)

    def _residual_norm(self):
        self._live()
        self.jac.fields.set_resident(self.unknown, self.d_x.ptr, self._want_grad)       # step 1: the fields of the iterate
        fields_ms = self.patch.timing()['total_ms'] if self._phases is not None else 0.0
        self._d_F = self.res.assemble_vector_resident()                                 # step 2: F
        # (igx_load_vector_jet_d leaves the timing of the coefficient kernel before it in place)
        self._note(fields_ms=fields_ms, residual_coefficients_ms=self.res.patch.timing()['total_ms'] if self._phases is not None else 0.0)
        nrm = C.c_double(0.0)
        _lib.check(_lib.load().igx_solver_masked_norm_d(self.handle, self._d_F, C.byref(nrm)), 'igx_solver_masked_norm_d')
        return float(nrm.value)

    def _form_jacobian(self):
        self.jac.apply_fields()                                                         # step 3: J
        coef_ms = self.patch.timing()['total_ms'] if self._phases is not None else 0.0
        self.patch.assemble('form', to_host=False)
        self._note(jacobian_coefficients_ms=coef_ms, jacobian_assembly_ms=self.patch.timing()['total_ms'] if self._phases is not None else 0.0)
        _lib.check(_lib.load().igx_solver_values_changed(self.handle), 'igx_solver_values_changed')

    def _update(self, lin_tol, lin_maxiter):
        info = _lib.SolveInfo()
        _lib.check(_lib.load().igx_solver_newton_update_d(self.handle, self._d_F, self.d_x.ptr, float(lin_tol), int(lin_maxiter), 1,
                                                         C.byref(info)), 'igx_solver_newton_update_d')
        if not info.converged:
            warnings.warn('NewtonSystem: the linear solve stopped after %d iterations at relative residual %.2e' % (info.iterations, info.relres),
                          RuntimeWarning, stacklevel=3)
        self._note(solve_ms=float(info.total_ms), inner_iterations=int(info.iterations))
        return int(info.iterations)

    def solve(self, x0=None, atol=1e-6, rtol=1e-6, maxiter=100, freeze_jac=1, lin_tol=1e-10, lin_maxiter=1000, precond='auto',
              callback=None, timed=False):
        """Newton's method from `x0` (a full vector whose fixed entries are replaced by g; default zero on the free dofs) to
        ``||R F(x)|| < max(atol, rtol ||R F(x0)||)``; returns the full solution vector.  ``NoConvergenceError`` after `maxiter`
        steps.  `callback(k, x)`: the iterate (host copy) after step k.  Statistics in ``info``; with `timed` also
        ``info['phases']``: the device ms of every field evaluation + coefficient kernel, Jacobian formation and linear solve, in
        the order they ran."""
        self._phases = [] if timed else None
        self.set_precond(self.default_precond if precond == 'auto' else precond)
        self._start(x0)

        def update():
            inner = self._update(lin_tol, lin_maxiter)
            its.append(inner)
            if callback is not None:
                callback(len(its), self.d_x.download())
            return inner
        its = []
        converged, info = newton_loop(self._residual_norm, self._form_jacobian, update, atol, rtol, maxiter, freeze_jac)
        self.info = dict(info, converged=converged, method=self.method, precond=self._precond)
        if timed:
            self.info['phases'], self._phases = self._phases, None
        x = self.d_x.download()
        if not converged:
            raise NoConvergenceError('newton', maxiter, x)
        return x

    def residual(self, x):
        """F(x) as a host vector (all dofs)."""
        self._start(x)
        self._residual_norm()
        return self._download(self._d_F)

    def _download(self, ptr):
        out = np.empty(self.n)
        _lib.check(_lib.load().igx_dev_download(self._ctx.handle, out.ctypes.data, ptr, out.nbytes), 'igx_dev_download')
        return out

    def jacobian(self, x):
        """J(x) as scipy CSR (all dofs)."""
        self._start(x)
        self.jac.fields.set_resident(self.unknown, self.d_x.ptr, self._want_grad)
        self.jac.apply_fields()
        A = self.patch.csr('form')
        _lib.check(_lib.load().igx_solver_values_changed(self._live()), 'igx_solver_values_changed')     # (the solver's values are new)
        return A


class NavierStokesSystem(OseenSystem):
    """The stationary Navier-Stokes problem ``nu A u + (u . grad) u + B^T p = f``, ``B u = 0``, ``(u, p) = g`` on the dofs of
    `bcs`, on one patch, by Picard or Newton steps with the iterate in device memory (the loop of the reference's
    solve-navier-stokes notebook).

    Everything linear is ``OseenSystem``'s: the spaces `kvs` = ``(kvs_u, kvs_p)``, `a` (times `viscosity`), `b`, `rhs`, `bcs`,
    GMRES(`restart`) and its preconditioners.  The convection form is fixed -- ``grad(u).dot(w).dot(v) * dx`` with the wind ``w``
    the iterate, and for Newton its derivative ``grad(w).dot(u).dot(v) * dx`` besides -- and needs as many velocity components as
    dimensions.  ``B``, ``B^T``, the preconditioner factors and all buffers are made once; per step the wind is evaluated from
    the iterate by one fused kernel, the coefficient tables are formed on the device, the velocity blocks are assembled and
    replaced in the live solver, and only the residual norm and the solve statistics come down."""
    NL_METHODS = ('picard', 'newton')
    d_x = d_b = None

    def __init__(self, kvs, geo, bcs, rhs=0.0, viscosity=1.0, a='inner(grad(u), grad(v)) * dx', b='div(u) * p * dx', ncomp=None,
                 restart=40):
        from .form_assemblers import is_space_pair
        if is_space_pair(kvs) and (len(kvs[0]) if ncomp is None else int(ncomp)) != len(kvs[0]):
            raise ValueError('NavierStokesSystem needs as many velocity components as dimensions')
        OseenSystem.__init__(self, kvs, geo, bcs, rhs=rhs, convection=None, a=a, b=b, ncomp=ncomp, viscosity=viscosity, restart=restart)
        self.convection = self.WIND_FORM
        self._stokes_blocks_held = True             # the solver holds the blocks of `viscosity a` alone, as constructed

    def _drop_owner(self):
        for name in ('d_x', 'd_b'):
            if getattr(self, name) is not None:
                getattr(self, name).free()
                setattr(self, name, None)
        OseenSystem._drop_owner(self)

    def update(self, newton=False, **inputs):
        """``OseenSystem.update``; with `newton` (a wind given by its dofs only) every block also gets the Newton term
        ``grad(w).dot(u).dot(v)``: the matrix of a Newton step at ``w``."""
        self._stokes_blocks_held = False
        if not newton:
            return OseenSystem.update(self, **inputs)
        self._live()
        dofs = self._velocity_dofs(inputs['w']) if set(inputs) == {'w'} else None
        if dofs is None:
            raise ValueError('NavierStokesSystem.update: the Newton blocks need w given by its dofs')
        if self._d_wind is None:
            self._d_wind = DeviceArray(self._ctx, self.ncomp * self.N)
        self._d_wind.upload(dofs)
        self._wind_blocks(self._d_wind.ptr, newton=True)

    def _check_solve_args(self, x0, method, picard_steps):
        if method not in self.NL_METHODS:
            raise ValueError("unknown method %r: 'picard' or 'newton'" % (method,))
        if not isinstance(picard_steps, (int, np.integer)) or picard_steps < 0:
            raise ValueError('picard_steps must be a non-negative integer, not %r' % (picard_steps,))
        if x0 is None:
            return None
        x = np.array(x0, dtype=np.float64).ravel()
        if x.size != self.n:
            raise ValueError('x0 has %d entries, the system %d' % (x.size, self.n))
        return x

    def _restore_stokes_blocks(self):
        """The blocks of `viscosity a` alone back in the solver (a solve from the Stokes solution after an earlier solve)."""
        if self._stokes_blocks_held:
            return
        lib = _lib.load()
        atab = self._device_a_tables()
        for p in range(self.ncomp):
            for q in range(self.ncomp):
                if not self.present[p][q]:
                    continue
                if atab[p][q] is None:
                    _lib.check(lib.igx_solver_hide_block(self.handle, p, q, 1), 'igx_solver_hide_block')
                    continue
                self.patch.set_form_sum_resident(atab[p][q], self.viscosity, None)
                self.patch.assemble('form', to_host=False)
                _lib.check(lib.igx_solver_replace_block(self.handle, p, q), 'igx_solver_replace_block')
        self._stokes_blocks_held = True

    def _vectors(self, x):
        if self.d_x is None:
            self.d_x = DeviceArray(self._ctx, self.n)
            self.d_b = DeviceArray.from_host(self._ctx, self.b)
        self.d_x.upload(x)

    def solve(self, x0=None, method='newton', picard_steps=0, atol=1e-8, rtol=1e-8, maxiter=50, lin_tol=1e-10, lin_maxiter=1000,
              precond='auto', triangular=True, pressure='auto', restart=None, timed=False, callback=None):
        """Picard (`method` 'picard') or Newton steps ('newton', after `picard_steps` leading Picard steps) from `x0` -- a full
        vector whose fixed entries are replaced by g; default the Stokes solution, solved to `lin_tol` -- to ``||R F(x)|| <
        max(atol, rtol ||R F(x0)||)``, tested before every step; returns the full solution vector, ``NoConvergenceError`` (with
        the last iterate) after `maxiter` steps.  A step: the wind (for Newton with its gradient) from the iterate; the diagonal
        blocks ``viscosity a + (w . grad)`` assembled and replaced; ``r = R (b - K x)`` and its norm; for Newton all blocks
        assembled again with ``(u . grad) w`` added; ``x += K^-1 r`` by GMRES from zero to ``lin_tol ||r||``.  Newton therefore
        assembles the diagonal blocks twice per step: the residual is the Picard matrix's.  `precond`, `triangular`, `pressure`
        and `restart` as ``OseenSystem.solve``.  `callback(k, x)`: a host copy of the iterate after step k, normalised as the
        result is (it costs a download per step; without it only scalars come down).

        ``info``: ``iterations`` (steps), ``residual_norms`` (before every step and after the last), ``inner_iterations`` and
        ``restarts`` per correction solve, ``blocks_assembled``, ``stokes`` (the info of the first solve, or None); with `timed`
        also ``phases``: the device ms of every wind evaluation, group of assemblies and correction solve, in their order."""
        x = self._check_solve_args(x0, method, picard_steps)
        restart = self.restart if restart is None else self._check_restart(restart)
        if pressure not in self.PRESSURES:
            raise ValueError("unknown pressure %r: 'auto', 'mean' or None" % (pressure,))
        if precond != 'auto' and (precond if precond is not None else 'none') not in self.PRECONDS:
            raise ValueError('unknown preconditioner %r' % (precond,))
        h = self._live()
        lib = _lib.load()
        nc, nv = self.ncomp, self.ncomp * self.N
        project = pressure is not None and self.enclosed
        stokes = None
        if x is None:
            self._restore_stokes_blocks()
            x = OseenSystem.solve(self, tol=lin_tol, maxiter=lin_maxiter, precond=precond, triangular=triangular, pressure=pressure,
                                  restart=restart)
            stokes = self.info
        else:
            x[self.bc_indices] = self.bc_values
            _lib.check(lib.igx_solver_saddle_projection(h, 1 if project else 0, None, None), 'igx_solver_saddle_projection')
            self._select(precond, triangular, restart)
            self.set_precond(self.default_precond if precond == 'auto' else precond)
        tri = bool(triangular) and self._precond != 'none'
        self._vectors(x)
        self._phases = [] if timed else None
        self._stokes_blocks_held = False
        inner, restarts, count = [], [], [0]

        def newton_step():
            return method == 'newton' and len(inner) >= picard_steps

        def residual_norm():
            count[0] += self._wind_blocks(self.d_x.ptr, newton=False, want_grad=newton_step())
            nrm = C.c_double(0.0)
            _lib.check(lib.igx_solver_saddle_residual_d(h, self.d_b.ptr, self.d_x.ptr, C.byref(nrm)), 'igx_solver_saddle_residual_d')
            return float(nrm.value)

        def form_jacobian():
            if newton_step():
                count[0] += self._wind_blocks(self.d_x.ptr, newton=True, evaluate=False)

        def update():
            info = _lib.SolveInfo()
            _lib.check(lib.igx_solver_saddle_correct_d(h, self.d_x.ptr, float(lin_tol), int(lin_maxiter), 1, 1 if timed else 0,
                                                       C.byref(info)), 'igx_solver_saddle_correct_d')
            if not info.converged:
                warnings.warn('NavierStokesSystem: the linear solve stopped after %d iterations at relative residual %.2e'
                              % (info.iterations, info.relres), RuntimeWarning, stacklevel=3)
            inner.append(int(info.iterations))
            restarts.append(int(lib.igx_solver_gmres_restarts(h)))
            if self._phases is not None:
                self._phases.append(dict(solve_ms=float(info.total_ms), inner_iterations=int(info.iterations)))
            if callback is not None:
                callback(len(inner), normalised(self.d_x.download()))
            return int(info.iterations)

        def normalised(x):
            if project:
                x[nv:] -= x[nv] if pressure == 'auto' else x[nv:].mean()
            return x
        try:
            converged, info = newton_loop(residual_norm, form_jacobian, update, atol, rtol, maxiter, 1)
        finally:
            phases, self._phases = self._phases, None
        del info['jacobians']
        self.info = dict(info, converged=converged, method=method, picard_steps=int(picard_steps), restarts=restarts,
                         blocks_assembled=count[0], stokes=stokes, precond=self._precond, triangular=tri, restart=restart)
        if timed:
            self.info['phases'] = phases
        x = normalised(self.d_x.download())
        if not converged:
            raise NoConvergenceError(method, maxiter, x)
        return x

    def residual(self, u):
        """``R F(u)`` as a host vector (all dofs; zero on the fixed ones), ``F(u) = (viscosity A + N(u)) u + B^T p - f`` and the
        divergence rows; the fixed entries of `u` are replaced by g."""
        x = self._check_solve_args(u, 'picard', 0)
        h = self._live()
        x[self.bc_indices] = self.bc_values
        self._vectors(x)
        self._stokes_blocks_held = False
        self._wind_blocks(self.d_x.ptr, newton=False)
        d_y = DeviceArray(self._ctx, self.n)
        _lib.check(_lib.load().igx_solver_saddle_product_d(h, self.d_x.ptr, self.d_b.ptr, -1.0, None, d_y.ptr, None),
                   'igx_solver_saddle_product_d')
        return -d_y.download()


################################################################################
# Generalized eigenproblems of one patch on the device: block LOBPCG
################################################################################

EIG_WIDTHS = (4, 8, 16)                  # the compiled row strides MB of the block kernels (csrc/solve_eig.hip)
EIG_MAX_BLOCK = EIG_WIDTHS[-1]
# A projected mass Gram matrix, scaled to a unit diagonal, counts as positive definite when its smallest eigenvalue is above
# this: below it the columns of [X W P] are dependent to within sqrt(eps) and the projected pencil loses half of its digits.
RR_MIN_EIG = 1e-9


def eig_width(m):
    """The row stride of a block of `m` columns: the smallest compiled width >= m."""
    for w in EIG_WIDTHS:
        if m <= w:
            return w
    raise ValueError('block of %d columns: at most %d' % (m, EIG_MAX_BLOCK))


def _sym(G):
    G = np.asarray(G, dtype=np.float64)
    return 0.5 * (G + G.T)


def _unit_diagonal(G):
    """``(s, s G s)`` with ``s = diag(G)^-1/2``, or None when G has a non-finite entry or a non-positive diagonal one."""
    if not np.all(np.isfinite(G)):
        return None
    d = np.diag(G)
    if not np.all(d > 0.0):
        return None
    s = 1.0 / np.sqrt(d)
    return s, G * s[:, None] * s[None, :]


def rayleigh_ritz(GK, GM, m):
    """The `m` lowest eigenpairs of the projected pencil ``GK c = lam GM c`` (``scipy.linalg.eigh``): ``(lam, C, ok)`` with
    ``C^T GM C = I``.  Both matrices are symmetrised; GM is scaled to a unit diagonal first, so that blocks of very different
    norms do not decide its conditioning.  ``ok`` is False, and lam and C are None, when a matrix is not finite, GM is not
    positive definite to ``RR_MIN_EIG`` on that scale, or LAPACK fails: nothing is raised and nothing half-computed comes back."""
    GK, GM = _sym(GK), _sym(GM)
    sc = _unit_diagonal(GM)
    if sc is None or not np.all(np.isfinite(GK)):
        return None, None, False
    s, GMs = sc
    GKs = GK * s[:, None] * s[None, :]
    try:
        if scipy.linalg.eigvalsh(GMs)[0] <= RR_MIN_EIG:
            return None, None, False
        lam, C = scipy.linalg.eigh(GKs, GMs)
    except (scipy.linalg.LinAlgError, ValueError):
        return None, None, False
    if not (np.all(np.isfinite(lam)) and np.all(np.isfinite(C))):
        return None, None, False
    return lam[:m].copy(), np.ascontiguousarray(s[:, None] * C[:, :m]), True


def _inv_chol_t(G):
    """``L^-T`` of the Cholesky factor ``G = L L^T`` (so that ``B L^-T`` is orthonormal when G is the Gram matrix of B), or None
    when G is not numerically positive definite (judged on the unit-diagonal scale, as rayleigh_ritz does)."""
    sc = _unit_diagonal(_sym(G))
    if sc is None:
        return None
    s, Gs = sc
    try:
        if scipy.linalg.eigvalsh(Gs)[0] <= RR_MIN_EIG:
            return None
        L = scipy.linalg.cholesky(Gs, lower=True)
    except (scipy.linalg.LinAlgError, ValueError):
        return None
    return np.ascontiguousarray(s[:, None] * scipy.linalg.solve_triangular(L, np.eye(L.shape[0]), lower=True).T)


def lobpcg_loop(ops, m, k, tol, maxiter):
    """Knyazev's block LOBPCG for the `k` lowest eigenpairs of ``K x = lam M x`` with a block of `m` columns, on an operations
    object that keeps the blocks wherever they live (EigenSystem: on the device; the tests: numpy arrays).  Only Gram matrices
    and residual norms come back from `ops`, only coefficient matrices go to it:

    - ``ops.start()``: the masked start block becomes ``X``;
    - ``ops.products(name)``: ``K<name>``, ``M<name>`` from block ``name`` ('X', 'W'), one pass over both matrices;
    - ``ops.gram(A, B)``: the Gram matrix of the concatenated blocks named in the lists A and B;
    - ``ops.combine(updates, triple)``: for every ``(dst, srcs, coeffs)`` the block ``sum_j srcs[j] @ coeffs[j]`` -- all read
      before any is written; `triple`: the same for the K and M companions of the named blocks;
    - ``ops.residuals(lam)``: ``R = KX - MX diag(lam)``; returns the column norms of R and of KX;
    - ``ops.precond(src, dst)``.

    Pair i has converged when ``||R_i|| <= tol ||K X_i||``; the loop stops when the first k have.  A failed Cholesky or projected
    eigh drops P for that iteration (a restart); two restarts in consecutive iterations end the solve unconverged.
    Returns ``(lam, info)`` with all m Ritz values; the Ritz vectors are the block ``X`` of `ops`."""
    eye = np.eye(m)
    info = dict(iterations=0, restarts=0, products=0, block=m, converged=np.zeros(k, dtype=bool), residuals=np.full(k, np.inf),
                failed=None)

    def fail(why):
        info['failed'] = why
        return np.full(m, np.nan), info

    ops.start()
    ops.products('X')
    info['products'] += 1
    Ci = _inv_chol_t(ops.gram(['X'], ['MX']))
    if Ci is None:
        return fail('the start block is not of full rank in the mass inner product')
    ops.combine([('X', ['X'], [Ci])], True)
    lam, C, ok = rayleigh_ritz(ops.gram(['X'], ['KX']), ops.gram(['X'], ['MX']), m)
    if not ok:
        return fail('the Rayleigh-Ritz step on the start block failed')
    ops.combine([('X', ['X'], [C])], True)
    have_p, last_restart = False, -2

    def restart(it):
        nonlocal have_p, last_restart
        info['restarts'] += 1
        again = last_restart == it - 1
        last_restart = it
        have_p = False
        return again

    it = 0
    while True:
        rn, kn = ops.residuals(lam)
        rn, kn = np.asarray(rn)[:m], np.asarray(kn)[:m]
        with np.errstate(divide='ignore', invalid='ignore'):
            rel = np.where(kn > 0.0, rn / kn, np.where(rn == 0.0, 0.0, np.inf))
        info['residuals'] = rel[:k].copy()
        info['converged'] = rn[:k] <= tol * kn[:k]
        if info['converged'].all() or it >= maxiter:
            break
        it += 1
        info['iterations'] = it
        ops.precond('R', 'W')
        ops.combine([('W', ['W', 'X'], [eye, -ops.gram(['MX'], ['W'])])], False)          # W -= X (X^T M W)
        ops.products('W')
        info['products'] += 1
        Ci = _inv_chol_t(ops.gram(['W'], ['MW']))
        if Ci is None:                                          # (W is dependent: nothing to iterate with)
            if restart(it):
                info['failed'] = 'two restarts in a row'
                break
            continue
        ops.combine([('W', ['W'], [Ci])], True)
        names = ['X', 'W'] + (['P'] if have_p else [])
        GK = ops.gram(names, ['K' + b for b in names])
        GM = ops.gram(names, ['M' + b for b in names])
        lam_new, C, ok = rayleigh_ritz(GK, GM, m)
        if not ok and have_p:                                   # this iteration runs without P
            if restart(it):
                info['failed'] = 'two restarts in a row'
                break
            names = ['X', 'W']
            lam_new, C, ok = rayleigh_ritz(GK[:2 * m, :2 * m], GM[:2 * m, :2 * m], m)
        if not ok:
            if restart(it):
                info['failed'] = 'two restarts in a row'
                break
            continue
        lam = lam_new
        coeffs = [C[j * m:(j + 1) * m] for j in range(len(names))]
        ops.combine([('X', names, coeffs), ('P', names[1:], coeffs[1:])], True)
        Ci = _inv_chol_t(ops.gram(['P'], ['MP']))
        if Ci is None:                                          # the next iteration runs without P
            if restart(it):
                info['failed'] = 'two restarts in a row'
                break
            continue
        ops.combine([('P', ['P'], [Ci])], True)
        have_p = True
    return lam, info


def _symmetric_problem(problem, kvs, args):
    """Is the matrix of `problem` known to be symmetric before any device work?  The built-in stiffness and mass forms are; a
    general form string is when its traced coefficient table is (the test NewtonSystem applies to its Jacobian); an assembler
    class or object when its kind is one of the two."""
    from . import forms
    kind = _form_kind(problem)
    if kind in ('mass', 'stiffness'):
        return True
    if kind != 'form' or not isinstance(problem, str):
        return False
    try:
        return _symmetric_traced_table(forms.symbolic_table(problem, len(kvs), dict(args)))
    except Exception:
        return False


class _DeviceEigOps:
    """The operations of ``lobpcg_loop`` on the blocks of a device session (``igx_solver_eig_*``)."""

    def __init__(self, handle, n, m, X0, timed):
        self.h, self.n, self.m = handle, n, m
        self.X0 = np.ascontiguousarray(X0, dtype=np.float64)
        self.timed = 1 if timed else 0
        self.lib = _lib.load()

    @staticmethod
    def _ids(names):
        return (C.c_int32 * len(names))(*[_lib.IGX_EIG_BLOCKS[b] for b in names])

    def start(self):
        _lib.check(self.lib.igx_solver_eig_begin(self.h, self.m, _lib.dptr(self.X0), self.timed), 'igx_solver_eig_begin')

    def products(self, name):
        B = _lib.IGX_EIG_BLOCKS
        _lib.check(self.lib.igx_solver_eig_products(self.h, B[name], B['K' + name], B['M' + name]), 'igx_solver_eig_products')

    def gram(self, A, B):
        G = np.empty((len(A) * self.m, len(B) * self.m))
        _lib.check(self.lib.igx_solver_eig_gram(self.h, len(A), self._ids(A), len(B), self._ids(B), _lib.dptr(G)), 'igx_solver_eig_gram')
        return G

    def combine(self, updates, triple):
        dst = self._ids([u[0] for u in updates])
        nsrc = (C.c_int32 * len(updates))(*[len(u[1]) for u in updates])
        src = (C.c_int32 * (3 * len(updates)))()
        for i, (_, names, _) in enumerate(updates):
            for j, b in enumerate(names):
                src[3 * i + j] = _lib.IGX_EIG_BLOCKS[b]
        coef = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.float64).reshape(-1) for u in updates for c in u[2]]))
        _lib.check(self.lib.igx_solver_eig_combine(self.h, len(updates), dst, nsrc, src, _lib.dptr(coef), 1 if triple else 0),
                   'igx_solver_eig_combine')

    def residuals(self, lam):
        lam = np.ascontiguousarray(lam, dtype=np.float64)
        rn, kn = np.empty(self.m), np.empty(self.m)
        _lib.check(self.lib.igx_solver_eig_residuals(self.h, _lib.dptr(lam), _lib.dptr(rn), _lib.dptr(kn)), 'igx_solver_eig_residuals')
        return rn, kn

    def precond(self, src, dst):
        B = _lib.IGX_EIG_BLOCKS
        _lib.check(self.lib.igx_solver_eig_precond(self.h, B[src], B[dst]), 'igx_solver_eig_precond')

    def download(self, name, k):
        out = np.empty((self.n, k))
        _lib.check(self.lib.igx_solver_eig_download(self.h, _lib.IGX_EIG_BLOCKS[name], k, _lib.dptr(out)), 'igx_solver_eig_download')
        return out

    def info(self):
        info = _lib.EigInfo()
        _lib.check(self.lib.igx_solver_eig_info(self.h, C.byref(info)), 'igx_solver_eig_info')
        return info.as_dict()

    def end(self):
        _lib.check(self.lib.igx_solver_eig_end(self.h), 'igx_solver_eig_end')


def default_eig_block(k):
    """``k + max(2, k // 2)`` columns (the guard columns keep the k-th pair away from the edge of the block), at most 16."""
    return min(EIG_MAX_BLOCK, k + max(2, k // 2))


def _check_eig_args(k, block, n_free):
    if k < 1:
        raise ValueError('k must be at least 1, not %r' % (k,))
    if block > EIG_MAX_BLOCK:
        raise ValueError('block of %d columns: at most %d' % (block, EIG_MAX_BLOCK))
    if k > block:
        raise ValueError('k = %d pairs need a block of at least k columns, not %d' % (k, block))
    if 3 * block > n_free:
        raise ValueError('a block of %d columns needs at least %d free dofs, the problem has %d' % (block, 3 * block, n_free))


def _eig_fixed_dofs(bcs, n):
    """The sorted unique fixed dofs of `bcs` (``(indices, values)`` or just the indices) among `n` dofs."""
    if bcs is None:
        idx = np.zeros(0, dtype=np.int64)
    elif isinstance(bcs, tuple) and len(bcs) == 2 and np.ndim(bcs[0]) >= 1:
        idx = np.asarray(bcs[0], dtype=np.int64).ravel()
    else:
        idx = np.asarray(bcs, dtype=np.int64).ravel()
    idx = np.unique(idx)
    if idx.size and (idx[0] < 0 or idx[-1] >= n):
        raise ValueError('fixed dof out of range')
    return idx


class _EigBlockPieces:
    """What the eigen-solvers share (``EigenSystem``, ``VectorEigenSystem``, ``MultipatchEigenSystem``): the solve, the switch of
    the preconditioner, and the block kernels alone on host arrays of shape ``(n, m)`` (``igx_solver_eig_*_d``).  A class
    supplies ``_live()``, ``_ctx``, ``n``, ``n_free``, ``PRECONDS`` and ``set_precond`` (also under the name
    ``_set_eig_precond``)."""

    def _eig_solve(self, k, tol, maxiter, precond, block, X0, seed, timed):
        """``solve`` of every eigen-system: ``lobpcg_loop`` on the device session of the system."""
        k = int(k)
        m = default_eig_block(max(k, 1)) if block is None else int(block)
        _check_eig_args(k, m, self.n_free)
        self._check_solve_precond(precond)
        if X0 is None:
            X0 = np.random.default_rng(seed).standard_normal((self.n, m))
        else:
            X0 = np.asarray(X0, dtype=np.float64)
            if X0.shape != (self.n, m):
                raise ValueError('X0 of shape %r, expected %r' % (X0.shape, (self.n, m)))
        h = self._live()
        key = self.set_precond(precond)
        ops = _DeviceEigOps(h, self.n, m, X0, timed)
        try:
            lam, info = lobpcg_loop(ops, m, k, float(tol), int(maxiter))
            U = ops.download('X', k)
            dev = ops.info()
        finally:
            ops.end()
        info.update(precond=key, block_products=dev['products'], n_free=dev['n_free'], width=dev['mb'])
        self.info = info
        self._eig_solve_info(key)
        if timed:
            info.update({name: dev[name] for name in dev if name.endswith('_ms')})
        return lam[:k].copy(), U

    def _check_solve_precond(self, precond):
        """Hook of ``_eig_solve``: ValueError for a name `precond` that ``set_precond`` would refuse, before the start block is
        drawn.  (Nothing for the one-patch systems: their ``set_precond`` refuses it after.)"""

    def _eig_solve_info(self, key):
        """Hook of ``_eig_solve``: further entries of ``self.info`` after a solve preconditioned with `key`."""

    def _precond_key(self, precond):
        """The name of `precond` ('none' for None, 'auto' as it is), or ValueError: before any device work."""
        key = precond if precond is not None else 'none'
        if key != 'auto' and key not in self.PRECONDS:
            raise ValueError('unknown preconditioner %r' % (precond,))
        return key

    def _auto_precond(self):
        return self.default_precond

    def _switch_eig_precond(self, precond, install):
        """``set_precond`` of every eigen-system: checks the name, resolves 'auto' (``_auto_precond``) and, unless it is the one
        in place, has ``install(handle, key)`` hand the preconditioner to the device; returns its name."""
        key = self._precond_key(precond)
        h = self._live()
        if key == 'auto':
            key = self._auto_precond()
        if key != self._eig_precond:
            install(h, key)
            self._eig_precond = key
        return key

    # -- the pieces alone, on host arrays of shape (n, m)
    def _upload_block(self, A):
        A = np.asarray(A, dtype=np.float64)
        if A.ndim != 2 or A.shape[0] != self.n or not 1 <= A.shape[1] <= EIG_MAX_BLOCK:
            raise ValueError('block of shape %r: (%d, m) with 1 <= m <= %d' % (A.shape, self.n, EIG_MAX_BLOCK))
        return A.shape[1]

    def _padded(self, A, mb):
        P = np.zeros((self.n, mb))
        P[:, :A.shape[1]] = A
        return DeviceArray.from_host(self._ctx, P)

    def _down(self, d, mb, m):
        return np.ascontiguousarray(d.download().reshape(self.n, mb)[:, :m])

    def block_products(self, X):
        """``(R K R^T X, R M R^T X)`` by one pass of the block product over both matrices."""
        h = self._live()
        m = self._upload_block(X)
        mb = eig_width(m)
        d_x = self._padded(np.asarray(X, dtype=np.float64), mb)
        d_k, d_m = DeviceArray(self._ctx, self.n * mb), DeviceArray(self._ctx, self.n * mb)
        _lib.check(_lib.load().igx_solver_eig_products_d(h, mb, d_x.ptr, d_k.ptr, d_m.ptr), 'igx_solver_eig_products_d')
        return self._down(d_k, mb, m), self._down(d_m, mb, m)

    def block_product(self, X, which='K'):
        """``R K R^T X`` (or ``R M R^T X``, ``which='M'``) by the one-matrix form of the block product."""
        h = self._live()
        m = self._upload_block(X)
        mb = eig_width(m)
        d_x = self._padded(np.asarray(X, dtype=np.float64), mb)
        d_y = DeviceArray(self._ctx, self.n * mb)
        args = (d_y.ptr, None) if which == 'K' else (None, d_y.ptr)
        _lib.check(_lib.load().igx_solver_eig_products_d(h, mb, d_x.ptr, *args), 'igx_solver_eig_products_d')
        return self._down(d_y, mb, m)

    def gram(self, A, B):
        """``A^T B`` over the free dofs; A and B: blocks of the same number of columns, or lists of up to three such blocks
        (the Gram matrix of their concatenations)."""
        h = self._live()
        A = [A] if isinstance(A, np.ndarray) else list(A)
        B = [B] if isinstance(B, np.ndarray) else list(B)
        m = self._upload_block(A[0])
        if any(self._upload_block(Z) != m for Z in A + B) or not (1 <= len(A) <= 3 and 1 <= len(B) <= 3):
            raise ValueError('gram: one to three blocks a side, all of the same number of columns')
        mb = eig_width(m)
        dA = [self._padded(np.asarray(Z, dtype=np.float64), mb) for Z in A]
        dB = [self._padded(np.asarray(Z, dtype=np.float64), mb) for Z in B]
        G = np.empty((len(A) * m, len(B) * m))
        pa = (C.c_void_p * len(dA))(*[d.ptr for d in dA])
        pb = (C.c_void_p * len(dB))(*[d.ptr for d in dB])
        _lib.check(_lib.load().igx_solver_eig_gram_d(h, mb, m, len(dA), pa, len(dB), pb, _lib.dptr(G)), 'igx_solver_eig_gram_d')
        return G

    def combine(self, blocks, coeffs):
        """``sum_j blocks[j] @ coeffs[j]`` for up to three blocks of m columns and m x m coefficient matrices."""
        h = self._live()
        blocks, coeffs = list(blocks), [np.asarray(c, dtype=np.float64) for c in coeffs]
        m = self._upload_block(blocks[0])
        if not 1 <= len(blocks) <= 3 or len(coeffs) != len(blocks) or any(self._upload_block(Z) != m for Z in blocks) \
                or any(c.shape != (m, m) for c in coeffs):
            raise ValueError('combine: one to three blocks of m columns with an m x m coefficient matrix each')
        mb = eig_width(m)
        dS = [self._padded(np.asarray(Z, dtype=np.float64), mb) for Z in blocks]
        d_y = DeviceArray(self._ctx, self.n * mb)
        ps = (C.c_void_p * len(dS))(*[d.ptr for d in dS])
        cf = np.ascontiguousarray(np.stack(coeffs))
        _lib.check(_lib.load().igx_solver_eig_combine_d(h, mb, m, len(dS), ps, _lib.dptr(cf), d_y.ptr), 'igx_solver_eig_combine_d')
        return self._down(d_y, mb, m)

    def residuals(self, KX, MX, lam):
        """``(R, ||R_j||, ||KX_j||)`` with ``R = KX - MX diag(lam)`` on the free dofs (zero elsewhere), by the fused kernel."""
        h = self._live()
        m = self._upload_block(KX)
        lam = np.ascontiguousarray(lam, dtype=np.float64)
        if self._upload_block(MX) != m or lam.shape != (m,):
            raise ValueError('residuals: KX and MX of m columns and m values of lam')
        mb = eig_width(m)
        d_k, d_m = self._padded(np.asarray(KX, dtype=np.float64), mb), self._padded(np.asarray(MX, dtype=np.float64), mb)
        d_r = DeviceArray(self._ctx, self.n * mb)
        rn, kn = np.empty(m), np.empty(m)
        _lib.check(_lib.load().igx_solver_eig_residuals_d(h, mb, m, d_k.ptr, d_m.ptr, _lib.dptr(lam), d_r.ptr, _lib.dptr(rn),
                                                          _lib.dptr(kn)), 'igx_solver_eig_residuals_d')
        return self._down(d_r, mb, m), rn, kn

    def apply_precond(self, R, precond='auto'):
        """The preconditioner applied to every column of the block R."""
        h = self._live()
        m = self._upload_block(R)
        self._set_eig_precond(precond)
        mb = eig_width(m)
        d_r = self._padded(np.asarray(R, dtype=np.float64), mb)
        d_z = DeviceArray(self._ctx, self.n * mb)
        _lib.check(_lib.load().igx_solver_eig_precond_d(h, mb, d_r.ptr, d_z.ptr), 'igx_solver_eig_precond_d')
        return self._down(d_z, mb, m)


class EigenSystem(_PatchErrorNorms, _EigBlockPieces, _DeviceSystem):
    """The lowest eigenpairs of ``K x = lam M x`` on the free dofs of one patch (x = 0 on the dofs of `bcs`), by block LOBPCG
    with both matrices, the blocks and the preconditioner in device memory.

    M is the mass matrix of the patch; K the stiffness matrix (`problem` None) or the matrix of any form that ``FormSystem``
    accepts and whose traced coefficient table is symmetric (`problem`, with `args` / `inputs` its inputs).  Both are assembled on
    the device and handed to the solver as ``ParabolicSystem`` does; no ``C = M + tau gamma K`` is formed.  `bcs`:
    ``(indices, values)`` or just the indices; only the indices are used.

    ``solve(k)`` returns ``(lam, U)``: the k smallest eigenvalues in ascending order and ``U`` of shape ``(prod(ndofs), k)`` with
    ``U^T M U = I`` and zeros on the fixed dofs; ``info`` holds the statistics.  ``block_products``, ``gram``, ``combine``,
    ``residuals`` and ``apply_precond`` run the block kernels alone on host arrays of shape ``(n, m)``."""

    def __init__(self, kvs, geo, bcs=None, problem=None, args=None, device=None, **inputs):
        from . import assemble
        args = dict(args or {})
        args.update(inputs)
        if geo is not None:
            args.setdefault('geo', geo)
        self.kvs = tuple(kvs)
        self.geo = geo
        if problem is not None:
            _check_device_form(problem, self.kvs, args)
            if not _symmetric_problem(problem, self.kvs, args):
                raise ValueError('EigenSystem: %r is not known to be symmetric (the built-in stiffness and mass forms are, and a '
                                 'form string whose traced coefficient table is)' % (problem,))
        self.ndofs = tuple(kv.numdofs for kv in self.kvs)
        self.n = int(np.prod(self.ndofs))
        idx = _eig_fixed_dofs(bcs, self.n)
        if _form_kind(problem) == 'stiffness' and idx.size == 0:
            raise ValueError('EigenSystem: the stiffness matrix without any fixed dof is singular (the constants), and the relative '
                             "stopping rule ||r|| <= tol ||K x|| has no scale there.  Shift instead: problem='(inner(grad(u), "
                             "grad(v)) + u*v) * dx', then subtract 1 from the eigenvalues")
        self.n_free = self.n - idx.size
        if problem is None:
            self.patch = assemblers.DevicePatch(self.kvs, geo, device=device)
            self._own_patch = True
            self.kind = 'stiffness'
        else:
            self.assembler = assemble.instantiate_assembler(problem, self.kvs, args)
            self._own_patch = self.assembler is not problem
            self.patch = self.assembler.patch
            self.kind = self.assembler._kind
        self._ctx = self.patch.ctx
        try:
            self._attach('igx_solver_create_parabolic', (self.patch.handle, _lib.KINDS[self.kind], 1), (idx, np.zeros(idx.size)),
                         'cg', 'cg')
            self.box = dirichlet_box(self.ndofs, self.bc_indices)
            lib = _lib.load()
            self.patch.assemble(self.kind, to_host=False)            # the values stay on the device and change hands
            _lib.check(lib.igx_solver_take_values(self.handle, _lib.IGX_ROLE_OPERATOR), 'igx_solver_take_values')
            self.patch.assemble('mass', to_host=False)
            _lib.check(lib.igx_solver_take_values(self.handle, _lib.IGX_ROLE_MASS), 'igx_solver_take_values')
        except BaseException:
            self._release()
            self._drop_owner()
            raise
        self._eig_precond = False                                    # (no preconditioner of the eigen pieces set yet)

    @property
    def default_precond(self):
        return 'kron' if self.box is not None else 'jacobi'

    def _kron_factors(self):
        return fastdiag_factors(self.kvs, self.box[0], self.box[1], True)     # the parametric Laplacian of the free box

    def set_precond(self, precond):
        """The preconditioner of ``solve`` and ``apply_precond``: 'auto', 'kron', 'jacobi' or None."""
        def install(h, key):
            lib = _lib.load()
            if key == 'kron':
                if self.box is None:
                    raise ValueError("precond='kron' needs the fixed dofs to be a union of whole sides of the patch")
                U, lam, mode = self._kron_factors()
                lo, hi, Up, Lp = _box_args(self.box[0], self.box[1], U, lam)
                _lib.check(lib.igx_solver_eig_set_precond(h, _lib.IGX_PRECOND_KRON, lo, hi, Up, Lp, mode), 'igx_solver_eig_set_precond')
            else:
                _lib.check(lib.igx_solver_eig_set_precond(h, self.PRECONDS[key], None, None, None, None, 0), 'igx_solver_eig_set_precond')
        return self._switch_eig_precond(precond, install)

    _set_eig_precond = set_precond

    def solve(self, k=6, tol=1e-8, maxiter=200, precond='auto', block=None, X0=None, seed=0, timed=False):
        """Block LOBPCG (``lobpcg_loop``) to ``||K x_i - lam_i M x_i|| <= tol ||K x_i||`` for the k lowest pairs.  `block`: the
        columns iterated (default ``k + max(2, k // 2)``, at most 16); `X0`: a start block of shape ``(n, block)``, else normal
        deviates of ``numpy.random.default_rng(seed)``.  Deterministic: the same inputs give the same bits."""
        return self._eig_solve(k, tol, maxiter, precond, block, X0, seed, timed)

    def spmv(self, x):
        raise NotImplementedError('EigenSystem holds two matrices: block_products(X) or block_product(X, which)')


class VectorEigenSystem(_VectorBlocks, _EigBlockPieces, _DeviceSystem):
    """The lowest eigenpairs of ``K x = lam (I (x) M) x`` for a vector-valued form K (``bfuns=[('u', nc), ('v', nc)]``, nc = 2 or
    3) on the free dofs of one patch: the natural frequencies and mode shapes of an elastic body, by block LOBPCG with the
    nc x nc blocks, the mass matrix, the iterated blocks and the preconditioner in device memory.

    `problem`, `bfuns`, `args` / `inputs` (``geo`` among them): as ``VectorFormSystem`` takes them (a form string); the block
    coefficient tables must be symmetric.  `bcs`: ``(indices, values)`` or just the indices, in the blocked numbering
    (component-major, as ``assemble(..., layout='blocked')``); only the indices are used.  `mass`: None for the mass matrix of
    the patch, or a scalar bilinear form string that ``FormSystem`` accepts and whose traced table is symmetric, such as
    ``'rho*u*v*dx'`` for a density; the same M weighs every component.

    ``solve(k)`` returns ``(lam, U)``: the k smallest eigenvalues in ascending order and ``U`` of shape ``(nc * N, k)`` with
    ``U^T (I (x) M) U = I`` and zeros on the fixed dofs; ``U.reshape((nc,) + ndofs + (k,))`` gives the components on the tensor
    grid of dofs.  ``block_products``, ``gram``, ``combine``, ``residuals`` and ``apply_precond`` run the block kernels alone on
    host arrays of shape ``(nc * N, m)``.  The preconditioner is the block-diagonal Kronecker one of ``VectorFormSystem``
    (``kron_factors``) when the fixed dofs of every component are whole sides, else Jacobi."""

    def __init__(self, problem, kvs, bcs=None, args=None, bfuns=None, mass=None, **inputs):
        from . import tforms
        from .form_assemblers import FormAssembler, _full_table
        args = dict(args or {})
        args.update(inputs)
        self.kvs = tuple(kvs)
        nc = _vector_components(problem, self.kvs, args, bfuns)
        if mass is not None:
            ok = isinstance(mass, str)
            if ok:
                try:
                    _check_device_form(mass, self.kvs, args)
                    ok = _symmetric_problem(mass, self.kvs, args)
                except Exception as e:
                    raise ValueError('VectorEigenSystem: mass=%r: %s' % (mass, e))
            if not ok:
                raise ValueError('VectorEigenSystem: mass=%r is not a scalar bilinear form string whose traced coefficient table '
                                 "is symmetric (such as 'rho*u*v*dx'), or None for the mass matrix of the patch" % (mass,))
        self.ncomp = nc
        self.ndofs = tuple(kv.numdofs for kv in self.kvs)
        self.N = int(np.prod(self.ndofs))
        self.n = nc * self.N
        idx = _eig_fixed_dofs(bcs, self.n)
        self.n_free = self.n - idx.size
        self.assembler = FormAssembler(self.kvs, args['geo'], problem, bfuns=bfuns, inputs=args)
        self.patch = self.assembler.patch
        table = self.assembler._table
        if not symmetric_block_tables(table):
            raise ValueError('VectorEigenSystem: the block coefficient tables of %r are not symmetric' % (problem,))
        if idx.size == 0 and all(table[p][q][0][0] is None for p in range(nc) for q in range(nc)):
            raise ValueError('VectorEigenSystem: without any fixed dof and without a zeroth-order term K annihilates the constants, '
                             'and the relative stopping rule ||r|| <= tol ||K x|| has no scale there.  Shift instead: add '
                             "'+ inner(u, v)' to the form, then subtract 1 from the eigenvalues")
        self._ctx = self.patch.ctx
        try:
            self._attach('igx_solver_create_block', (self.patch.handle, nc, 1), (idx, np.zeros(idx.size)), 'cg', 'cg')
            self._take_blocks(table)
            self._component_boxes()
            if mass is None:
                self.patch.assemble('mass', to_host=False)           # the values stay on the device and change hands
            else:
                d = len(self.kvs)
                grid = [self.patch.gauss(k)[0] for k in range(d)]
                X = np.asarray(args['geo'].grid_eval(grid))
                scalar = {k: v for k, v in args.items() if k != 'geo'}
                _, _, mtable, _ = tforms.evaluate(mass, tuple(len(g) for g in grid), X, scalar, None)
                self.patch.set_form(_full_table(mtable[0][0], d))
                self.patch.assemble('form', to_host=False)
            _lib.check(_lib.load().igx_solver_take_mass(self.handle), 'igx_solver_take_mass')
        except BaseException:
            self._release()
            self._drop_owner()
            raise
        self._eig_precond = False                                    # (no preconditioner of the eigen pieces set yet)

    def set_precond(self, precond):
        """The preconditioner of ``solve`` and ``apply_precond``: 'auto', 'kron', 'jacobi' or None."""
        def install(h, key):
            if key == 'kron' and not self._factors_set:
                self._set_block_kron(h)                              # (ValueError when a component has no free box)
                self._factors_set = True
            _lib.check(_lib.load().igx_solver_eig_set_precond(h, self.PRECONDS[key], None, None, None, None, 0),
                       'igx_solver_eig_set_precond')
        return self._switch_eig_precond(precond, install)

    _set_eig_precond = set_precond

    def solve(self, k=6, tol=1e-8, maxiter=200, precond='auto', block=None, X0=None, seed=0, timed=False):
        """Block LOBPCG (``lobpcg_loop``) to ``||K x_i - lam_i (I (x) M) x_i|| <= tol ||K x_i||`` for the k lowest pairs;
        arguments, ``info`` and determinism as ``EigenSystem.solve`` (`X0` of shape ``(nc * N, block)``)."""
        return self._eig_solve(k, tol, maxiter, precond, block, X0, seed, timed)

    def spmv(self, x):
        raise NotImplementedError('VectorEigenSystem holds two matrices: block_products(X) or block_product(X, which)')


STIFFNESS_FORM = 'inner(grad(u), grad(v)) * dx'
MASS_FORM = 'u * v * dx'


class _SymmetricLevelSystem(MultipatchSystem):
    """A coarse level of ``MultipatchEigenSystem``: its form was shown to be symmetric (``_symmetric_problem``) before any level
    was made, which the assembler of a general form string cannot declare."""
    _inspect_symmetry = False


class MultipatchEigenSystem(_EigBlockPieces, MultipatchSystem):
    """The lowest eigenpairs of ``K x = lam M x`` on the free dofs of the multipatch `MP` (x = 0 on the dofs of `bcs`), by block
    LOBPCG with both global CSR matrices, the blocks and the preconditioner in device memory.

    M is the mass matrix summed over `MP`; K the summed stiffness matrix (`problem` None) or that of any form ``FormSystem``
    accepts whose matrix is known to be symmetric on every patch (`problem`, with `args` / `inputs` its inputs).  The mass sums
    are copied into an array of the solver's own, then `problem` is summed: K is what `MP` holds, so a later
    ``MP.assemble_system`` restarts it (``solve`` then raises IgxError) and ``MP.close()`` destroys the solver.  `bcs`:
    ``(indices, values)`` or just the indices; only the indices are used.

    ``solve(k)`` returns ``(lam, U)`` as ``EigenSystem.solve`` does, ``U`` of shape ``(MP.numdofs, k)``.  Preconditioners: 'mg'
    (one V-cycle of ``set_multigrid`` per column), 'jacobi', None.  ``block_products``, ``gram``, ``combine``, ``residuals`` and
    ``apply_precond`` run the block kernels alone on host arrays of shape ``(n, m)``; ``spmv(x)`` is ``R K R^T x`` and
    ``vcycle(r)`` the V-cycle on one vector."""

    PRECONDS = {None: _lib.IGX_PRECOND_NONE, 'none': _lib.IGX_PRECOND_NONE, 'jacobi': _lib.IGX_PRECOND_JACOBI, 'mg': _lib.IGX_PRECOND_MG}

    def __init__(self, MP, bcs=None, problem=None, args=None, **inputs):
        self.MP = MP
        args = dict(args or {})
        args.update(inputs)
        if args.get('bfuns') is not None:
            raise ValueError('MultipatchEigenSystem: vector-valued problems (bfuns) are not supported')
        if problem is not None:
            for kvs, geo in MP.patches:
                pargs = dict(args, geo=geo)
                _check_device_form(problem, tuple(kvs), pargs)
                if not _symmetric_problem(problem, tuple(kvs), pargs):
                    raise ValueError('MultipatchEigenSystem: %r is not known to be symmetric (the built-in stiffness and mass '
                                     'forms are, and a form string whose traced coefficient table is)' % (problem,))
        self.n = MP.numdofs
        idx = _eig_fixed_dofs(bcs, self.n)
        if _form_kind(problem) == 'stiffness' and idx.size == 0:
            raise ValueError('MultipatchEigenSystem: the stiffness matrix without any fixed dof is singular (the constants), and '
                             "the relative stopping rule ||r|| <= tol ||K x|| has no scale there.  Shift instead: "
                             "problem='(inner(grad(u), grad(v)) + u*v) * dx', then subtract 1 from the eigenvalues")
        self.n_free = self.n - idx.size
        form = STIFFNESS_FORM if problem is None else problem
        self._problem = (form, None, args, {})
        self._eig_precond = False                                    # (no preconditioner of the eigen pieces set yet)
        lib = _lib.load()
        kinds = []
        h = MP._sum_system(MASS_FORM, None, args, False, 'csr', 'blocked', {})
        self._ctx = MP._ctx
        d_M = lib.igx_dev_alloc(self._ctx.handle, max(1, MP.info()['nnz']) * 8)
        if not d_M:
            raise _lib.IgxError('igx_dev_alloc failed: ' + _lib.last_error())
        try:
            _lib.check(lib.igx_multipatch_values_d(h, d_M), 'igx_multipatch_values_d')
            h = MP._sum_system(form, None, args, False, 'csr', 'blocked', {},
                               on_assembler=lambda p, asm: kinds.append(getattr(asm, '_kind', None)))
            self.kind = kinds[0] if kinds and all(k == kinds[0] for k in kinds) else None
            self._attach('igx_solver_create_multipatch', (h,), (idx, np.zeros(idx.size)), 'cg', 'cg')
            _lib.check(lib.igx_solver_set_mass_d(self.handle, d_M), 'igx_solver_set_mass_d')      # (the array changes hands)
        except BaseException:
            lib.igx_dev_free(self._ctx.handle, d_M)
            self._release()
            raise
        MP._solvers.add(self)

    def _level_system(self, MPc, bcs):
        problem, rhs, args, kwargs = self._problem
        return _SymmetricLevelSystem(MPc, problem, rhs, bcs, args=args, **kwargs)

    def set_method(self, method):
        if method != 'cg':
            raise ValueError('MultipatchEigenSystem has no linear solve: its method stays cg')
        _DeviceSystem.set_method(self, method)

    def _precond_key(self, precond):
        if precond == 'schwarz':
            raise ValueError("the Schwarz preconditioner is not offered for eigenproblems (in the host model it takes as many "
                             "iterations as Jacobi): use precond='mg'")
        return super()._precond_key(precond)

    def _check_solve_precond(self, precond):
        self._precond_key(precond)

    def _eig_solve_info(self, key):
        self._mg_solve_info(key)

    def _auto_precond(self):
        """'mg' if a hierarchy of at least two levels is set up or ``set_multigrid()`` makes one, else 'jacobi'."""
        if self._mg is None:
            try:
                self.set_multigrid()
            except ValueError:
                return 'jacobi'
        if len(self._mg['systems']) < 2:
            self._drop_multigrid()
            return 'jacobi'
        return 'mg'

    def set_precond(self, precond):
        """The preconditioner of ``solve`` and of ``apply_precond`` on blocks: 'auto', 'mg', 'jacobi' or None.  'auto' is 'mg' when
        ``set_multigrid()`` succeeds with at least one coarser level (the fixed dofs a union of whole patch sides, injective
        maps), else 'jacobi'; 'mg' alone calls ``set_multigrid()`` with its defaults if no hierarchy is set up."""
        def install(h, key):
            if key == 'mg' and self._mg is None:
                self.set_multigrid()
            _lib.check(_lib.load().igx_solver_eig_set_precond(h, self.PRECONDS[key], None, None, None, None, 0),
                       'igx_solver_eig_set_precond')
        return self._switch_eig_precond(precond, install)

    _set_eig_precond = set_precond

    def _drop_multigrid(self):
        super()._drop_multigrid()
        if getattr(self, '_eig_precond', None) == 'mg':
            self._eig_precond = False

    def set_multigrid(self, levels=None, coarse=None, smooth_steps=1, coarse_max=2048, block_rows=None):
        # (documented by MultipatchSystem.set_multigrid, which inspect.getdoc and help() show for it)
        super().set_multigrid(levels, coarse, smooth_steps, coarse_max, block_rows)
        if self._eig_precond == 'mg':
            self._eig_precond = False             # (checked again against the new hierarchy)
        return self

    def solve(self, k=6, tol=1e-8, maxiter=200, precond='auto', block=None, X0=None, seed=0, timed=False):
        """Block LOBPCG (``lobpcg_loop``) to ``||K x_i - lam_i M x_i|| <= tol ||K x_i||`` for the k lowest pairs; arguments and
        ``info`` as ``EigenSystem.solve``.  `precond`: see ``set_precond``.  The V-cycle is applied column by column (`block`
        cycles per iteration).  Deterministic on injective maps: the same inputs give the same bits."""
        return self._eig_solve(k, tol, maxiter, precond, block, X0, seed, timed)

    def vcycle(self, r):
        """One V-cycle of the hierarchy on the vector `r` of all dofs (``MultipatchSystem.apply_precond(r, 'mg')``)."""
        h = self._live()
        if self._mg is None:
            self.set_multigrid()
        if self._precond != 'mg':
            _lib.check(_lib.load().igx_solver_set_precond(h, _lib.IGX_PRECOND_MG, None, None, None, None, 0), 'igx_solver_set_precond')
            self._precond = 'mg'
        return self._device_op(_lib.load().igx_solver_precond_d, 'igx_solver_precond_d', r)

    def schwarz_setup(self):
        raise ValueError("the Schwarz preconditioner is not offered for eigenproblems: use precond='mg'")



################################################################################
# Local multigrid for hierarchical spline spaces (pyiga/solvers.py:174-324; csrc/hmg.hip)
################################################################################

HMG_SMOOTHERS = ('gs', 'forward_gs', 'backward_gs', 'symmetric_gs')
_ip32 = C.POINTER(C.c_int32)


def _csr32(A):
    """`A` as scipy CSR with ascending columns in every row and int32 index arrays (explicit zeros stay)."""
    A = scipy.sparse.csr_matrix(A)
    if not A.has_sorted_indices:
        A = A.copy()
        A.sort_indices()
    if A.nnz >= 2 ** 31:
        raise ValueError('matrix with %d entries: int32 positions' % A.nnz)
    return scipy.sparse.csr_matrix((np.asarray(A.data, dtype=np.float64), A.indices.astype(np.int32), A.indptr.astype(np.int32)), shape=A.shape)


def _ones_pattern(indptr, indices, shape):
    return scipy.sparse.csr_matrix((np.ones(len(indices), dtype=np.int64), indices, indptr), shape=shape)


def triple_product_pattern(indptr, indices, P):
    """``(indptr, indices)`` (int32, ascending columns) of the structural pattern of ``P^T A P``: the product of the 0/1 matrices
    of the stored entries of `A` (given by its pattern) and `P`, so that no entry is lost to cancellation."""
    P = scipy.sparse.csr_matrix(P)
    Pb = _ones_pattern(P.indptr, P.indices, P.shape)
    Cp = scipy.sparse.csr_matrix(Pb.T @ _ones_pattern(indptr, indices, (P.shape[0], P.shape[0])) @ Pb)
    Cp.sort_indices()
    return Cp.indptr.astype(np.int32), Cp.indices.astype(np.int32)


def colour_order(indptr, indices, ind):
    """The rows `ind` of the pattern sorted by (colour, index) and the colour offsets: the first-fit colouring in ascending
    index order over the pattern restricted to the set (``first_fit_colouring`` with the set as its mask)."""
    ind = np.asarray(ind, dtype=np.int64)
    n = len(indptr) - 1
    mask = np.zeros(n, dtype=np.uint8)
    mask[ind] = 1
    if int(mask.sum()) != ind.size:
        raise ValueError('an index list names a dof twice')
    colour, nc = first_fit_colouring(indptr, indices, mask)
    rows = np.flatnonzero(mask)
    rows = rows[np.argsort(colour[rows], kind='stable')]
    coff = np.concatenate(([0], np.cumsum(np.bincount(colour[rows], minlength=nc)))).astype(np.int32)
    return rows.astype(np.int32), coff


class _DeviceBytes:
    """Host arrays of any dtype copied to device memory, freed together."""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def alloc(self, nbytes):
        ptr = _lib.load().igx_dev_alloc(self.ctx.handle, max(int(nbytes), 8))
        if not ptr:
            raise _lib.IgxError('igx_dev_alloc failed: ' + _lib.last_error())
        self.ptrs.append(ptr)
        return ptr

    def upload(self, a):
        a = np.ascontiguousarray(a)
        ptr = self.alloc(a.nbytes)
        if a.nbytes:
            _lib.check(_lib.load().igx_dev_upload(self.ctx.handle, ptr, a.ctypes.data, a.nbytes), 'igx_dev_upload')
        return ptr

    def free(self):
        if getattr(self.ctx, 'handle', None):
            _lib.check(_lib.load().igx_sync(self.ctx.handle), 'igx_sync')           # (nothing in flight may read what goes now)
            for p in self.ptrs:
                _lib.load().igx_dev_free(self.ctx.handle, p)
        self.ptrs = []


def csr_rap_device(ctx, A, PT, Cpat, d_a_vals=None, max_blocks=None):
    """The values of ``PT A PT^T`` on the pattern `Cpat` = ``(indptr, indices)``, computed on the device (``igx_csr_rap_d``) and
    left there: returns ``(buffers, pointer)``; the caller frees `buffers`.  `A`: scipy CSR, or with `d_a_vals` (device values)
    only its pattern is read.  `PT`: the transposed prolongation as scipy CSR."""
    A, PT = _csr32(A), _csr32(PT)
    buf = _DeviceBytes(ctx)
    try:
        cip, cix = np.ascontiguousarray(Cpat[0], dtype=np.int32), np.ascontiguousarray(Cpat[1], dtype=np.int32)
        d_cv = buf.alloc(8 * cix.size)
        tmax = int(np.diff(PT.indptr).max()) if PT.shape[0] else 0
        _lib.check(_lib.load().igx_csr_rap_d(
            ctx.handle, A.shape[0], PT.shape[0], buf.upload(A.indptr), buf.upload(A.indices), d_a_vals or buf.upload(A.data), A.nnz,
            buf.upload(PT.indptr), buf.upload(PT.indices), buf.upload(PT.data), PT.nnz, tmax, buf.upload(cip), buf.upload(cix), d_cv, cix.size,
            int(max_blocks or 0)), 'igx_csr_rap_d')
        _lib.check(_lib.load().igx_sync(ctx.handle), 'igx_sync')
    except BaseException:
        buf.free()
        raise
    return buf, d_cv


def csr_rap(A, P, max_blocks=None, device=None):
    """``P^T A P`` as scipy CSR with the values computed on the device (``igx_csr_rap_d``) on the structural pattern."""
    ctx = _lib.context(device)
    A, P = _csr32(A), scipy.sparse.csr_matrix(P)
    cip, cix = triple_product_pattern(A.indptr, A.indices, P)
    buf, d_cv = csr_rap_device(ctx, A, P.T, (cip, cix), max_blocks=max_blocks)
    try:
        vals = np.empty(cix.size)
        if vals.size:
            _lib.check(_lib.load().igx_dev_download(ctx.handle, vals.ctypes.data, d_cv, vals.nbytes), 'igx_dev_download')
    finally:
        buf.free()
    return scipy.sparse.csr_matrix((vals, cix, cip), shape=(P.shape[1], P.shape[1]))


def csr_rect_spmv(M, x, y=None, max_blocks=None, device=None):
    """``M x`` (or ``y + M x``) for a rectangular sparse matrix, computed on the device (``igx_csr_rect_spmv_d``)."""
    ctx = _lib.context(device)
    M = _csr32(M)
    x = _lib.f64(x)
    if x.shape != (M.shape[1],):
        raise ValueError('vector of shape %r for a matrix of shape %r' % (x.shape, M.shape))
    buf = _DeviceBytes(ctx)
    try:
        d_y = buf.upload(np.zeros(M.shape[0]) if y is None else _lib.f64(y))
        _lib.check(_lib.load().igx_csr_rect_spmv_d(ctx.handle, M.shape[0], M.shape[1], buf.upload(M.indptr), buf.upload(M.indices),
                                                   buf.upload(M.data), M.nnz, int(np.diff(M.indptr).max()) if M.shape[0] else 0,
                                                   buf.upload(x), d_y, int(y is not None), int(max_blocks or 0)), 'igx_csr_rect_spmv_d')
        out = np.empty(M.shape[0])
        if out.size:
            _lib.check(_lib.load().igx_dev_download(ctx.handle, out.ctypes.data, d_y, out.nbytes), 'igx_dev_download')
    finally:
        buf.free()
    return out


class HMultigrid:
    """The virtual hierarchy of a hierarchical spline space on the device (``igx_hmg``): per level the Galerkin matrix, the
    prolongation and its transpose, and the smoothing set as row lists by colour; on level 0 the dense inverse.

    Args:
        A: the matrix of the finest level, scipy sparse (uploaded once), or a triple ``(indptr, indices, d_values)`` whose values
            are on the device already (copied there)
        Ps: the prolongations between consecutive levels, coarsest first (``HSpace.virtual_hierarchy_prolongators``)
        lv_inds: per level the dofs the smoother visits (level 0: the dofs of the direct solve).  The lists are honoured as
            sets: a sweep runs in (colour, index) order of the first-fit colouring of the level's matrix restricted to the set,
            which is a Gauss-Seidel sweep in that order (rows of one colour do not couple)
        free: the dofs the residual norm of a solve runs over (default: all)
        smoother: ``'gs'`` (forward sweeps before, backward after the coarse correction), ``'forward_gs'``, ``'backward_gs'``
            or ``'symmetric_gs'``; ``'exact'`` needs a direct solve per level and raises NotImplementedError
        coarse_max: level 0 is solved with a dense inverse formed on the host; more dofs than this raise ValueError
        block_rows: a smoothing set of at most this many rows sweeps in one launch of one block (default ``MG_BLOCK_ROWS``),
            a larger one with one launch per colour
        max_blocks: cap of the grid of the triple-product kernel (None: the library's default); the values do not depend on it
    """

    def __init__(self, A, Ps, lv_inds, free=None, smoother='gs', smooth_steps=2, coarse_max=2048, block_rows=None, max_blocks=None,
                 device=None):
        if smoother == 'exact':
            raise NotImplementedError("smoother='exact' needs a direct solve on every level and is not available on the device; "
                                      "use 'gs', 'forward_gs', 'backward_gs' or 'symmetric_gs'")
        if smoother not in HMG_SMOOTHERS:
            raise ValueError('unknown smoother %r (one of %s)' % (smoother, ', '.join(HMG_SMOOTHERS)))
        smooth_steps = int(smooth_steps)
        if not 1 <= smooth_steps <= 16:
            raise ValueError('smooth_steps must be 1 .. 16')
        Ps = [_csr32(P) for P in Ps]
        L = len(Ps) + 1
        if not 1 <= L <= _lib.IGX_HMG_MAX_LEVELS or len(lv_inds) != L:
            raise ValueError('%d prolongations and %d index lists: one list per level, at most %d levels' % (len(Ps), len(lv_inds), _lib.IGX_HMG_MAX_LEVELS))
        if isinstance(A, tuple):
            indptr, indices, d_vals = A
            indptr, indices = np.ascontiguousarray(indptr, dtype=np.int32), np.ascontiguousarray(indices, dtype=np.int32)
            host = None
        else:
            host = _csr32(A)
            if host.shape[0] != host.shape[1]:
                raise ValueError('the matrix is not square')
            indptr, indices, d_vals = host.indptr, host.indices, None
        n = indptr.size - 1
        inds = [np.asarray(ix, dtype=np.int64).ravel() for ix in lv_inds]
        if inds[0].size > int(coarse_max):
            raise ValueError('level 0 keeps %d dofs for the direct solve, more than coarse_max = %d' % (inds[0].size, int(coarse_max)))
        sizes = [P.shape[1] for P in Ps] + [n]
        for l, P in enumerate(Ps):
            if P.shape[0] != sizes[l + 1]:
                raise ValueError('prolongation %d has %d rows, the level above %d dofs' % (l, P.shape[0], sizes[l + 1]))
        for l, ix in enumerate(inds):
            if ix.size and (ix.min() < 0 or ix.max() >= sizes[l]):
                raise ValueError('an index of level %d is outside its %d dofs' % (l, sizes[l]))
        # the structural patterns of the Galerkin chain, host
        pats = [None] * L
        pats[L - 1] = (indptr, indices)
        for l in range(L - 1, 0, -1):
            pats[l - 1] = triple_product_pattern(pats[l][0], pats[l][1], Ps[l - 1])
        self.n, self.numlevels, self.sizes = n, L, sizes
        self.smoother, self.smooth_steps = smoother, smooth_steps
        self.lv_inds, self._pats = inds, pats
        self._ctx = _lib.context(device)
        lib = _lib.load()
        h = C.c_void_p()
        _lib.check(lib.igx_hmg_create(self._ctx.handle, L, C.byref(h)), 'igx_hmg_create')
        self.handle = h
        tmp = _DeviceBytes(self._ctx)
        try:
            if d_vals is None:
                d_vals = tmp.upload(host.data)
            for l in range(L):
                ip, ix = pats[l]
                _lib.check(lib.igx_hmg_set_matrix(h, l, sizes[l], ip.ctypes.data_as(_ip32), ix.ctypes.data_as(_ip32), d_vals if l == L - 1 else None),
                           'igx_hmg_set_matrix')
            for l in range(1, L):
                P = Ps[l - 1]
                _lib.check(lib.igx_hmg_set_transfer(h, l, sizes[l - 1], P.indptr.ctypes.data_as(_ip32), P.indices.ctypes.data_as(_ip32), _lib.dptr(P.data)),
                           'igx_hmg_set_transfer')
            for l in range(L - 1, 0, -1):
                _lib.check(lib.igx_hmg_galerkin(h, l, int(max_blocks or 0)), 'igx_hmg_galerkin')
            block_rows = MG_BLOCK_ROWS if block_rows is None else int(block_rows)
            self.colours = [None] * L
            for l in range(1, L):
                rows, coff = colour_order(pats[l][0], pats[l][1], inds[l])
                self.colours[l] = (rows, coff)
                _lib.check(lib.igx_hmg_set_smoother(h, l, coff.size - 1, coff.ctypes.data_as(_ip32), rows.ctypes.data_as(_ip32), block_rows),
                           'igx_hmg_set_smoother')
            # level 0: the matrix on its dofs, inverted on the host
            A0 = self.level_matrix(0)
            i0 = inds[0]
            inv = np.ascontiguousarray(scipy.linalg.inv(A0[i0][:, i0].toarray())) if i0.size else np.zeros((0, 0))
            i032 = np.ascontiguousarray(i0, dtype=np.int32)
            _lib.check(lib.igx_hmg_set_inverse(h, i032.ctypes.data_as(_ip32), i0.size, _lib.dptr(inv)), 'igx_hmg_set_inverse')
            mask = np.ones(n, dtype=np.uint8)
            if free is not None:
                mask[:] = 0
                mask[np.asarray(free, dtype=np.int64)] = 1
            self.free = np.flatnonzero(mask)
            _lib.check(lib.igx_hmg_set_free(h, mask.ctypes.data_as(C.POINTER(C.c_uint8))), 'igx_hmg_set_free')
            _lib.check(lib.igx_hmg_set_options(h, _lib.HMG_SMOOTHERS[smoother], smooth_steps), 'igx_hmg_set_options')
        except BaseException:
            self.close()
            raise
        finally:
            tmp.free()
        self.info = None

    def _live(self):
        if not getattr(self, 'handle', None):
            raise _lib.IgxError('the hierarchy was closed')
        return self.handle

    def close(self):
        h, self.handle = getattr(self, 'handle', None), None
        if h and getattr(self._ctx, 'handle', None):
            _lib.load().igx_hmg_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def level_matrix(self, l):
        """The matrix of level `l` (0: coarsest), downloaded as scipy CSR on the structural pattern of the Galerkin product."""
        ip, ix = self._pats[l]
        vals = np.empty(ix.size)
        _lib.check(_lib.load().igx_hmg_level_values(self._live(), int(l), _lib.dptr(vals)), 'igx_hmg_level_values')
        return scipy.sparse.csr_matrix((vals, ix, ip), shape=(self.sizes[l], self.sizes[l]))

    def level_info(self, l):
        out = _lib.HmgLevel()
        _lib.check(_lib.load().igx_hmg_level_info(self._live(), int(l), C.byref(out)), 'igx_hmg_level_info')
        return {k: getattr(out, k) for k, _ in out._fields_ if k != 'reserved'}

    def _vec(self, v, what):
        v = _lib.f64(v)
        if v.shape != (self.n,):
            raise ValueError('%s has shape %r, the finest level %d dofs' % (what, v.shape, self.n))
        return v

    # -- device vectors in and out (HierarchicalSystem keeps its vectors there)
    def spmv_d(self, d_x, d_y, d_b=None, sign=1.0):
        """``d_y = [d_b +] sign A d_x`` on the finest level."""
        _lib.check(_lib.load().igx_hmg_spmv_d(self._live(), d_x.ptr, None if d_b is None else d_b.ptr, float(sign), d_y.ptr), 'igx_hmg_spmv_d')

    def cycle_d(self, d_f, d_x):
        _lib.check(_lib.load().igx_hmg_cycle_d(self._live(), d_f.ptr, d_x.ptr), 'igx_hmg_cycle_d')

    def solve_d(self, d_f, d_x, method='iterate', tol=1e-8, maxiter=5000):
        if method not in _lib.HMG_METHODS:
            raise ValueError("unknown method %r ('iterate' or 'cg')" % (method,))
        if method == 'cg' and self.smoother not in ('gs', 'symmetric_gs'):
            raise ValueError("method='cg' needs a symmetric cycle: smoother 'gs' or 'symmetric_gs', not %r" % self.smoother)
        info = _lib.HmgInfo()
        _lib.check(_lib.load().igx_hmg_solve_d(self._live(), _lib.HMG_METHODS[method], d_f.ptr, d_x.ptr, float(tol), int(maxiter), C.byref(info)),
                   'igx_hmg_solve_d')
        self.info = dict(info.as_dict(), method=method)
        return self.info

    # -- host vectors
    def spmv(self, x):
        d_x, d_y = DeviceArray.from_host(self._ctx, self._vec(x, 'x')), DeviceArray(self._ctx, self.n)
        self.spmv_d(d_x, d_y)
        return d_y.download()

    def cycle(self, f, x=None):
        """One cycle with the right-hand side `f` from the guess `x` (default: zero): the reference's ``step``."""
        d_f = DeviceArray.from_host(self._ctx, self._vec(f, 'f'))
        d_x = DeviceArray.from_host(self._ctx, np.zeros(self.n) if x is None else self._vec(x, 'x'))
        self.cycle_d(d_f, d_x)
        return d_x.download()

    def solve(self, f, method='iterate', tol=1e-8, maxiter=5000):
        """``A x = f`` from ``x = 0``; the statistics are left in ``info``."""
        d_f, d_x = DeviceArray.from_host(self._ctx, self._vec(f, 'f')), DeviceArray(self._ctx, self.n)
        self.solve_d(d_f, d_x, method=method, tol=tol, maxiter=maxiter)
        return d_x.download()

    def profile(self, f, reps=5):
        """Device time of one cycle by phase (events after every phase; mean over `reps` cycles on a zero guess)."""
        d_f, d_x = DeviceArray.from_host(self._ctx, self._vec(f, 'f')), DeviceArray.from_host(self._ctx, np.zeros(self.n))
        out = _lib.HmgProfile()
        _lib.check(_lib.load().igx_hmg_profile_d(self._live(), d_f.ptr, d_x.ptr, int(reps), C.byref(out)), 'igx_hmg_profile_d')
        L = self.numlevels
        return dict(levels=L, launches=out.launches, total_ms=out.total_ms, coarse_ms=out.coarse_ms, smooth_ms=list(out.smooth_ms)[:L],
                    residual_ms=list(out.residual_ms)[:L], transfer_ms=list(out.transfer_ms)[:L])


def _hmg_finest(hs, A, ctx, keep, max_blocks=None):
    """The matrix of the finest level for `hs` from `A`: a scipy matrix as it is, or an ``HDiscretization`` whose HB values are on
    the device -- as ``(indptr, indices, d_values)``; for a THB space ``T^T A_hb T`` is formed there (buffers go to `keep`)."""
    from .hierarchical import HDiscretization
    if not isinstance(A, HDiscretization):
        return A
    if A.hs is not hs:
        raise ValueError('the discretisation belongs to another space')
    if not A.values_d:
        raise ValueError('the discretisation holds no values on the device: call assemble_hb_values() or assemble_matrix() first')
    if not hs.truncate:
        return (A.indptr, A.indices, A.values_d)
    T = _csr32(hs.thb_to_hb())
    Ahb = scipy.sparse.csr_matrix((np.zeros(A.indices.size), A.indices, A.indptr), shape=(hs.numdofs, hs.numdofs))
    cip, cix = triple_product_pattern(A.indptr, A.indices, T)
    buf, d_cv = csr_rap_device(ctx, Ahb, T.T, (cip, cix), d_a_vals=A.values_d, max_blocks=max_blocks)
    keep.append(buf)
    return (cip, cix, d_cv)


def local_mg_step(hs, A, f, Ps, lv_inds, smoother='symmetric_gs', smooth_steps=2, **kwargs):
    """A callable ``step(x)`` that performs one cycle of the local multigrid method on the device (pyiga/solvers.py:174-241).

    The index lists `lv_inds` are honoured as sets: every sweep runs in (colour, index) order of the first-fit colouring of the
    level's Galerkin matrix restricted to the set -- one launch or one barrier per colour is exactly the sequential Gauss-Seidel
    sweep in that order -- not in the order of the lists.  ``smoother='exact'`` raises NotImplementedError.  The hierarchy is
    the attribute ``step.hierarchy`` (an :class:`HMultigrid`; ``close()`` frees it).  Keywords: those of :class:`HMultigrid`."""
    ctx = _lib.context(kwargs.get('device'))
    keep = []
    try:
        if smoother == 'exact':
            raise NotImplementedError("smoother='exact' needs a direct solve on every level and is not available on the device")
        H = HMultigrid(_hmg_finest(hs, A, ctx, keep, kwargs.get('max_blocks')), Ps, lv_inds, smoother=smoother, smooth_steps=smooth_steps, **kwargs)
    finally:
        for b in keep:
            b.free()
    d_f = DeviceArray.from_host(ctx, H._vec(f, 'f'))

    def step(x):
        d_x = DeviceArray.from_host(ctx, H._vec(x, 'x'))
        H.cycle_d(d_f, d_x)
        return d_x.download()
    step.hierarchy = H
    return step


def solve_hmultigrid(hs, A, f, strategy='cell_supp', smoother='gs', smooth_steps=2, tol=1e-8, maxiter=5000, method='iterate',
                     coarse_max=2048, max_blocks=None, block_rows=None):
    """Solves a scalar problem in a hierarchical spline space by local multigrid on the device (pyiga/solvers.py:285-324).

    `A`: the matrix in the basis of `hs`, scipy sparse (uploaded once), or an ``HDiscretization`` of `hs` whose values are on
    the device.  `strategy`: the smoothing sets, ``'new'``, ``'trunc'``, ``'func_supp'`` or ``'cell_supp'``.  `smoother`: see
    :class:`HMultigrid`.  ``method='iterate'`` repeats the cycle until the residual over the non-Dirichlet dofs has dropped by
    `tol`; ``method='cg'`` uses the cycle as the preconditioner of CG (symmetric positive definite matrices, smoother ``'gs'``
    or ``'symmetric_gs'``; else ValueError).  Returns ``(x, iterations)``, the count ``numpy.inf`` when not converged."""
    if smoother == 'exact':
        raise NotImplementedError("smoother='exact' needs a direct solve on every level and is not available on the device")
    if method not in _lib.HMG_METHODS:
        raise ValueError("unknown method %r ('iterate' or 'cg')" % (method,))
    if method == 'cg' and smoother not in ('gs', 'symmetric_gs'):
        raise ValueError("method='cg' needs a symmetric cycle: smoother 'gs' or 'symmetric_gs', not %r" % (smoother,))
    ctx = _lib.context(None)
    keep = []
    try:
        H = HMultigrid(_hmg_finest(hs, A, ctx, keep, max_blocks), hs.virtual_hierarchy_prolongators(), hs.indices_to_smooth(strategy),
                       free=hs.non_dirichlet_dofs(), smoother=smoother, smooth_steps=smooth_steps, coarse_max=coarse_max,
                       block_rows=block_rows, max_blocks=max_blocks)
    finally:
        for b in keep:
            b.free()
    try:
        x = H.solve(f, method=method, tol=tol, maxiter=maxiter)
        return x, (H.info['iterations'] if H.info['converged'] else np.inf)
    finally:
        H.close()


class HierarchicalSystem:
    """The Dirichlet problem of a scalar form over a hierarchical spline space, assembled and solved on the device.

    ``HierarchicalSystem(hs, problem, rhs, geo=geo, lift=None, **inputs)``: `problem` a bilinear form string, `rhs` a linear one
    (or None for ``'f * v * dx'``), `inputs` the named inputs of both.  The matrix is assembled with ``HDiscretization`` and its
    values stay in device memory; for a THB space ``T^T A T`` and ``T^T rhs`` are formed there.  The Dirichlet sides are those
    of ``hs.bdspecs``.  `lift`: canonical coefficients that are non-zero on Dirichlet dofs only; the system solves for
    ``f - A lift`` (formed on the device) and adds the lift back.  Only the right-hand side goes up and only the solution comes
    down.  Limits: scalar forms on one patch in 2D or 3D (as ``HDiscretization``); ``method='cg'`` needs a symmetric positive
    definite matrix; ``smoother='exact'`` is refused; level 0 keeps at most `coarse_max` dofs; the pattern of every triple
    product is built on the host."""

    def __init__(self, hs, problem, rhs=None, geo=None, lift=None, max_blocks=None, **inputs):
        from .hierarchical import HDiscretization
        if geo is None:
            raise ValueError("required input parameter 'geo' missing")
        self.hs, self.n = hs, hs.numdofs
        self.max_blocks = max_blocks
        self._ctx = _lib.context(None)
        self._H, self._key = None, None
        self._bufs = []
        self.info = None
        if lift is not None:
            lift = _lib.f64(lift)
            if lift.shape != (self.n,):
                raise ValueError('lift has shape %r, the space %d dofs' % (lift.shape, self.n))
            if np.any(lift[hs.non_dirichlet_dofs()] != 0.0):
                raise ValueError('lift must vanish on the non-Dirichlet dofs')
        self.lift = lift
        self.geo, self.problem, self.rhs_form, self.inputs = geo, problem, rhs, dict(inputs)     # (read by error_norms / estimate)
        disc = HDiscretization(hs, problem, dict(inputs, geo=geo), max_blocks=max_blocks)
        try:
            disc.assemble_hb_values()
            keep = []
            self._matrix = _hmg_finest(hs, disc, self._ctx, keep, max_blocks)
            if keep:                                  # (THB: the product owns its values; the HB values may go)
                self._bufs += keep
            else:                                     # (HB: the values change hands)
                self._owned, disc.values_d = disc.values_d, None
            # the right-hand side: assembled per level on the device, gathered to canonical order (HB functionals)
            trunc, disc.truncate = disc.truncate, False
            try:
                b = disc.assemble_rhs(rhs)
            finally:
                disc.truncate = trunc
        finally:
            disc.close()
        self._d_f = DeviceArray(self._ctx, self.n)
        if hs.truncate:
            TT = _csr32(hs.thb_to_hb().T)
            tmp = _DeviceBytes(self._ctx)
            try:
                _lib.check(_lib.load().igx_csr_rect_spmv_d(self._ctx.handle, self.n, self.n, tmp.upload(TT.indptr), tmp.upload(TT.indices), tmp.upload(TT.data),
                                                           TT.nnz, int(np.diff(TT.indptr).max()), tmp.upload(b), self._d_f.ptr, 0, 0), 'igx_csr_rect_spmv_d')
            finally:
                tmp.free()
        else:
            self._d_f.upload(b)

    _owned = None

    def _hierarchy(self, strategy, smoother, smooth_steps, coarse_max, block_rows):
        key = (strategy, smoother, int(smooth_steps), int(coarse_max), block_rows)
        if self._H is None or self._key != key:
            if self._H is not None:
                self._H.close()
                self._H = None
            hs = self.hs
            self._H = HMultigrid(self._matrix, hs.virtual_hierarchy_prolongators(), hs.indices_to_smooth(strategy),
                                 free=hs.non_dirichlet_dofs(), smoother=smoother, smooth_steps=smooth_steps, coarse_max=coarse_max,
                                 block_rows=block_rows, max_blocks=self.max_blocks)
            self._key = key
        return self._H

    def setup(self, strategy='cell_supp', smoother='gs', smooth_steps=2, coarse_max=2048, block_rows=None):
        """Builds the hierarchy (kept until other options are asked for); ``solve`` does it on demand."""
        if self._matrix is None:
            raise _lib.IgxError('the system was closed')
        self._hierarchy(strategy, smoother, smooth_steps, coarse_max, block_rows)
        return self

    def solve(self, strategy='cell_supp', smoother='gs', method='cg', tol=1e-8, maxiter=5000, smooth_steps=2, coarse_max=2048, block_rows=None):
        """The solution in canonical order (with the lift added back); the statistics are left in ``info``."""
        if smoother == 'exact':
            raise NotImplementedError("smoother='exact' needs a direct solve on every level and is not available on the device")
        if method == 'cg' and smoother not in ('gs', 'symmetric_gs'):
            raise ValueError("method='cg' needs a symmetric cycle: smoother 'gs' or 'symmetric_gs', not %r" % (smoother,))
        self.setup(strategy, smoother, smooth_steps, coarse_max, block_rows)
        H = self._H
        d_f = self._d_f
        if self.lift is not None:                     # f - A g: one product on the device
            d_g, d_f = DeviceArray.from_host(self._ctx, self.lift), DeviceArray(self._ctx, self.n)
            H.spmv_d(d_g, d_f, d_b=self._d_f, sign=-1.0)
        d_x = DeviceArray(self._ctx, self.n)
        self.info = H.solve_d(d_f, d_x, method=method, tol=tol, maxiter=maxiter)
        x = d_x.download()
        return x if self.lift is None else x + self.lift

    @property
    def hierarchy(self):
        """The :class:`HMultigrid` of the last ``setup`` / ``solve`` (None before)."""
        return self._H

    def rhs(self):
        """The right-hand side in the basis of the space, downloaded."""
        return self._d_f.download()

    def spmv(self, x):
        return self.setup()._H.spmv(x) if self._H is None else self._H.spmv(x)

    def cycle(self, r):
        """One cycle from a zero guess on `r` with the hierarchy of the last ``setup`` / ``solve`` (default options else)."""
        return (self.setup()._H if self._H is None else self._H).cycle(r)

    def level_matrix(self, l):
        return (self.setup()._H if self._H is None else self._H).level_matrix(l)

    # -- error norms and the residual estimator, level by level on the device
    def _level_sums(self, u, nk, sums):
        """The per-cell sums of `nk` quantities over the active cells, ``(nk, total_active_cells)`` in the order of
        ``hs.active_cells(flat=True)``: per level with active cells one ``DevicePatch`` on the level's knot vectors, the level
        coefficients ``level_restriction(lv) u_hb`` formed on the device, ``sums(patch, d_coeffs, d_elem)`` writing the
        ``(nk, numspans)`` element sums of the whole level to `d_elem`, and the gather of the active cells.  Only the dofs go up
        (unless `u` is a ``DeviceArray``) and only the per-cell array comes down."""
        from .assemblers import DevicePatch
        hs, ctx, lib = self.hs, self._ctx, _lib.load()
        if isinstance(u, DeviceArray):
            if u.n != self.n:
                raise ValueError('%d coefficients, the space has %d dofs' % (u.n, self.n))
            d_u = u
        else:
            c = _lib.f64(u.coeffs if hasattr(u, 'coeffs') else u)
            if c.shape != (self.n,):
                raise ValueError('coefficients of shape %r, the space has %d dofs' % (c.shape, self.n))
            d_u = DeviceArray.from_host(ctx, c)
        ncells = hs.total_active_cells
        d_out = DeviceArray(ctx, nk * ncells)
        tmp = _DeviceBytes(ctx)
        own = [d_out] + ([] if d_u is u else [d_u])          # freed below, not left to the collector

        def spmv(M, d_x, d_y):
            M = _csr32(M)
            _lib.check(lib.igx_csr_rect_spmv_d(ctx.handle, M.shape[0], M.shape[1], tmp.upload(M.indptr), tmp.upload(M.indices), tmp.upload(M.data),
                                               M.nnz, int(np.diff(M.indptr).max()) if M.shape[0] else 0, d_x, d_y, 0, int(self.max_blocks or 0)),
                       'igx_csr_rect_spmv_d')
        try:
            if hs.truncate:                               # THB coefficients -> HB coefficients of the same function
                d_hb = DeviceArray(ctx, self.n)
                own.append(d_hb)
                spmv(hs.thb_to_hb(), d_u.ptr, d_hb.ptr)
                d_u = d_hb
            off = 0
            for lv in range(hs.numlevels):
                act = np.flatnonzero(hs._cact[lv])
                if not act.size:
                    continue
                kvs = hs.knotvectors(lv)
                nelem = hs.mesh(lv).numel
                patch = DevicePatch(kvs, self.geo)
                try:
                    d_c = tmp.alloc(8 * hs.mesh(lv).numbf)
                    spmv(hs.level_restriction(lv), d_u.ptr, d_c)
                    d_elem = patch._dev_buffer('_d_qelem', 8 * nk * nelem)
                    sums(patch, d_c, d_elem)
                    d_idx = tmp.upload(act.astype(np.int64))
                    for k in range(nk):
                        _lib.check(lib.igx_hier_gather_d(ctx.handle, C.c_void_p(d_elem + 8 * k * nelem), nelem, d_idx, act.size,
                                                         C.c_void_p(d_out.ptr + 8 * (k * ncells + off))), 'igx_hier_gather_d')
                    _lib.check(lib.igx_sync(ctx.handle), 'igx_sync')        # (the gather reads what the patch frees next)
                finally:
                    patch.close()
                off += act.size
            return d_out.download().reshape(nk, ncells)
        finally:
            tmp.free()                                    # (waits for the stream first)
            for d in own:
                d.free()

    def error_norms(self, u, exact=None, grad_exact=None, elementwise=False):
        """``(l2, h1)`` of ``u_h - exact`` for the hierarchical spline with the canonical coefficients `u` (a host array, an
        ``HSplineFunc`` or a ``DeviceArray``; THB coefficients for a THB space), as :func:`approx.error_norms`: `exact` and
        `grad_exact` in physical coordinates, `h1` None when `exact` comes without `grad_exact`.  ``elementwise=True``: the flat
        arrays of the squared contributions of the active cells in the order of ``hs.active_cells(flat=True)``; the totals are
        the sums over those cells in that order."""
        from . import approx
        if grad_exact is not None and exact is None:
            raise ValueError('error_norms: grad_exact without exact')
        if self._matrix is None:
            raise _lib.IgxError('the system was closed')
        want_grad = exact is None or grad_exact is not None
        nk = 2 if want_grad else 1
        out = np.empty(2)

        def sums(patch, d_c, d_elem):
            d_exact = approx._exact_arrays(patch, self.geo, exact, grad_exact, True)
            ptrs = (C.c_void_p * 4)()
            for r, e in enumerate(d_exact or ()):
                if e is not None:
                    ptrs[r] = e
            _lib.check(_lib.load().igx_patch_error_sums_d(patch.handle, d_c, 1 if want_grad else 0, ptrs, d_elem, _lib.dptr(out)),
                       'igx_patch_error_sums_d')
        cells = self._level_sums(u, nk, sums)
        if elementwise:
            return cells[0], (cells[1] if want_grad else None)
        return float(np.sqrt(cells[0].sum())), (float(np.sqrt(cells[1].sum())) if want_grad else None)

    def _check_estimate(self):
        from . import assemble
        if self.problem is None or not isinstance(self.problem, str) or self.rhs_form is not None or \
                assemble._normalise_form(self.problem) != assemble._normalise_form('inner(grad(u),grad(v))*dx'):
            raise ValueError("estimate: the residual estimator eta_K = h_K ||f + Lap u_h||_K belongs to the Poisson problem: the system must be built "
                             "with the form 'inner(grad(u),grad(v))*dx' and the default right-hand side 'f * v * dx'")
        for lv in range(self.hs.numlevels):
            if not self.hs._cact[lv].any():
                continue
            for kv in self.hs.knotvectors(lv):
                kn = np.asarray(kv.kv)
                mult = np.unique(kn[kv.p + 1:len(kn) - kv.p - 1], return_counts=True)[1]
                if kv.p < 2 or (mult.size and int(mult.max()) >= kv.p):
                    raise ValueError('estimate: the space of level %d is not C^1 (degree %d, largest interior knot multiplicity %d): the jump terms '
                                     'of the normal derivative across its cell faces would be missing from the estimator'
                                     % (lv, kv.p, int(mult.max()) if mult.size else 0))

    def estimate(self, u, f=None):
        """``(eta, eta2)``: the residual-based a-posteriori estimator of the Poisson problem for the canonical coefficients `u`
        (as :meth:`error_norms`) and its squared cell indicators ``eta_K^2 = h_K^2 ||f + Lap u_h||^2_K``, ``h_K = |K|^(1/dim)``,
        over the active cells in the order of ``hs.active_cells(flat=True)``; ``eta = sqrt(sum(eta2))``.  `f`: the right-hand
        side, a callable of the physical coordinates (default: the system's own input ``f``; anything else: TypeError), taken as
        ``error_norms`` takes `exact`; without one it is zero.

        ValueError unless the system was built with ``inner(grad(u),grad(v))*dx`` and the default right-hand side, and every
        level's space is C^1 (degree >= 2, no interior knot of multiplicity >= p): otherwise jump terms would be missing."""
        from . import approx
        self._check_estimate()
        if self._matrix is None:
            raise _lib.IgxError('the system was closed')
        if f is None:
            f = self.inputs.get('f')
        if f is not None and not callable(f):
            raise TypeError('estimate: the right-hand side f is a callable of the physical coordinates (or None for zero), not %r; '
                            'wrap a constant as  lambda *x: c' % type(f).__name__)
        out = np.empty(2)

        def sums(patch, d_c, d_elem):
            d_f = approx._exact_arrays(patch, self.geo, f, None, True)
            _lib.check(_lib.load().igx_patch_residual_sums_d(patch.handle, d_c, None if d_f is None else d_f[0], d_elem, _lib.dptr(out)),
                       'igx_patch_residual_sums_d')
        cells = self._level_sums(u, 2, sums)
        eta2 = approx.eta2_of_sums(cells, self.hs.dim)
        return float(np.sqrt(eta2.sum())), eta2

    def close(self):
        if self._H is not None:
            self._H.close()
            self._H = None
        for b in self._bufs:
            b.free()
        self._bufs = []
        if self._owned and getattr(self._ctx, 'handle', None):
            _lib.load().igx_dev_free(self._ctx.handle, self._owned)
        self._owned = None
        self._matrix = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def adaptive_solve(hs, geo, f, theta=0.5, strategy='dorfler', max_rounds=10, max_dofs=None, tol=None, lift=None, inplace=False,
                   solve_tol=None, **solve_options):
    """The adaptive loop solve -> estimate -> mark -> refine for the Poisson problem ``-Lap u = f`` with the Dirichlet sides of
    ``hs.bdspecs`` over the hierarchical space `hs`.

    Per round a :class:`HierarchicalSystem` is built and solved (`solve_options`: the keywords of its ``solve``, whose own `tol`
    is given as `solve_tol` here: `tol` is the estimator's), the residual estimator is evaluated (``estimate``), and unless
    ``eta <= tol``, the space has reached `max_dofs` dofs or this was round
    `max_rounds`, the cells picked by ``hierarchical.mark(hs, eta2, theta, strategy)`` are refined with
    ``hs.refine(marked, truncate=hs.truncate)``.  `lift`: None or a callable ``hs -> lift array`` (inhomogeneous Dirichlet data).
    The loop works on ``hs.copy()`` unless `inplace`.  Only the dofs and the per-cell indicators cross the bus.

    Returns ``(hs, u, history)``: the final space, the solution on it (canonical coefficients) and one dict per round with
    ``dofs``, ``cells`` (active cells per level), ``eta``, ``eta2``, ``iterations`` and ``marked`` (the dict given to ``refine``;
    empty in the last round).  Limits: no coarsening; nothing of a round's assembly or solution is reused in the next."""
    from .hierarchical import mark
    if max_rounds < 1:
        raise ValueError('adaptive_solve: max_rounds = %r' % (max_rounds,))
    if solve_tol is not None:
        solve_options = dict(solve_options, tol=solve_tol)
    if not inplace:
        hs = hs.copy()
    history, u = [], None
    for rnd in range(int(max_rounds)):
        S = HierarchicalSystem(hs, 'inner(grad(u),grad(v))*dx', None, geo=geo, lift=None if lift is None else lift(hs), f=f)
        try:
            u = S.solve(**solve_options)
            eta, eta2 = S.estimate(u)
            rec = dict(dofs=hs.numdofs, cells=tuple(int(m.sum()) for m in hs._cact), eta=eta, eta2=eta2, iterations=S.info['iterations'], marked={})
        finally:
            S.close()
        history.append(rec)
        if (tol is not None and eta <= tol) or (max_dofs is not None and hs.numdofs >= max_dofs) or rnd == max_rounds - 1:
            break
        marked = mark(hs, eta2, theta, strategy)
        if not marked:
            break
        rec['marked'] = marked
        hs.refine(marked, truncate=hs.truncate)
    return hs, u, history

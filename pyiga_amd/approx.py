"""Interpolation and L2 projection in tensor-product spline spaces (the part of ``pyiga.approx`` the Dirichlet helpers use,
pyiga/approx.py:14-47, 62-96), and the error norms of a spline given by its dofs."""
import numpy as np
import scipy.sparse.linalg

from . import bspline
from . import utils


def interpolate(kvs, f, geo=None, nodes=None):
    """Coefficients of the interpolant of `f` in the tensor-product B-spline basis `kvs`.

    `f` is a function in parameter coordinates, or in physical coordinates if the geometry map `geo` is given, or an array of
    its values at the nodes (leading axes = the numbers of dofs; `geo` is then ignored).  `nodes`: a tensor grid in the
    parameter domain, by default the Greville abscissae.  Trailing axes of the values (vector-valued `f`) are kept.  One
    collocation solve per axis.
    """
    if isinstance(kvs, bspline.KnotVector):
        kvs = (kvs,)
    kvs = tuple(kvs)
    if nodes is None:
        nodes = [kv.greville() for kv in kvs]
    if isinstance(f, np.ndarray):
        if np.shape(f)[:len(kvs)] != tuple(kv.numdofs for kv in kvs):
            raise ValueError('array f has wrong shape')
        vals = f
    elif geo is not None:
        vals = utils.grid_eval_transformed(f, nodes, geo)
    else:
        vals = utils.grid_eval(f, nodes)
    X = np.array(vals, dtype=float)
    for ax, (kv, nd) in enumerate(zip(kvs, nodes)):
        lu = scipy.sparse.linalg.splu(bspline.collocation(kv, nd).tocsc())
        Y = np.moveaxis(X, ax, 0)
        shape = Y.shape
        X = np.moveaxis(lu.solve(np.ascontiguousarray(Y.reshape(shape[0], -1))).reshape(shape), 0, ax)
    return X


def project_L2(kvs, f, f_physical=False, geo=None):
    """Coefficients of the L2 projection of `f` into the tensor-product B-spline basis `kvs` (pyiga/approx.py:62-96).

    `f` is given in the parameter domain, or in physical coordinates with ``f_physical=True`` (needs `geo`).  Without `geo` the
    load vector is multiplied by ``(x) M_k^-1`` with the device Kronecker apply (trailing value axes of a vector-valued `f`
    allowed).  With `geo` the mass matrix is assembled and solved on the device by CG with the Kronecker product of the 1D
    inverse mass matrices as preconditioner (relative tolerance 1e-12, at most 100 iterations, as the reference).
    A hierarchical space (``hierarchical.HSpace``) as `kvs`: the mass matrix and the load vector are assembled on the device
    (``HDiscretization``) and the system is solved on the host; the result is the coefficient vector in canonical order.
    """
    import sys
    import scipy.linalg
    from . import _lib, assemble, hierarchical
    from .solvers import KronDiagOperator, PatchSystem
    if isinstance(kvs, hierarchical.HSpace):
        from . import geometry
        hs = kvs
        if f_physical:
            assert geo is not None, 'Cannot use physical coordinates without geometry'
        g = geo if geo is not None else geometry.unit_cube(hs.dim)
        # (a function in parametric coordinates is composed with nothing: without geometry the two coordinates coincide)
        if geo is not None and not f_physical:
            raise NotImplementedError('project_L2 into a hierarchical space: f in parametric coordinates together with a geometry')
        disc = hierarchical.HDiscretization(hs, 'u*v*dx', {'geo': g, 'f': f})
        try:
            M = disc.assemble_matrix()
            rhs = disc.assemble_rhs()
        finally:
            disc.close()
        return scipy.sparse.linalg.spsolve(M.tocsc(), rhs)
    if isinstance(kvs, bspline.KnotVector):
        kvs = (kvs,)
    if not isinstance(kvs, (tuple, list)):
        raise NotImplementedError('project_L2: only tensor-product spaces (a sequence of KnotVector)')
    kvs = tuple(kvs)
    rhs = assemble.inner_products(kvs, f, f_physical=f_physical, geo=geo)
    if geo is None:
        assert not f_physical, 'Cannot use physical coordinates without geometry'
        EV = [scipy.linalg.eigh(assemble.bsp_mass_1d(kv).toarray()) for kv in kvs]
        op = KronDiagOperator([U for _, U in EV], [lam for lam, _ in EV], _lib.IGX_KRON_PRODUCT)
        n = int(np.prod([kv.numdofs for kv in kvs]))
        return op.matmat(np.reshape(rhs, (n, -1))).reshape(rhs.shape)
    b = np.ravel(rhs)
    n = int(np.prod([kv.numdofs for kv in kvs]))
    assert b.shape[0] == n, 'L2 projection with geometry only implemented for scalar functions'
    S = PatchSystem(kvs, geo, b, None, kind='mass')
    try:
        x = S.solve(tol=1e-12, maxiter=100, precond='kron')
        if not S.info['converged']:
            print('WARNING: L2 projection - CG did not converge:', S.info['iterations'], file=sys.stderr)
    finally:
        S.close()
    return x.reshape(rhs.shape)


def _trace_exact(exact, grad_exact, dim):
    """C texts of the exact value and (if given) of its `dim` partials, or None when one of them cannot be traced."""
    from . import symbolic
    src = symbolic.trace_function(exact, dim)
    if src is None:
        return None
    srcs = [src]
    if grad_exact is not None:
        try:
            X = symbolic.coordinates(dim)
            val = grad_exact(*(X[..., k] for k in range(dim)))
            if not isinstance(val, (tuple, list)) or len(val) != dim:
                return None
            srcs += [symbolic.c_source(np.broadcast_to(np.asarray(v, dtype=object), (1,) * dim)) for v in val]
        except Exception:
            return None
    return srcs


def _exact_arrays(patch, geo, exact, grad_exact, f_physical):
    """Device pointers of the exact value and of its physical partials over the resident Gauss points of `patch` (None where
    absent): by ONE generated kernel when the functions are traceable and the coordinates the kernel sees are the ones they are
    given in, else sampled on the host and uploaded."""
    from . import _lib, geometry
    if exact is None:
        return None
    dim = patch.dim
    n = 1 + (dim if grad_exact is not None else 0)
    ptrs = None
    # the generated kernels evaluate at the PHYSICAL points of a spline geometry (no geometry: the two coincide)
    if geo is None or (f_physical and isinstance(geo, (bspline.BSplineFunc, geometry.NurbsFunc))):
        srcs = _trace_exact(exact, grad_exact, dim)
        if srcs is not None:
            try:
                ptrs, _ = patch.eval_exprs_inputs(srcs, [], buf='_d_qex')
            except _lib.IgxError as e:                           # (no run-time compiler on this box / not traceable into a kernel: sampled on the host)
                if not _lib.sampled_fallback(e, 'the exact solution of an error norm'):
                    raise
    if ptrs is None:
        grid = tuple(patch.gauss(k)[0] for k in range(dim))
        G = tuple(len(ax) for ax in grid)
        sample = (lambda f: utils.grid_eval_transformed(f, grid, geo)) if (f_physical and geo is not None) else (lambda f: utils.grid_eval(f, grid))
        arrs = [np.broadcast_to(np.asarray(sample(exact), dtype=float), G)]
        if grad_exact is not None:
            g = np.asarray(sample(grad_exact), dtype=float)
            if g.shape != G + (dim,):
                raise ValueError('grad_exact returns the %d physical partials (d/dx first)' % dim)
            arrs += [g[..., k] for k in range(dim)]
        ptrs = patch.upload_fields(arrs, buf='_d_qex')
    return list(ptrs) + [None] * (4 - n)


def error_norms(kvs, geo, u, exact=None, grad_exact=None, f_physical=True, elementwise=False, patch=None):
    """``(l2, h1)``: the L2 norm and the H1 seminorm of ``u_h - exact`` over the geometry `geo` (None: the parameter domain), for
    the spline `u_h` of the tensor-product space `kvs` given by `u` -- a dof array of ``prod(ndofs)`` entries, a scalar
    ``BSplineFunc`` on `kvs`, or an ``operators.DeviceArray`` of the dofs (read where it is).

    ``exact(x, y[, z])`` returns the value, ``grad_exact(x, y[, z])`` the physical partials, d/dx first; with
    ``f_physical=False`` both are given in parametric coordinates.  `h1` is None when `exact` comes without `grad_exact`; without
    `exact` the norms are those of `u_h` itself.  ``elementwise=True``: the two entries are the arrays of the SQUARED element
    contributions, of shape ``numspans``.  `patch`: a ``DevicePatch`` of (kvs, geo) to use instead of setting one up.

    One fused device pass (``igx_patch_error_sums_d``): spline, gradient, difference, square and weight at the Gauss points of
    the ``max(p) + 1`` rule, summed element by element in a fixed order.  2D and 3D.
    """
    from . import assemblers, geometry
    from .operators import DeviceArray
    if isinstance(kvs, bspline.KnotVector):
        kvs = (kvs,)
    kvs = tuple(kvs)
    dim = len(kvs)
    assert dim in (2, 3), 'error_norms: 2D and 3D patches'
    if grad_exact is not None and exact is None:
        raise ValueError('error_norms: grad_exact without exact')
    ndofs = tuple(kv.numdofs for kv in kvs)
    n = int(np.prod(ndofs))
    if isinstance(u, DeviceArray):
        size, c = u.n, None
    else:
        c = np.asarray(u.coeffs if hasattr(u, 'coeffs') else u, dtype=np.float64)
        size = c.size
    if size != n:
        raise ValueError('error_norms: %d dofs, the space has %d' % (size, n))
    want_grad = exact is None or grad_exact is not None
    P = patch if patch is not None else assemblers.DevicePatch(kvs, geo if geo is not None else geometry.unit_cube(dim))
    try:
        d_u = u.ptr if c is None else P.upload_dofs(c.reshape(ndofs), buf='_d_qdofs')
        d_exact = _exact_arrays(P, geo, exact, grad_exact, f_physical)
        res = P.error_sums(d_u, want_grad, d_exact, elementwise=elementwise)
    finally:
        if patch is None:
            P.close()
    if elementwise:
        return res[1][0], (res[1][1] if want_grad else None)
    return float(np.sqrt(res[0])), (float(np.sqrt(res[1])) if want_grad else None)


def eta2_of_sums(sums, dim):
    """``eta_K^2 = h_K^2 sum_K W (f + Lap u_h)^2`` with ``h_K = (sum_K W)^(1/dim)`` from the two element sums of
    ``DevicePatch.residual_sums`` (arrays of any one shape)."""
    return np.power(sums[1], 2.0 / dim) * sums[0]


def residual_estimator(kvs, geo, u, f=None, patch=None):
    """The squared element indicators ``eta_K^2 = h_K^2 ||f + Lap u_h||^2_K`` (shape ``numspans``) of the residual-based
    a-posteriori estimator of the Poisson problem ``-Lap u = f`` for the spline `u_h` of the tensor-product space `kvs` over the
    geometry `geo` (None: the parameter domain); ``h_K = |K|^(1/dim)``.

    `u` as in :func:`error_norms`; `f` is taken as that function takes `exact` (physical coordinates): a traceable callable is
    evaluated by a generated kernel, anything else is sampled on the host and uploaded; None is zero.  One fused device pass
    (``igx_patch_residual_sums_d``: second derivatives of `u_h` and of the geometry map at the Gauss points).  Interior
    residuals only: the jump terms of a space that is not C^1, and Neumann terms, are not included.  2D and 3D.
    """
    from . import assemblers, geometry
    from .operators import DeviceArray
    if isinstance(kvs, bspline.KnotVector):
        kvs = (kvs,)
    kvs = tuple(kvs)
    dim = len(kvs)
    assert dim in (2, 3), 'residual_estimator: 2D and 3D patches'
    ndofs = tuple(kv.numdofs for kv in kvs)
    n = int(np.prod(ndofs))
    if isinstance(u, DeviceArray):
        size, c = u.n, None
    else:
        c = np.asarray(u.coeffs if hasattr(u, 'coeffs') else u, dtype=np.float64)
        size = c.size
    if size != n:
        raise ValueError('residual_estimator: %d dofs, the space has %d' % (size, n))
    P = patch if patch is not None else assemblers.DevicePatch(kvs, geo if geo is not None else geometry.unit_cube(dim))
    try:
        d_u = u.ptr if c is None else P.upload_dofs(c.reshape(ndofs), buf='_d_qdofs')
        d_f = _exact_arrays(P, geo, f, None, True)
        _, elem = P.residual_sums(d_u, None if d_f is None else d_f[0], elementwise=True)
    finally:
        if patch is None:
            P.close()
    return eta2_of_sums(elem, dim)

"""Interpolation in tensor-product spline spaces (the part of ``pyiga.approx`` the Dirichlet helpers use,
pyiga/approx.py:14-47)."""
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
    Hierarchical spaces are not supported.
    """
    import sys
    import scipy.linalg
    from . import _lib, assemble
    from .solvers import KronDiagOperator, PatchSystem
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

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

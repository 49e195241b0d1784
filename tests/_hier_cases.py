"""Case table of the hierarchical-space tests (tests/test_hier_cpu.py, tests/test_hier_gpu.py) and of
tests/golden/make_golden_hier.py.  Written against the interface the reference and this package share (``bspline.make_knots``,
``KnotVector``, ``HSpace``), so the same table builds the spaces on either: the module that provides them is passed in.

id -> (knot vectors as (p, spans, mult) or (knots, p), truncate, disparity, rounds, region, form, numactive, nnz)
The last two columns are what the reference gives (the make script checks them).
"""
import numpy as np

STIFF = 'inner(grad(u),grad(v))*dx'
MASS = 'u*v*dx'
NONSYM = '(inner(grad(u),grad(v)) + inner((1.0,1.0),grad(u))*v)*dx'
COEFF = '(inner(grad(u),grad(v)) + c*u*v)*dx'

NONUNI = ([0, 0, 0, 0, .2, .5, .6, 1, 1, 1, 1.], 3)

CASES = {
    'hb2':       (((2, 4, 1),) * 2, False, np.inf, 3, 'corner', STIFF, (32, 12, 12, 16), 2070),
    'hb2p1':     (((1, 4, 1),) * 2, False, np.inf, 3, 'corner', STIFF, (21, 12, 12, 16), 559),
    'hb2d':      (((3, 6, 1),) * 2, False, np.inf, 2, 'diag', STIFF, (56, 81, 163), 19258),
    'aniso_m2':  (((3, 4, 2), (2, 5, 1)), False, np.inf, 2, 'diag', STIFF, (44, 60, 124), 9542),
    'nonuni':    ((NONUNI, (1, 5, 1)), False, np.inf, 3, 'corner', STIFF, (38, 14, 6, 8), 1246),
    'nonsym':    (((3, 4, 1),) * 2, False, 1, 2, 'corner', NONSYM, (0, 117, 16), None),
    'thb2':      (((3, 4, 1),) * 2, True, 1, 3, 'corner', STIFF, (0, 105, 60, 16), 7542),
    'thb2d':     (((2, 5, 1),) * 2, True, 2, 3, 'diag', STIFF, (0, 120, 106, 260), 18002),
    'thb2inf':   (((2, 6, 1),) * 2, True, np.inf, 3, 'corner', STIFF, (55, 27, 27, 36), 3647),
    'thb_aniso': (((3, 4, 2), (2, 5, 1)), True, np.inf, 3, 'corner', STIFF, (62, 18, 16, 16), 3385),
    'hb3':       (((2, 3, 1),) * 3, False, np.inf, 2, 'corner', STIFF, (124, 7, 8), 7811),
    'thb3':      (((2, 3, 1),) * 3, True, 1, 2, 'corner', STIFF, (0, 511, 8), 39731),
}

EXTRA_FORM_CASES = ('hb2', 'thb2inf', 'hb3')        # mass and the form with a coefficient
AFFINE_CASES = ('hb2', 'thb_aniso', 'hb3')
SOLVE_CASE = 'thb2inf'
EVAL_CASES = ('thb2inf', 'hb2d')
RF_THB_CASES = ('hb2p1',)                          # HB cases whose truncated representation is stored entry by entry too
RF_PROBE_ONLY = ('hb3',)                           # both bases as pattern + probes (3D entry by entry: thb3)
RF_LV1_CASES = ('hb2', 'thb2', 'nonuni')            # represent_fine with lv=, rows=, restrict=


def probe_vectors(n):
    """Two seeded vectors with entries in [-1, 1]: a representation matrix that does not fit into the golden file entry by entry
    is stored as its pattern and its transposed products with these."""
    return np.random.default_rng(20240611).uniform(-1.0, 1.0, (n, 2))


def f_rhs(*X):
    """cos(x) exp(y) (+ z in 3D), physical coordinates."""
    return np.cos(X[0]) * np.exp(X[1]) + (X[2] if len(X) == 3 else 0.0)


def c_coeff(*X):
    return 1.0 + X[0] * X[1]


def region(kind, lv):
    if kind == 'corner':
        return lambda *X: min(X) > 1 - 0.5 ** (lv + 1)
    return lambda *X: abs(X[0] - X[-1]) < 0.5 ** (lv + 1)


def knotvectors(bspline, spec):
    kvs = []
    for s in spec:
        if len(s) == 3:
            kvs.append(bspline.make_knots(s[0], 0., 1., s[1], mult=s[2]))
        else:
            kvs.append(bspline.KnotVector(np.array(s[0], dtype=float), s[1]))
    return tuple(kvs)


def build(bspline, HSpace, name, truncate=None):
    """The space of case `name` and the list of what every refine call returned."""
    spec, tr, disp, rounds, reg = CASES[name][:5]
    kvs = knotvectors(bspline, spec)
    dim = len(kvs)
    hs = HSpace(kvs, truncate=tr if truncate is None else truncate, disparity=disp, bdspecs=[(a, s) for a in range(dim) for s in (0, 1)])
    refined = [hs.refine_region(lv, region(reg, lv)) for lv in range(rounds)]
    return hs, refined


def geometry_of(geometry, dim, affine=False):
    if affine:
        return geometry.unit_square() if dim == 2 else geometry.unit_cube()
    return geometry.bspline_quarter_annulus() if dim == 2 else geometry.twisted_box()


def rel_maxdiff(A, B):
    A = A.toarray() if hasattr(A, 'toarray') else np.asarray(A)
    B = B.toarray() if hasattr(B, 'toarray') else np.asarray(B)
    return abs(A - B).max() / abs(B).max()

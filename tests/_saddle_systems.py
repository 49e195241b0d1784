"""The two Stokes problems of the device tests of the saddle-point solver, built with this package as the reference's solve-stokes
notebook builds its system: the notebook itself at n_el = (6, 4) ('stokes') and the 3D cavity of golden_saddle.npz ('stokes3').
Needs the device (the Dirichlet data is projected with the package's own routines)."""
import numpy as np

from pyiga_amd import assemble, bspline, geometry, solvers


def _lid2(x, y):
    return (x * y * -y, x * y * x)


def _zero2(x, y):
    return (0.0, 0.0)


def _lid3(x, y, z):
    return (x * y * -y, x * y * x, 0.0 * z)


def _zero3(x, y, z):
    return (0.0, 0.0, 0.0)


def problem(name):
    """(kvs_u, kvs_p, geo, bcs with the first pressure dof pinned) of the notebook ('stokes') or of the 3D cavity ('stokes3')."""
    if name == 'stokes':
        geo = geometry.quarter_annulus()
        kvs_u = tuple(bspline.make_knots(3, 0.0, 1.0, n, mult=2) for n in (6, 4))
        kvs_p = tuple(bspline.make_knots(2, 0.0, 1.0, n, mult=1) for n in (6, 4))
        sides = [('bottom', _zero2), ('top', _zero2), ('left', _lid2), ('right', _zero2)]
    else:
        geo = geometry.twisted_box()
        kvs_u = tuple(bspline.make_knots(2, 0.0, 1.0, n, mult=2) for n in (2, 3, 2))
        kvs_p = tuple(bspline.make_knots(1, 0.0, 1.0, n, mult=1) for n in (2, 3, 2))
        sides = [('bottom', _zero3), ('top', _zero3), ('left', _lid3), ('right', _zero3), ('front', _zero3), ('back', _zero3)]
    bcs = assemble.compute_dirichlet_bcs(kvs_u, geo, sides)
    nv = len(kvs_u) * int(np.prod([kv.numdofs for kv in kvs_u]))
    return kvs_u, kvs_p, geo, (np.append(bcs[0], nv), np.append(bcs[1], 0.0)), nv


def system(name, which, **kw):
    kvs_u, kvs_p, geo, bcs, nv = problem(name)
    if which == 'unpinned':
        bcs = (bcs[0][:-1], bcs[1][:-1])
    return solvers.SaddlePointSystem((kvs_u, kvs_p), geo, bcs, **kw), nv

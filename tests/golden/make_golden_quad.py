#!/usr/bin/env python3
"""Golden integrals and error norms from the REAL reference (c-f-h/pyiga).

Build the unmodified reference outside the repository as the header of make_golden.py describes, then

    PYTHONPATH=/tmp/pyiga_oracle python3 tests/golden/make_golden_quad.py

Writes `tests/golden/golden_quad.npz`: inputs and outputs of the reference's public API only (no reference source).

* `assemble.integrate` (pyiga/assemble.py:658-697) in 2D (quarter annulus, p = 3, n = 6) and 3D (line x quarter annulus, p = 2,
  n = 4): a scalar function of the physical coordinates, a function of the parametric ones (with and without the geometry), a
  scalar `BSplineFunc` with random coefficients (stored), a 2-vector function (over the parameter domain: the reference cannot
  weigh a vector-valued function with a geometry), and the identities of the reference's own
  test_integrate (test/test_assemble.py:478-491).
* Error norms through `integrate` as well: an object whose `grid_eval` returns (u_h - g)^2, resp. |grad u_h - grad g|^2 with the
  physical gradient J^-T times `BSplineFunc.grid_jacobian`, for random dofs (stored) and g = sin x cos y [cos z].

The functions are restated in tests/test_quad_gpu.py (`FUNCS`).
"""
import os

import numpy as np

import pyiga
from pyiga import assemble, bspline, geometry

pyiga.set_max_threads(1)
OUT = os.path.dirname(os.path.abspath(__file__))
G = {}


def cylinder():
    return geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.quarter_annulus())


def f_phys(*X):
    return np.sin(X[0]) * np.cos(X[1]) + 2.0 + (X[2] * X[2] if len(X) == 3 else 0.0)


def f_par(*X):
    return X[0] * X[0] + X[1] + (np.exp(X[2]) if len(X) == 3 else 0.0)


def f_vec(*X):
    return (X[0] + X[1], X[0] * X[-1] + 1.0)


def g_exact(*X):
    return np.sin(X[0]) * np.cos(X[1]) * (np.cos(X[2]) if len(X) == 3 else 1.0)


def g_grad(*X):
    cz = np.cos(X[2]) if len(X) == 3 else 1.0
    out = (np.cos(X[0]) * np.cos(X[1]) * cz, -np.sin(X[0]) * np.sin(X[1]) * cz)
    return out + ((-np.sin(X[0]) * np.cos(X[1]) * np.sin(X[2]),) if len(X) == 3 else ())


class SquaredError:
    """(u_h - g)^2, or |grad u_h - grad g|^2, on a tensor grid of the parameter domain"""

    def __init__(self, uh, geo, grad):
        self.uh, self.geo, self.grad = uh, geo, grad

    def grid_eval(self, grid):
        P = self.geo.grid_eval(grid)
        X = tuple(P[..., k] for k in range(P.shape[-1]))
        if not self.grad:
            return (self.uh.grid_eval(grid) - g_exact(*X)) ** 2
        gpar = self.uh.grid_jacobian(grid)                           # parametric gradient, (x, y, z) order
        J = self.geo.grid_jacobian(grid)
        gphys = np.linalg.solve(np.swapaxes(J, -1, -2), gpar[..., None])[..., 0]
        return ((gphys - np.stack(g_grad(*X), axis=-1)) ** 2).sum(axis=-1)


rng = np.random.default_rng(20241019)
for tag, p, n, geo in (('2d', 3, 6, geometry.quarter_annulus()), ('3d', 2, 4, cylinder())):
    kvs = geo.sdim * (bspline.make_knots(p, 0.0, 1.0, n),)
    G[tag + '_pn'] = np.array([p, n])
    G[tag + '_phys'] = assemble.integrate(kvs, f_phys, f_physical=True, geo=geo)
    G[tag + '_par_geo'] = assemble.integrate(kvs, f_par, geo=geo)
    G[tag + '_par'] = assemble.integrate(kvs, f_par)
    c = rng.uniform(-1.0, 1.0, size=tuple(kv.numdofs for kv in kvs))
    G[tag + '_dofs'] = c
    uh = bspline.BSplineFunc(kvs, c)
    G[tag + '_spline'] = assemble.integrate(kvs, uh, geo=geo)
    G[tag + '_vec'] = np.asarray(assemble.integrate(kvs, f_vec))     # (the reference multiplies by |det J| without the component axis: no geo)
    G[tag + '_l2sq'] = assemble.integrate(kvs, SquaredError(uh, geo, False), geo=geo)
    G[tag + '_h1sq'] = assemble.integrate(kvs, SquaredError(uh, geo, True), geo=geo)


def one(*X):
    return 1.0


sq, cube = geometry.unit_square(), geometry.unit_cube()
G['one_square'] = np.array([assemble.integrate(sq.kvs, one), assemble.integrate(sq.kvs, one, f_physical=True, geo=sq)])
G['one_cube'] = np.array([assemble.integrate(cube.kvs, one), assemble.integrate(cube.kvs, one, f_physical=True, geo=cube)])
G['one_annulus'] = assemble.integrate(2 * (bspline.make_knots(3, 0.0, 1.0, 10),), one, geo=geometry.quarter_annulus())

np.savez_compressed(os.path.join(OUT, 'golden_quad.npz'), **{k: np.asarray(v) for k, v in G.items()})
for k in sorted(G):
    if np.size(G[k]) <= 4:
        print(k, G[k])

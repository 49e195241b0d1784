#!/usr/bin/env python3
"""Golden solutions of non-symmetric Dirichlet problems from the REAL reference (c-f-h/pyiga).

Build the unmodified reference outside the repository as the header of make_golden.py describes, then

    PYTHONPATH=/tmp/pyiga_oracle python3 tests/golden/make_golden_nonsym_solve.py

Writes `tests/golden/golden_nonsym_solve.npz`: inputs and outputs of the reference's public API only (assemble.assemble,
RestrictedLinearSystem, operators.make_solver, LS.complete; no reference source).  Cases:
  notebook_*  the convection-diffusion problem of notebooks/solve-convdiff.ipynb at p = 3, n = 24 (the notebook: n = 200), the
              centres of its random inclusions drawn once from a seeded generator and stored
  cd3_*       the 3D convection-diffusion form on the quarter-annulus cylinder, p = 2, n = 6, with the load f3 and the
              Dirichlet data g3 of golden_solve.npz on every side
"""
import os

import numpy as np

import pyiga
from pyiga import assemble, bspline, geometry, operators

pyiga.set_max_threads(1)
OUT = os.path.dirname(os.path.abspath(__file__))
G = {}

# (1) the notebook problem
R_INCL, NUM_INCL = 0.035, 100
rng = np.random.default_rng(2024)
centers = []
while len(centers) < NUM_INCL:
    cx, cy = 2 * rng.random(2)
    if 1 < np.sqrt(cx ** 2 + cy ** 2) < 2:
        centers.append((cx, cy))
centers = np.array(centers)


def diff_coeff(x, y):
    z = np.inf * np.ones_like(x * y)
    for (cx, cy) in centers:
        z = np.minimum(z, (x - cx) ** 2 + (y - cy) ** 2)
    return 0.01 + (np.sqrt(z) < R_INCL) * 0.99


def g_inflow(x, y):
    return (4 * (0.25 - (1.5 - y) ** 2)) ** 7


NOTEBOOK_FORM = '(inner(diff_coeff * grad(u), grad(v)) + inner((x[1],-x[0]), grad(u)) * v) * dx'
geo = geometry.quarter_annulus()
kvs = 2 * (bspline.make_knots(3, 0.0, 1.0, 24),)
bcs = assemble.compute_dirichlet_bcs(kvs, geo, [('top', g_inflow), ('left', 0), ('right', 0)])
A = assemble.assemble(NOTEBOOK_FORM, kvs, geo=geo, diff_coeff=diff_coeff)
LS = assemble.RestrictedLinearSystem(A, 0, bcs)
u = LS.complete(operators.make_solver(LS.A).dot(LS.b))
G['notebook_centers'] = centers
G['notebook_r_incl'] = np.array(R_INCL)
G['notebook_bc_idx'], G['notebook_bc_val'] = np.asarray(bcs[0]), np.asarray(bcs[1])
G['notebook_u'] = np.asarray(u).ravel()


# (2) 3D convection-diffusion on the cylinder
def g3(x, y, z):
    return np.cos(x + 0.5 * y) + np.exp(0.3 * z - y)


def f3(x, y, z):
    return 1.0 + x * y - np.sin(z)


def kappa3(x, y, z):
    return 0.2 + 0.1 * z


CD3_FORM = '(inner(diff_coeff*grad(u),grad(v))+inner((x[1],-x[0],1.0),grad(u))*v)*dx'
geo3 = geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.quarter_annulus())
kvs3 = 3 * (bspline.make_knots(2, 0.0, 1.0, 6),)
bcs3 = assemble.compute_dirichlet_bcs(kvs3, geo3, ('all', g3))
A3 = assemble.assemble(CD3_FORM, kvs3, geo=geo3, diff_coeff=kappa3)
b3 = assemble.inner_products(kvs3, f3, f_physical=True, geo=geo3).ravel()
LS3 = assemble.RestrictedLinearSystem(A3, b3, bcs3)
G['cd3_rhs'] = b3
G['cd3_bc_idx'], G['cd3_bc_val'] = np.asarray(bcs3[0]), np.asarray(bcs3[1])
G['cd3_u'] = np.asarray(LS3.complete(operators.make_solver(LS3.A).dot(LS3.b))).ravel()

path = os.path.join(OUT, 'golden_nonsym_solve.npz')
np.savez_compressed(path, **G)
print('wrote', path, {k: np.shape(v) for k, v in G.items()})

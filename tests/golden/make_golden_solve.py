#!/usr/bin/env python3
"""Golden vectors of the solver helpers from the REAL reference (c-f-h/pyiga).

Build the unmodified reference outside the repository as the header of make_golden.py describes, then

    PYTHONPATH=/tmp/pyiga_oracle python3 tests/golden/make_golden_solve.py

Writes `tests/golden/golden_solve.npz`: inputs and outputs of the reference's public API only (no reference source).
"""
import os

import numpy as np

import pyiga
from pyiga import approx, assemble, bspline, geometry, solvers

pyiga.set_max_threads(1)
OUT = os.path.dirname(os.path.abspath(__file__))
G = {}


def cylinder():
    return geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.quarter_annulus())


def g3(x, y, z):
    return np.cos(x + 0.5 * y) + np.exp(0.3 * z - y)


def f3(x, y, z):
    return 1.0 + x * y - np.sin(z)


def put_csr(name, A):
    A = A.tocsr()
    A.sort_indices()
    G[name + '_data'], G[name + '_indices'], G[name + '_indptr'] = A.data, A.indices, A.indptr
    G[name + '_shape'] = np.array(A.shape)


# (1) fastdiag_solver on the knot vectors of test/test_solvers.py::test_fastdiag_solver
kvs_fd = [bspline.make_knots(4, 0.0, 1.0, 3), bspline.make_knots(3, 0.0, 1.0, 4), bspline.make_knots(2, 0.0, 1.0, 5)]
KM = [(assemble.stiffness(kv)[1:-1, 1:-1].toarray(), assemble.mass(kv)[1:-1, 1:-1].toarray()) for kv in kvs_fd]
rng = np.random.default_rng(7)
x_fd = rng.random(int(np.prod([K.shape[0] for K, _ in KM])))
G['fastdiag_x'] = x_fd
G['fastdiag_y'] = solvers.fastdiag_solver(KM).dot(x_fd)

# (2) RestrictedLinearSystem on a 3D p=2 cylinder patch, Dirichlet data on two sides
kvs3 = 3 * (bspline.make_knots(2, 0.0, 1.0, 4),)
geo = cylinder()
A = assemble.stiffness(kvs3, geo=geo)
b = assemble.inner_products(kvs3, f3, f_physical=True, geo=geo).ravel()
bcs2 = assemble.compute_dirichlet_bcs(kvs3, geo, [('left', g3), ('top', g3)])
G['rls_bc_idx'], G['rls_bc_val'] = np.asarray(bcs2[0]), np.asarray(bcs2[1])
G['rls_b_full'] = b
put_csr('rls_A_full', A)
LS = assemble.RestrictedLinearSystem(A, b, bcs2)
put_csr('rls_A', LS.A)
G['rls_b'] = LS.b
u_free = rng.random(LS.A.shape[0])
G['rls_u_free'] = u_free
G['rls_complete'] = LS.complete(u_free)
elim = np.asarray(bcs2[0])[::2]
LSe = assemble.RestrictedLinearSystem(A, b, bcs2, elim_rows=elim)
G['rls_elim_rows'] = elim
put_csr('rls_elim_A', LSe.A)
G['rls_elim_b'] = LSe.b

# (3) 3D Poisson solves on the cylinder: 'all' sides and two sides (make_solver on LS.A)
kvs5 = 3 * (bspline.make_knots(2, 0.0, 1.0, 5),)
A5 = assemble.stiffness(kvs5, geo=geo)
b5 = assemble.inner_products(kvs5, f3, f_physical=True, geo=geo).ravel()
G['poisson3d_rhs'] = b5
for tag, bd in (('all', ('all', g3)), ('two', [('left', g3), ('top', g3)])):
    bcs = assemble.compute_dirichlet_bcs(kvs5, geo, bd)
    LS = assemble.RestrictedLinearSystem(A5, b5, bcs)
    G['poisson3d_%s_bc_idx' % tag], G['poisson3d_%s_bc_val' % tag] = np.asarray(bcs[0]), np.asarray(bcs[1])
    G['poisson3d_%s_u' % tag] = LS.complete(solvers.make_solver(LS.A, spd=True).dot(LS.b))

# (4) project_L2: parameter domain (2D, 3D, vector-valued f) and physical domain (3D cylinder)
kv2 = (bspline.make_knots(3, 0.0, 1.0, 6), bspline.make_knots(2, 0.0, 1.0, 5))
G['l2_param2d'] = approx.project_L2(kv2, lambda x, y: np.exp(x) * np.cos(2 * y))
kv3 = (bspline.make_knots(2, 0.0, 1.0, 4), bspline.make_knots(3, 0.0, 1.0, 3), bspline.make_knots(2, 0.0, 1.0, 5))
G['l2_param3d'] = approx.project_L2(kv3, f3)
G['l2_param2d_vec'] = approx.project_L2(kv2, lambda x, y: (x * y, np.sin(x) - y, 1.0 + 0 * x))
G['l2_phys3d'] = approx.project_L2(kvs5, g3, f_physical=True, geo=geo)

path = os.path.join(OUT, 'golden_solve.npz')
np.savez_compressed(path, **G)
print('wrote', path, {k: np.shape(v) for k, v in G.items()})

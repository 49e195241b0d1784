#!/usr/bin/env python3
"""Golden vectors of the multipatch helpers from the REAL reference (c-f-h/pyiga).

Build the unmodified reference outside the repository as the header of make_golden.py describes, then

    PYTHONPATH=/tmp/pyiga_oracle python3 tests/golden/make_golden_multipatch.py

Writes `tests/golden/golden_multipatch.npz`: inputs and outputs of the reference's public API only (no reference source).
"""
import os

import numpy as np

import pyiga
from pyiga import bspline, geometry, assemble, vform

pyiga.set_max_threads(1)
OUT = os.path.dirname(os.path.abspath(__file__))
G = {}


def lshape():
    kvs = 2 * (bspline.make_knots(2, 0.0, 1.0, 8),)
    squ = geometry.unit_square()
    geos = (squ, squ.translate((1, 0)), squ.scale((-1, 1)).translate((2, 1)))
    MP = assemble.Multipatch([(kvs, g) for g in geos])
    MP.join_boundaries(0, 'right', 1, 'left')
    MP.join_boundaries(1, 'top', 2, 'bottom', flip=(True,))
    MP.finalize()
    return MP


def notebook_domain(p, n):
    kvs = 2 * (bspline.make_knots(p, 0.0, 1.0, n),)
    geos = [geometry.quarter_annulus(),
            geometry.unit_square().translate((-1, 1)),
            geometry.quarter_annulus().rotate_2d(np.pi).translate((-1, 3)),
            geometry.quarter_annulus().rotate_2d(-np.pi / 2).translate((-2, 1))]
    return kvs, geos


def f_rhs(x, y):
    return np.exp(-5 * ((x - 0.3) ** 2 + (y - 1) ** 2))


def g_dir(x, y):
    return 1e-1 * np.sin(8 * x)


def put_csr(name, A):
    A = A.tocsr()
    A.sort_indices()
    G[name + '_data'], G[name + '_indices'], G[name + '_indptr'] = A.data, A.indices, A.indptr


# slice_indices / boundary_dofs
for k, (ax, idx, shape, flip) in enumerate([(0, 0, (4, 5), None), (1, -1, (4, 5), (True,)), (2, 0, (3, 4, 5), (True, False)),
                                            (1, -1, (3, 4, 5), (False, True)), (0, -1, (3, 4, 5), (True, True))]):
    G['slice%d_mi' % k] = assemble.slice_indices(ax, idx, shape, flip=flip)
    G['slice%d_rav' % k] = assemble.slice_indices(ax, idx, shape, ravel=True, flip=flip)
kvs3 = (bspline.make_knots(2, 0.0, 1.0, 3), bspline.make_knots(1, 0.0, 1.0, 4), bspline.make_knots(3, 0.0, 1.0, 2))
for k, (bd, flip) in enumerate([('left', None), ('top', (True, False)), ((0, 1), (False, True)), ('back', None)]):
    G['bdofs%d' % k] = assemble.boundary_dofs(kvs3, bd, ravel=True, flip=flip)
# greville
for k, kv in enumerate([bspline.make_knots(3, 0.0, 1.0, 7), bspline.make_knots(2, -1.0, 2.0, 5, mult=2),
                        bspline.make_knots(1, 0.0, 1.0, 4), bspline.KnotVector(np.array([0, 0, 0, .1, .5, .5, 1, 1, 1.]), 2)]):
    G['grev%d' % k] = kv.greville()
# combine_bcs
G['comb_idx'], G['comb_val'] = assemble.combine_bcs([(np.array([5, 1, 3]), np.array([.5, .1, .3])),
                                                     (np.array([3, 7, 1]), np.array([3., 7., 1.]))])
# control nets of transformed geometries
G['tr_bspl'] = geometry.unit_square().translate((1, 2)).scale((-1, 3)).rotate_2d(0.3).coeffs
qa = geometry.quarter_annulus().rotate_2d(np.pi).translate((-1, 3)).scale(2.0)
G['tr_nurbs'] = qa.coeffs
G['bbox_qa'] = np.array(geometry.quarter_annulus().bounding_box(grid=4))
# L-shape
MP = lshape()
G['L_numdofs'] = MP.numdofs
for p in range(3):
    G['L_p2g%d' % p] = MP.patch_to_global_idx(p)
G['L_bc_idx'], G['L_bc_val'] = MP.compute_dirichlet_bcs([(0, 'top', lambda x, y: 1.0), (2, 'right', g_dir), (1, 'bottom', 0.5)])
# notebook domain at p = 3, n = 15
kvs, geos = notebook_domain(3, 15)
MPn = assemble.Multipatch([(kvs, g) for g in geos], automatch=True)
G['nb_numdofs'] = MPn.numdofs
for p in range(4):
    G['nb_p2g%d' % p] = MPn.patch_to_global_idx(p)
G['nb_bc_idx'], G['nb_bc_val'] = MPn.compute_dirichlet_bcs([(0, 'bottom', g_dir), (0, 'right', g_dir), (1, 'top', g_dir),
                                                           (2, 'left', g_dir), (2, 'bottom', g_dir), (3, 'bottom', 0)])
A, b = MPn.assemble_system(vform.stiffness_vf(2), vform.L2functional_vf(2, physical=True), f=f_rhs)
put_csr('nb_A', A)
G['nb_b'] = b
# two squares (test_multipatch_assemble)
kvs = 2 * (bspline.make_knots(2, 0.0, 1.0, 8),)
MP2 = assemble.Multipatch([(kvs, geometry.unit_square()), (kvs, geometry.unit_square().translate((1, 0)))], automatch=True)


def f2(x, y):
    return np.sin(2 * x) + np.exp(y)


A, b = MP2.assemble_system(vform.stiffness_vf(2), vform.L2functional_vf(2, physical=True), f=f2)
put_csr('sq_A', A)
G['sq_b'] = b
np.savez_compressed(os.path.join(OUT, 'golden_multipatch.npz'), **G)
print('wrote golden_multipatch.npz: %d arrays' % len(G))

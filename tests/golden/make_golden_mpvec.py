#!/usr/bin/env python3
"""Golden linear elasticity on multipatch domains from the REAL reference (c-f-h/pyiga).

Build the unmodified reference outside the repository as the header of make_golden.py describes, then

    PYTHONPATH=/tmp/pyiga_oracle python3 tests/golden/make_golden_mpvec.py

Writes `tests/golden/golden_mpvec.npz`: inputs and outputs of the reference's public API only (no reference source).  The
reference's `Multipatch.assemble_system` has no vector-valued path, so per case every patch is assembled with
`assemble.assemble(ELASTICITY, kvs, bfuns=[('u', nc), ('v', nc)], geo=geo, layout='blocked', mu=1, lam=2)` and the blocked
matrices are glued with the reference's own `patch_to_global`:  A = sum_p (I_nc (x) X_p) A_p (I_nc (x) X_p)^T, in patch
order.  The fixed dofs and their values come from the reference's `compute_dirichlet_bc` with a vector-valued function on one
side of patch 0 (local blocked index c N_p + i -> global blocked index c n + l2g_p[i]); the solution is `spsolve` of the
`RestrictedLinearSystem`, completed with the Dirichlet values.  The domains are joined by hand in the order
tests/_mpsolve_model.py and tests/_solver_cases.py join them, so the global numbering is the same.
"""
import os

import numpy as np
import scipy.sparse
import scipy.sparse.linalg

import pyiga
from pyiga import assemble, bspline, geometry

pyiga.set_max_threads(1)
OUT = os.path.dirname(os.path.abspath(__file__))
ELASTICITY = '(2*mu*inner(0.5*(grad(u)+grad(u).T), 0.5*(grad(v)+grad(v).T)) + lam*div(u)*div(v)) * dx'
G = {}


def lshape(p, n):
    kvs = 2 * (bspline.make_knots(p, 0.0, 1.0, n),)
    squ = geometry.unit_square()
    geos = (squ, squ.translate((1, 0)), squ.scale((-1, 1)).translate((2, 1)))
    MP = assemble.Multipatch([(kvs, g) for g in geos])
    MP.join_boundaries(0, 'right', 1, 'left')
    MP.join_boundaries(1, 'top', 2, 'bottom', flip=(True,))
    MP.finalize()
    return MP


def cubes2(p, n):
    kvs = 3 * (bspline.make_knots(p, 0.0, 1.0, n),)
    cube = geometry.unit_cube()
    MP = assemble.Multipatch([(kvs, cube), (kvs, cube.translate((1, 0, 0)))])
    MP.join_boundaries(0, (2, 1), 1, (2, 0))
    MP.finalize()
    return MP


def g2(x, y):
    return (0.01 + 0.02 * y, -0.02 + 0.01 * y * y)


def g3(x, y, z):
    return (0.01 * y, -0.02 * z, 0.005 + 0.01 * y * z)


CASES = (('lshape', lshape, 2, 4, 2, (0, 'left'), g2, (1e-3, -2e-3)),
         ('cubes2', cubes2, 2, 2, 3, (0, (2, 0)), g3, (1e-3, 0.0, -1e-3)))

for name, make, p, n, nc, (q, side), g, load in CASES:
    MP = make(p, n)
    nd = MP.numdofs
    A = scipy.sparse.csr_matrix((nc * nd, nc * nd))
    I = scipy.sparse.identity(nc, format='csr')
    for k in range(MP.numpatches):
        kvs, geo = MP.patches[k]
        Ak = assemble.assemble(ELASTICITY, kvs, bfuns=[('u', nc), ('v', nc)], geo=geo, layout='blocked', mu=1.0, lam=2.0)
        X = scipy.sparse.kron(I, MP.patch_to_global(k), format='csr')
        A = A + X @ scipy.sparse.csr_matrix(Ak) @ X.T
    A = A.tocsr()
    A.sum_duplicates()
    A.sort_indices()
    kvs, geo = MP.patches[q]
    idx, vals = assemble.compute_dirichlet_bc(kvs, geo, side, g)
    Nq = int(np.prod([kv.numdofs for kv in kvs]))
    comp, loc = np.divmod(np.asarray(idx), Nq)
    fixed = comp * nd + MP.patch_to_global_idx(q)[loc]
    order = np.argsort(fixed)
    fixed, vals = fixed[order].astype(np.int64), np.asarray(vals, dtype=np.float64)[order]
    b = np.concatenate([np.full(nd, f) for f in load])
    LS = assemble.RestrictedLinearSystem(A, b, (fixed, vals))
    u = LS.complete(scipy.sparse.linalg.spsolve(LS.A.tocsc(), LS.b))
    G[name + '_A_data'], G[name + '_A_indices'], G[name + '_A_indptr'] = A.data, A.indices, A.indptr
    G[name + '_A_shape'] = np.array(A.shape)
    G[name + '_fixed'], G[name + '_values'], G[name + '_rhs'], G[name + '_u'] = fixed, vals, b, u
    G[name + '_desc'] = np.array('%s p=%d n=%d nc=%d, %d x %d dofs: linear elasticity mu=1 lam=2, blocked per-patch matrices glued '
                                 'with patch_to_global; patch %d side %r fixed; spsolve' % (name, p, n, nc, nc, nd, q, side))

path = os.path.join(OUT, 'golden_mpvec.npz')
np.savez_compressed(path, **G)
print('wrote', path, {k: np.shape(v) for k, v in G.items()})

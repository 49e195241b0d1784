#!/usr/bin/env python3
"""Golden eigenpairs of the elastic vibration problem from the REAL reference (c-f-h/pyiga).

Build the unmodified reference outside the repository as the header of make_golden.py describes, then

    PYTHONPATH=/tmp/pyiga_oracle python3 tests/golden/make_golden_veceig.py

Writes `tests/golden/golden_veceig.npz`: inputs and outputs of the reference's public API only (no reference source).  Per case:
the reference's `assemble.assemble` of the elasticity form (mu = 1, lam = 2) with `layout='blocked'`, its `assemble.mass` on the
block diagonal, `boundary_dofs` for the fixed sides of every component, `RestrictedLinearSystem` for the restriction to the
free dofs, then dense `scipy.linalg.eigh` of the restricted pencil.  Stored: the fixed dofs (blocked numbering), the 12 lowest
eigenvalues, their M-orthonormal eigenvectors completed with zeros on the fixed dofs, and `ks`: the k of (4, 6, 10) that do not
cut a cluster, lam[k] - lam[k-1] > 1e-3 lam[k], decided on the reference's own numbers.  `annulus2` also stores the blocked CSR
of K and the scalar M, so that the host model of the controller runs without a device.
"""
import os

import numpy as np
import scipy.linalg
import scipy.sparse

import pyiga
from pyiga import assemble, bspline, geometry

pyiga.set_max_threads(1)
OUT = os.path.dirname(os.path.abspath(__file__))
NEV = 12
KS = (4, 6, 10)
MU, LAM = 1.0, 2.0
# (the form of tests/_vecsolve_model.py; the second string is the same form without `.T` on a sum)
ELASTICITY = '(2*mu*inner(0.5*(grad(u)+grad(u).T), 0.5*(grad(v)+grad(v).T)) + lam*div(u)*div(v)) * dx'
ELASTICITY_PLAIN = '(mu*inner(grad(u),grad(v)) + mu*inner(grad(u).T, grad(v)) + lam*div(u)*div(v)) * dx'
G = {}


def cylinder():
    return geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.quarter_annulus())


def all_sides(dim):
    return [(ax, side) for ax in range(dim) for side in (0, 1)]


def put_csr(name, A):
    A = scipy.sparse.csr_matrix(A)
    A.sort_indices()
    G[name + '_indptr'], G[name + '_indices'], G[name + '_data'] = A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data
    G[name + '_shape'] = np.array(A.shape, dtype=np.int64)


for name, p, n, nc, geo, sides in (('annulus2', 3, 10, 2, geometry.quarter_annulus(), all_sides(2)),
                                   ('cylinder3', 2, 4, 3, cylinder(), [(0, 0)])):
    kvs = geo.dim * (bspline.make_knots(p, 0.0, 1.0, n),)
    bfuns = [('u', nc), ('v', nc)]
    try:
        K = assemble.assemble(ELASTICITY, kvs, geo=geo, bfuns=bfuns, layout='blocked', mu=MU, lam=LAM)
        form = ELASTICITY
    except Exception as e:                                    # (the parser refuses `.T` of a sum)
        print('ELASTICITY refused (%s): the expanded form' % e)
        K = assemble.assemble(ELASTICITY_PLAIN, kvs, geo=geo, bfuns=bfuns, layout='blocked', mu=MU, lam=LAM)
        form = ELASTICITY_PLAIN
    K = scipy.sparse.csr_matrix(K)
    M1 = scipy.sparse.csr_matrix(assemble.mass(kvs, geo=geo))
    M = scipy.sparse.block_diag([M1] * nc, format='csr')
    N = M1.shape[0]
    one = np.unique(np.concatenate([assemble.boundary_dofs(kvs, s, ravel=True) for s in sides]))
    fixed = np.concatenate([one + c * N for c in range(nc)]).astype(np.int64)
    bcs = (fixed, np.zeros(fixed.size))
    zero = np.zeros(K.shape[0])
    LK = assemble.RestrictedLinearSystem(K, zero, bcs)
    LM = assemble.RestrictedLinearSystem(M, zero, bcs)
    lam, V = scipy.linalg.eigh(LK.A.toarray(), LM.A.toarray())
    ks = [k for k in KS if lam[k] - lam[k - 1] > 1e-3 * lam[k]]
    assert len(ks) >= 2, (name, lam[:NEV])
    G[name + '_fixed'] = np.sort(fixed)
    G[name + '_lam'] = lam[:NEV]
    G[name + '_V'] = np.stack([LK.complete(V[:, i]) for i in range(NEV)], axis=1)
    G[name + '_ks'] = np.array(ks, dtype=np.int64)
    G[name + '_desc'] = np.array('%s p=%d n=%d nc=%d, sides %r fixed in every component: assemble(%r, layout=blocked, mu=%g, lam=%g), '
                                 'block_diag([mass] * nc); eigh(RestrictedLinearSystem(K).A, RestrictedLinearSystem(M).A)'
                                 % (name, p, n, nc, sides, form, MU, LAM))
    if name == 'annulus2':
        put_csr(name + '_K', K)
        put_csr(name + '_M1', M1)
    print(name, 'n', K.shape[0], 'ks', ks, 'lam', lam[:NEV])

path = os.path.join(OUT, 'golden_veceig.npz')
np.savez_compressed(path, **G)
print('wrote', path, {k: np.shape(v) for k, v in G.items()}, os.path.getsize(path), 'bytes')

#!/usr/bin/env python3
"""Golden eigenpairs from the REAL reference (c-f-h/pyiga).

Build the unmodified reference outside the repository as the header of make_golden.py describes, then

    PYTHONPATH=/tmp/pyiga_oracle python3 tests/golden/make_golden_eig.py

Writes `tests/golden/golden_eig.npz`: inputs and outputs of the reference's public API only (no reference source).  Per case
(every side fixed): the reference's `assemble.stiffness` and `assemble.mass`, `compute_dirichlet_bcs` for the fixed dofs,
`RestrictedLinearSystem` for the restriction to the free dofs, then dense `scipy.linalg.eigh` of the restricted pencil.  Stored:
the fixed dofs, the 12 lowest eigenvalues and their M-orthonormal eigenvectors, completed with zeros on the fixed dofs.
"""
import os

import numpy as np
import scipy.linalg

import pyiga
from pyiga import assemble, bspline, geometry

pyiga.set_max_threads(1)
OUT = os.path.dirname(os.path.abspath(__file__))
NEV = 12
G = {}


def cylinder():
    return geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.quarter_annulus())


for name, p, n, geo in (('annulus', 3, 16, geometry.quarter_annulus()), ('cylinder', 2, 6, cylinder())):
    kvs = geo.dim * (bspline.make_knots(p, 0.0, 1.0, n),)
    K = assemble.stiffness(kvs, geo=geo)
    M = assemble.mass(kvs, geo=geo)
    bcs = assemble.compute_dirichlet_bcs(kvs, geo, ('all', 0.0))
    zero = np.zeros(K.shape[0])
    LK = assemble.RestrictedLinearSystem(K, zero, bcs)
    LM = assemble.RestrictedLinearSystem(M, zero, bcs)
    lam, V = scipy.linalg.eigh(LK.A.toarray(), LM.A.toarray())
    G[name + '_fixed'] = np.sort(np.asarray(bcs[0], dtype=np.int64))
    G[name + '_lam'] = lam[:NEV]
    G[name + '_V'] = np.stack([LK.complete(V[:, i]) for i in range(NEV)], axis=1)
    G[name + '_desc'] = np.array('%s p=%d n=%d, all sides fixed: eigh(RestrictedLinearSystem(stiffness).A, RestrictedLinearSystem(mass).A)'
                                 % (name, p, n))

path = os.path.join(OUT, 'golden_eig.npz')
np.savez_compressed(path, **G)
print('wrote', path, {k: np.shape(v) for k, v in G.items()})

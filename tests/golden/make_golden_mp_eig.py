#!/usr/bin/env python3
"""Golden eigenpairs of multipatch domains from the REAL reference (c-f-h/pyiga).

Build the unmodified reference outside the repository as the header of make_golden.py describes, then

    PYTHONPATH=/tmp/pyiga_oracle python3 tests/golden/make_golden_mp_eig.py

Writes `tests/golden/golden_mp_eig.npz`: inputs and outputs of the reference's public API only (no reference source).  Per case:
the reference's `Multipatch.assemble_system` for the stiffness and for the mass form (right-hand side 0), `MP.compute_dirichlet_bcs`
for the fixed dofs, `RestrictedLinearSystem` for the restriction to the free dofs, then dense `scipy.linalg.eigh` of the
restricted pencil.  Stored: the fixed dofs, the 12 lowest eigenvalues and their M-orthonormal eigenvectors, completed with zeros
on the fixed dofs.  The domains are joined by hand in the order tests/_mpsolve_model.py and tests/_solver_cases.py join them, so
the global numbering is the same.
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


def lshape(p, n):
    kvs = 2 * (bspline.make_knots(p, 0.0, 1.0, n),)
    squ = geometry.unit_square()
    geos = (squ, squ.translate((1, 0)), squ.scale((-1, 1)).translate((2, 1)))
    MP = assemble.Multipatch([(kvs, g) for g in geos])
    MP.join_boundaries(0, 'right', 1, 'left')
    MP.join_boundaries(1, 'top', 2, 'bottom', flip=(True,))
    MP.finalize()
    # the outer boundary: every side that is not an interface
    sides = [(0, 'left'), (0, 'bottom'), (0, 'top'), (1, 'bottom'), (1, 'right'), (2, 'left'), (2, 'right'), (2, 'top')]
    return MP, sides


def notebook(p, n):
    kvs = 2 * (bspline.make_knots(p, 0.0, 1.0, n),)
    geos = [geometry.quarter_annulus(),
            geometry.unit_square().translate((-1, 1)),
            geometry.quarter_annulus().rotate_2d(np.pi).translate((-1, 3)),
            geometry.quarter_annulus().rotate_2d(-np.pi / 2).translate((-2, 1))]
    MP = assemble.Multipatch([(kvs, g) for g in geos])
    MP.join_boundaries(0, (0, 1), 1, (1, 1), flip=(False,))
    MP.join_boundaries(1, (1, 0), 2, (0, 1), flip=(True,))
    MP.join_boundaries(1, (0, 0), 3, (0, 1), flip=(False,))
    MP.finalize()
    return MP, [(0, 'bottom'), (0, 'right'), (1, 'top'), (2, 'left'), (2, 'bottom'), (3, 'bottom')]


def cubes2(p, n):
    kvs = 3 * (bspline.make_knots(p, 0.0, 1.0, n),)
    cube = geometry.unit_cube()
    MP = assemble.Multipatch([(kvs, cube), (kvs, cube.translate((1, 0, 0)))])
    MP.join_boundaries(0, (2, 1), 1, (2, 0))
    MP.finalize()
    sides = [(q, (ax, sd)) for q in (0, 1) for ax in range(3) for sd in (0, 1) if (q, ax, sd) not in ((0, 2, 1), (1, 2, 0))]
    return MP, sides


for name, make, p, n in (('lshape', lshape, 2, 8), ('notebook', notebook, 3, 8), ('cubes2', cubes2, 2, 4)):
    MP, sides = make(p, n)
    K, _ = MP.assemble_system('inner(grad(u), grad(v)) * dx', '0 * v * dx')
    M, _ = MP.assemble_system('u * v * dx', '0 * v * dx')
    bcs = MP.compute_dirichlet_bcs([(q, bd, lambda *x: 0.0) for q, bd in sides])
    zero = np.zeros(K.shape[0])
    LK = assemble.RestrictedLinearSystem(K.tocsr(), zero, bcs)
    LM = assemble.RestrictedLinearSystem(M.tocsr(), zero, bcs)
    lam, V = scipy.linalg.eigh(LK.A.toarray(), LM.A.toarray())
    G[name + '_fixed'] = np.sort(np.asarray(bcs[0], dtype=np.int64))
    G[name + '_lam'] = lam[:NEV]
    G[name + '_V'] = np.stack([LK.complete(V[:, i]) for i in range(NEV)], axis=1)
    G[name + '_desc'] = np.array('%s p=%d n=%d, %d dofs: eigh of the RestrictedLinearSystem matrices of Multipatch.assemble_system '
                                 '(stiffness, mass)' % (name, p, n, K.shape[0]))

path = os.path.join(OUT, 'golden_mp_eig.npz')
np.savez_compressed(path, **G)
print('wrote', path, {k: np.shape(v) for k, v in G.items()})

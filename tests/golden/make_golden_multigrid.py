#!/usr/bin/env python3
"""Golden vectors of the multigrid pieces from the REAL reference (c-f-h/pyiga): run against the scratch build of the unmodified
reference that make_golden.py describes,

    PYTHONPATH=<scratch build of the reference> python3 tests/golden/make_golden_multigrid.py

Writes tests/golden/golden_multigrid.npz, data only:
  * KnotVector.refine, bspline.knot_insertion and bspline.prolongation for p = 1..5 with single and double interior knots;
  * for the L-shape (p = 2 and 3, n = 8) and the notebook domain (p = 3, n = 8), joined by hand as tests/_mpsolve_model.py joins
    them: the global matrix and right-hand side of Multipatch.assemble_system, the Dirichlet dofs and values, a start vector
    (zero on the Dirichlet dofs), the colour order (first-fit colouring in ascending dof order of the free rows of the
    reference's pattern, restated below), the result of solvers.gauss_seidel(A, x, b, indices=order, sweep=...) for the three
    sweep kinds, and the direct solution of the Dirichlet problem.
"""
import os

import numpy as np
import scipy.sparse
import scipy.sparse.linalg

from pyiga import assemble, bspline, geometry, solvers

OUT = os.path.dirname(os.path.abspath(__file__))
STIFF = 'inner(grad(u),grad(v))*dx'
NOTEBOOK_DIRICHLET = [(0, 'bottom'), (0, 'right'), (1, 'top'), (2, 'left'), (2, 'bottom'), (3, 'bottom')]
LSHAPE_DIRICHLET = [(0, 'left'), (0, 'bottom'), (2, 'top')]


def f2(x, y):
    return np.exp(-5 * ((x - 0.3) ** 2 + (y - 1) ** 2))


def g2(x, y):
    return 1e-1 * np.sin(8 * x)


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
    return MP


def lshape(p, n):
    kvs = 2 * (bspline.make_knots(p, 0.0, 1.0, n),)
    squ = geometry.unit_square()
    geos = (squ, squ.translate((1, 0)), squ.scale((-1, 1)).translate((2, 1)))
    MP = assemble.Multipatch([(kvs, g) for g in geos])
    MP.join_boundaries(0, 'right', 1, 'left')
    MP.join_boundaries(1, 'top', 2, 'bottom', flip=(True,))
    MP.finalize()
    return MP


def first_fit(indptr, indices, free):
    n = len(indptr) - 1
    colour = -np.ones(n, dtype=np.int64)
    for i in range(n):
        if not free[i]:
            continue
        nb = indices[indptr[i]:indptr[i + 1]]
        used = set(colour[nb[nb != i]].tolist())
        c = 0
        while c in used:
            c += 1
        colour[i] = c
    return colour


def splines(out):
    names = []
    for p in range(1, 6):
        for mult in (1, 2):
            if mult > p:
                continue
            name = 'kv_p%d_m%d' % (p, mult)
            kv = bspline.make_knots(p, 0.0, 1.0, 6, mult=mult)
            fine = kv.refine()
            out[name + '_kv'] = kv.kv
            out[name + '_refined'] = fine.kv
            out[name + '_refined_at'] = kv.refine([0.1, 0.55, 0.55]).kv
            out[name + '_P'] = bspline.prolongation(kv, fine).toarray()
            out[name + '_P2'] = bspline.prolongation(kv, fine.refine()).toarray()
            for k, u in enumerate((0.1, 0.5, 0.95)):
                out[name + '_ins%d' % k] = bspline.knot_insertion(kv, u).toarray()
            out[name + '_ins_u'] = np.array([0.1, 0.5, 0.95])
            names.append(name)
    out['spline_cases'] = np.array(names)


def domain(out, name, MP, sides):
    A, b = MP.assemble_system(STIFF, 'f*v*dx', f=f2)
    A = scipy.sparse.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    bcs = MP.compute_dirichlet_bcs([(p, bd, g2) for p, bd in sides])
    free = np.ones(MP.numdofs, dtype=bool)
    free[bcs[0]] = False
    colour = first_fit(A.indptr, A.indices, free)
    fr = np.flatnonzero(free)
    order = fr[np.argsort(colour[fr], kind='stable')]
    x0 = np.random.default_rng(7).standard_normal(MP.numdofs)
    x0[bcs[0]] = 0.0
    out[name + '_indptr'], out[name + '_indices'], out[name + '_data'] = A.indptr, A.indices, A.data
    out[name + '_b'] = b
    out[name + '_bc_idx'], out[name + '_bc_val'] = bcs
    out[name + '_order'] = order
    out[name + '_x0'] = x0
    for sweep in ('forward', 'backward', 'symmetric'):
        x = x0.copy()
        solvers.gauss_seidel(A, x, b, indices=order, sweep=sweep)
        out[name + '_gs_' + sweep] = x
    RS = assemble.RestrictedLinearSystem(A, b, bcs)
    out[name + '_u'] = RS.complete(scipy.sparse.linalg.spsolve(RS.A.tocsc(), RS.b))


def main():
    out = {}
    splines(out)
    domain(out, 'lshape_p2_n8', lshape(2, 8), LSHAPE_DIRICHLET)
    domain(out, 'lshape_p3_n8', lshape(3, 8), LSHAPE_DIRICHLET)
    domain(out, 'notebook_p3_n8', notebook(3, 8), NOTEBOOK_DIRICHLET)
    out['domain_cases'] = np.array(['lshape_p2_n8', 'lshape_p3_n8', 'notebook_p3_n8'])
    path = os.path.join(OUT, 'golden_multigrid.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()

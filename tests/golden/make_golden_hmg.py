#!/usr/bin/env python3
"""Golden vectors for the local multigrid on hierarchical spline spaces, from the REAL reference (c-f-h/pyiga).

Run where an unmodified build of the reference is importable (see the header of make_golden.py):

    PYTHONPATH=/path/to/built/reference python3 tests/golden/make_golden_hmg.py

Writes tests/golden/golden_hmg.npz -- data only.  The spaces are those of tests/_hier_cases.py, the tables those of
tests/_hmg_cases.py.  Per space `id` of SPACE_CASES:

    <id>_new, _trunc, _func_supp, _cell_supp, _global   the index-set families HSpace.<family>_indices(): rows (virtual level,
                                                        level, multi-index) in the order the reference lists them
    <id>_cell_supp_all                                  cell_supp_indices(remove_dirichlet=False)
    <id>_smooth_<strategy>, _smooth_<strategy>_off      indices_to_smooth(strategy): the lists of all levels, and their offsets
    <id>_nP, <id>_P<l>_{data,indices,indptr,shape}      virtual_hierarchy_prolongators() as CSR triples (they are small)

Per solve row (case, strategy, smoother) of SOLVE_ROWS, key `r` = case_strategy_smoother: stiffness on the quarter annulus (2D) /
the twisted box (3D), right-hand side f_rhs, all sides Dirichlet, local_mg_step(hs, A, f, Ps, indices_to_smooth(strategy),
smoother, 2) iterated as iterative_solve does with tol 1e-8:

    <r>_its                 the iteration count
    <r>_x1, <r>_x2          the iterates 1 and 2 (natural order of the index lists)
    <r>_ratios              the residual ratio after every iteration
"""
import os
import sys

import numpy as np
import scipy.sparse

import pyiga
from pyiga import assemble, bspline, geometry, solvers
from pyiga.hierarchical import HSpace

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import _hier_cases as hc                                          # noqa: E402
import _hmg_cases as mc                                           # noqa: E402

pyiga.set_max_threads(1)
OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    out = {}
    for name in mc.SPACE_CASES:
        hs = mc.build(bspline, HSpace, name)
        for fam in mc.FAMILIES:
            out['%s_%s' % (name, fam)] = mc.pack_family(getattr(hs, fam + '_indices')(), hs.dim)
            flat, off = mc.pack_lists(hs.indices_to_smooth(fam))
            out['%s_smooth_%s' % (name, fam)], out['%s_smooth_%s_off' % (name, fam)] = flat, off
        out[name + '_global'] = mc.pack_family(hs.global_indices(), hs.dim)
        out[name + '_cell_supp_all'] = mc.pack_family(hs.cell_supp_indices(remove_dirichlet=False), hs.dim)
        Ps = hs.virtual_hierarchy_prolongators()
        out[name + '_nP'] = np.array(len(Ps))
        for l, P in enumerate(Ps):
            P = scipy.sparse.csr_matrix(P)
            P.sort_indices()
            key = '%s_P%d' % (name, l)
            out[key + '_data'], out[key + '_indices'], out[key + '_indptr'] = P.data, P.indices.astype(np.int32), P.indptr.astype(np.int32)
            out[key + '_shape'] = np.array(P.shape)
        print(name, hs.numactive, [P.shape for P in Ps])
    for row in mc.SOLVE_ROWS:
        name, strategy, smoother = row
        hs = mc.build(bspline, HSpace, name)
        geo = hc.geometry_of(geometry, hs.dim)
        A = scipy.sparse.csr_matrix(assemble.assemble(hc.CASES[name][5], hs, geo=geo))
        f = assemble.assemble('f * v * dx', hs, geo=geo, f=hc.f_rhs)
        step = solvers.local_mg_step(hs, A, f, hs.virtual_hierarchy_prolongators(), hs.indices_to_smooth(strategy), smoother, mc.SMOOTH_STEPS)
        nd = hs.non_dirichlet_dofs()
        res0 = np.linalg.norm(f[nd])
        x = np.zeros(A.shape[0])
        iterates, ratios = [], []
        while True:
            x = step(x)
            iterates.append(x.copy())
            ratios.append(np.linalg.norm((f - A @ x)[nd]) / res0)
            if ratios[-1] < mc.TOL or len(ratios) >= 500:
                break
        x_ref, its = solvers.solve_hmultigrid(hs, A, f, strategy=strategy, smoother=smoother, smooth_steps=mc.SMOOTH_STEPS, tol=mc.TOL)
        assert its == len(ratios) and np.array_equal(x_ref, x), (row, its, len(ratios))
        key = mc.row_key(row)
        out[key + '_its'] = np.array(its)
        out[key + '_x1'], out[key + '_x2'] = iterates[0], iterates[1]
        out[key + '_ratios'] = np.array(ratios)
        print(key, its, '%.3e' % ratios[-1])
    path = os.path.join(OUT, 'golden_hmg.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Times of the device multipatch Dirichlet solve (pyiga_amd.solvers.MultipatchSystem): the notebook domain (2D p=3 n=256, the
Dirichlet sides of the reference's notebook) and two 3D p=3 patches of 64^3 spans glued along their face z = 0 (parameter side
(0, 0) of both) with the far ends z = 1 and z = -1 (side (0, 1) of each) fixed, so that the interface stays free and the
patches coupled; PCG to a relative residual of 1e-8 with Schwarz and Jacobi.  A timed solve records events between the phases
of every iteration: device ms of the SpMV, of the preconditioner and of the vector updates / dot products per iteration; an untimed
solve gives the wall time.  Run it under `rocprofv3 --kernel-trace --stats -- python3 tools/mp_solve_timing.py` for the
per-kernel device times.  Prints one JSON line per (case, preconditioner).  The SpMV's budget is 12 bytes per nonzero (value +
column index) of the free rows plus 4 per row (indptr), one read of x and one write of y."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyiga_amd import assemble, bspline, geometry, solvers  # noqa: E402


def f2(x, y):
    return np.exp(-5 * ((x - 0.3) ** 2 + (y - 1) ** 2))


def g2(x, y):
    return 1e-1 * np.sin(8 * x)


def f3(x, y, z):
    return 1.0 + x * y


def notebook(p, n):
    kvs = 2 * (bspline.make_knots(p, 0.0, 1.0, n),)
    geos = [geometry.quarter_annulus(), geometry.unit_square().translate((-1, 1)),
            geometry.quarter_annulus().rotate_2d(np.pi).translate((-1, 3)),
            geometry.quarter_annulus().rotate_2d(-np.pi / 2).translate((-2, 1))]
    MP = assemble.Multipatch([(kvs, g) for g in geos], automatch=True)
    sides = [(0, 'bottom'), (0, 'right'), (1, 'top'), (2, 'left'), (2, 'bottom'), (3, 'bottom')]
    return MP, f2, [(p_, bd, g2) for p_, bd in sides]


def cylinders(p, n):
    kvs = 3 * (bspline.make_knots(p, 0.0, 1.0, n),)
    geo = geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.bspline_quarter_annulus())
    MP = assemble.Multipatch([(kvs, geo), (kvs, geo.scale((1, 1, -1)))], automatch=True)
    return MP, f3, [(0, (0, 1), 0.0), (1, (0, 1), 0.0)]           # not the glued face (0, 0): the patches stay coupled


def run(name, MP, f, bdconds, preconds, tol=1e-8, maxiter=5000):
    t0 = time.perf_counter()
    bcs = MP.compute_dirichlet_bcs(bdconds)
    t_bcs = time.perf_counter() - t0
    t0 = time.perf_counter()
    S = solvers.MultipatchSystem(MP, 'inner(grad(u),grad(v))*dx', 'f*v*dx', bcs=bcs, f=f)
    t_setup = time.perf_counter() - t0
    info = MP.info()
    nnz, nall = info['nnz'], MP.numdofs
    indptr, _ = MP.pattern()
    free = np.ones(nall, dtype=bool)
    free[bcs[0]] = False
    nnz_free = int(np.diff(indptr.astype(np.int64))[free].sum())
    shared = np.arange(int(MP.M_ofs[-1]), nall)                   # the global dofs of the interfaces
    for pc in preconds:
        t0 = time.perf_counter()
        S.set_precond(pc)
        t_pc = time.perf_counter() - t0
        S.solve(tol=tol, maxiter=maxiter, precond=pc, timed=True)
        ti = dict(S.info)
        t0 = time.perf_counter()
        u = S.solve(tol=tol, maxiter=maxiter, precond=pc, check_every=10)
        wall = time.perf_counter() - t0
        it = max(1, ti['iterations'])
        spmv_bytes = 12.0 * nnz_free + 4.0 * nall + 16.0 * nall
        spmv_ms = ti['spmv_ms'] / it
        out = {'case': name, 'ndofs': nall, 'n_free': ti['n_free'], 'nnz': nnz, 'nnz_free_rows': nnz_free, 'patches': MP.numpatches,
               'interface_dofs': int(shared.size), 'interface_dofs_free': int(free[shared].sum()),
               'precond': pc or 'none', 'tol': tol, 'iterations': ti['iterations'], 'converged': ti['converged'],
               'relres': ti['relres'], 'spmv_ms_per_iter': round(spmv_ms, 4),
               'precond_ms_per_iter': round(ti['precond_ms'] / it, 4), 'vector_ms_per_iter': round(ti['vector_ms'] / it, 4),
               'iter_ms': round((ti['spmv_ms'] + ti['precond_ms'] + ti['vector_ms']) / it, 4),
               'spmv_bytes': spmv_bytes, 'spmv_TBps': round(spmv_bytes / (spmv_ms * 1e-3) / 1e12, 3) if spmv_ms > 0 else None,
               'solve_wall_s': round(wall, 4), 'solve_device_ms_timed': round(ti['total_ms'], 2),
               'iterations_untimed': S.info['iterations'], 'precond_setup_s': round(t_pc, 4),
               'system_setup_s': round(t_setup, 3), 'bcs_s': round(t_bcs, 3), 'u_max': float(np.abs(u).max())}
        print(json.dumps(out), flush=True)
    S.close()
    MP.close()


if __name__ == '__main__':
    which = sys.argv[1:] or ['notebook', 'cylinders']
    if 'notebook' in which:
        run('notebook_p3_n256', *notebook(3, 256), ['schwarz', 'jacobi'])
    if 'cylinders' in which:
        run('cylinders3d_p3_n64', *cylinders(3, 64), ['schwarz', 'jacobi'])

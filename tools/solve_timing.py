#!/usr/bin/env python3
"""Times of the device Dirichlet solve (pyiga_amd.solvers.PatchSystem, igx_solver_*): C2 (2D p=3 n=256, quarter annulus) and C4
(3D p=4 n=128, cylinder), 'all' sides Dirichlet, PCG to a relative residual of 1e-8.  A timed solve records events between the
phases of every iteration: device ms of the SpMV, of the preconditioner and of the vector updates / dot products per iteration;
an untimed solve gives the wall time.  Run it under `rocprofv3 --kernel-trace --stats -- python3 tools/solve_timing.py` for the
per-kernel device times.  Prints one JSON line per (case, preconditioner).  The SpMV bytes are the values of the free rows (8 per
nonzero) plus one read of x and one write of y."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyiga_amd import assemble, bspline, geometry, solvers  # noqa: E402

CASES = {
    'c2': (2, 3, 256, lambda: geometry.quarter_annulus()),
    'c4': (3, 4, 128, lambda: geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.quarter_annulus())),
}


def f2(x, y):
    return np.exp(x) * np.cos(y)


def f3(x, y, z):
    return 1.0 + x * y - np.sin(z)


def run(name, preconds, tol=1e-8, maxiter=5000):
    dim, p, n, mkgeo = CASES[name]
    kvs = dim * (bspline.make_knots(p, 0.0, 1.0, n),)
    geo = mkgeo()
    t0 = time.perf_counter()
    bcs = assemble.compute_dirichlet_bcs(kvs, geo, ('all', 0.0))
    t_bcs = time.perf_counter() - t0
    t0 = time.perf_counter()
    S = solvers.PatchSystem(kvs, geo, f2 if dim == 2 else f3, bcs)
    t_setup = time.perf_counter() - t0
    asm_ms = S.patch.timing()['total_ms']
    nnz = S.patch.nnz
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
        nfree, nall = ti['n_free'], S.n
        spmv_bytes = 8.0 * nnz * nfree / nall + 16.0 * nall
        spmv_ms = ti['spmv_ms'] / it
        out = {'case': name, 'dim': dim, 'p': p, 'n': n, 'ndofs': nall, 'n_free': nfree, 'nnz': nnz, 'precond': pc or 'none',
               'tol': tol, 'iterations': ti['iterations'], 'converged': ti['converged'], 'relres': ti['relres'],
               'spmv_ms_per_iter': round(spmv_ms, 4), 'precond_ms_per_iter': round(ti['precond_ms'] / it, 4),
               'vector_ms_per_iter': round(ti['vector_ms'] / it, 4),
               'iter_ms': round((ti['spmv_ms'] + ti['precond_ms'] + ti['vector_ms']) / it, 4),
               'spmv_TBps': round(spmv_bytes / (spmv_ms * 1e-3) / 1e12, 3) if spmv_ms > 0 else None,
               'solve_wall_s': round(wall, 4), 'solve_device_ms_timed': round(ti['total_ms'], 2),
               'iterations_untimed': S.info['iterations'], 'precond_setup_s': round(t_pc, 4),
               'assemble_ms': round(asm_ms, 3), 'system_setup_s': round(t_setup, 3), 'bcs_s': round(t_bcs, 3),
               'u_max': float(np.abs(u).max())}
        print(json.dumps(out), flush=True)
    S.close()


if __name__ == '__main__':
    which = sys.argv[1:] or ['c2', 'c4']
    for name in which:
        run(name, ['kron', 'jacobi'] if name == 'c2' else ['kron'])

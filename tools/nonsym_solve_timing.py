#!/usr/bin/env python3
"""Times of the device BiCGStab solve (pyiga_amd.solvers.FormSystem, igx_solver_* with IGX_METHOD_BICGSTAB):
  c5        the convection-diffusion form of bench.py's C5 (3D p=5 n=96, cylinder, diff_coeff = 1 + x), every side Dirichlet
  notebook  the problem of the reference's notebooks/solve-convdiff.ipynb at its size (2D p=3 n=200, quarter annulus, 100 random
            inclusions from a seeded generator, inflow data on 'top', 0 on 'left' / 'right', rhs 0)
to a relative residual of 1e-8.  A timed solve records events between the phases of every iteration: device ms of the two SpMVs,
of the two preconditioner applies and of the vector kernels (p, s and x / r updates, t.t, the scalar steps) per iteration; an
untimed solve gives the wall time.  Run it under `rocprofv3 --kernel-trace --stats -- python3 tools/nonsym_solve_timing.py` for
the per-kernel device times.  Prints one JSON line per (case, preconditioner).  The SpMV bytes are two passes over the values of
the free rows (8 per nonzero) plus one read of x and one write of y each."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyiga_amd import assemble, assemblers, bspline, geometry, solvers  # noqa: E402


def f3(x, y, z):
    return 1.0 + x * y - np.sin(z)


def c5():
    kvs = 3 * (bspline.make_knots(5, 0.0, 1.0, 96),)
    geo = geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.quarter_annulus())
    bcs = assemble.compute_dirichlet_bcs(kvs, geo, ('all', 0.0))
    asm = assemblers.ConvDiffAssembler3D(kvs, geo, assemblers.AffineCoefficient(1.0, 1.0))
    return solvers.FormSystem(asm, kvs, f3, bcs, geo=geo), asm


def notebook(n=200, seed=2024):
    rng = np.random.default_rng(seed)
    centers = []
    while len(centers) < 100:
        cx, cy = 2 * rng.random(2)
        if 1 < np.sqrt(cx ** 2 + cy ** 2) < 2:
            centers.append((cx, cy))

    def diff_coeff(x, y):
        z = np.inf * np.ones_like(x * y)
        for (cx, cy) in centers:
            z = np.minimum(z, (x - cx) ** 2 + (y - cy) ** 2)
        return 0.01 + (np.sqrt(z) < 0.035) * 0.99
    geo = geometry.quarter_annulus()
    kvs = 2 * (bspline.make_knots(3, 0.0, 1.0, n),)
    bcs = assemble.compute_dirichlet_bcs(kvs, geo, [('top', lambda x, y: (4 * (0.25 - (1.5 - y) ** 2)) ** 7), ('left', 0), ('right', 0)])
    form = '(inner(diff_coeff * grad(u), grad(v)) + inner((x[1],-x[0]), grad(u)) * v) * dx'
    return solvers.FormSystem(form, kvs, 0.0, bcs, geo=geo, diff_coeff=diff_coeff), None


CASES = {'c5': (c5, ['kron', 'jacobi']), 'notebook': (notebook, ['kron', 'jacobi'])}


def run(name, tol=1e-8, maxiter=5000):
    make, preconds = CASES[name]
    t0 = time.perf_counter()
    S, keep = make()
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
        spmv_bytes = 2 * (8.0 * nnz * nfree / nall + 16.0 * nall)
        spmv_ms = ti['spmv_ms'] / it
        iter_ms = (ti['spmv_ms'] + ti['precond_ms'] + ti['vector_ms']) / it
        out = {'case': name, 'dim': len(S.kvs), 'p': S.kvs[0].p, 'n': S.kvs[0].numspans, 'ndofs': nall, 'n_free': nfree, 'nnz': nnz,
               'precond': pc, 'tol': tol, 'iterations': ti['iterations'], 'converged': ti['converged'],
               'breakdown': ti['breakdown'], 'relres': ti['relres'],
               'spmv_ms_per_iter': round(spmv_ms, 4), 'precond_ms_per_iter': round(ti['precond_ms'] / it, 4),
               'vector_ms_per_iter': round(ti['vector_ms'] / it, 4), 'iter_ms': round(iter_ms, 4),
               'vector_share': round(ti['vector_ms'] / it / iter_ms, 4) if iter_ms > 0 else None,
               'spmv_TBps': round(spmv_bytes / (spmv_ms * 1e-3) / 1e12, 3) if spmv_ms > 0 else None,
               'solve_wall_s': round(wall, 4), 'solve_device_ms_timed': round(ti['total_ms'], 2),
               'iterations_untimed': S.info['iterations'], 'precond_setup_s': round(t_pc, 4),
               'assemble_ms': round(asm_ms, 3), 'system_setup_s': round(t_setup, 3),
               'u_max': float(np.abs(u).max()), 'u_finite': bool(np.isfinite(u).all())}
        print(json.dumps(out), flush=True)
    S.close()
    if keep is not None:
        keep.patch.close()


if __name__ == '__main__':
    for name in sys.argv[1:] or ['notebook', 'c5']:
        run(name)

#!/usr/bin/env python3
"""Times of the device solve of vector-valued forms (pyiga_amd.solvers.VectorFormSystem, igx_solver_create_block):
  elast2d   linear elasticity on the quarter annulus, p=3 n=128 (2 components), clamped on side (1, 0)
  elast3d   linear elasticity on the cylinder, p=3 n=32 (3 components), clamped on side (0, 0)
with mu = 1, lam = 2 and a constant body force, to a relative residual of 1e-8 by CG, with the block-Kronecker and the Jacobi
preconditioner.  A timed solve records events between the phases of every iteration: device ms of the block SpMV, of the
preconditioner and of the vector kernels per iteration; an untimed solve gives the wall time.  Next to each case the scalar
stiffness matrix of the same patch is solved by PatchSystem (k_spmv), the yardstick of the block SpMV's rate.  Run it under
`rocprofv3 --kernel-trace --stats -- python3 tools/vec_solve_timing.py` for the per-kernel device times.  Prints one JSON line per
(case, preconditioner) and one per scalar yardstick.

Byte budget of one block SpMV: 8 bytes per value of every present block in the free rows of its test component, plus one read of
each of the nc components of x and one write of y (8 * n each); the row tables are a few KB and left out.  The scalar SpMV: 8
per nonzero of the free rows plus 16 * N."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyiga_amd import assemble, bspline, geometry, solvers  # noqa: E402

FORM = '(2*mu*inner(0.5*(grad(u)+grad(u).T), 0.5*(grad(v)+grad(v).T)) + lam*div(u)*div(v)) * dx'


def _case(name):
    if name == 'elast2d':
        kvs = 2 * (bspline.make_knots(3, 0.0, 1.0, 128),)
        return kvs, geometry.quarter_annulus(), (1, 0)
    kvs = 3 * (bspline.make_knots(3, 0.0, 1.0, 32),)
    return kvs, geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.quarter_annulus()), (0, 0)


def _free_nnz(indptr, free):
    return float(np.diff(indptr.astype(np.int64))[free].sum())


def run(name, tol=1e-8, maxiter=5000):
    kvs, geo, side = _case(name)
    d = len(kvs)
    N = int(np.prod([kv.numdofs for kv in kvs]))
    one = assemble.boundary_dofs(kvs, side, ravel=True)
    fixed = np.concatenate([one + c * N for c in range(d)])
    rhs = np.concatenate([np.full(N, 1e-3 * (c + 1)) for c in range(d)])
    t0 = time.perf_counter()
    S = solvers.VectorFormSystem(FORM, kvs, rhs, (fixed, np.zeros(fixed.size)), bfuns=[('u', d), ('v', d)], geo=geo, mu=1.0, lam=2.0)
    t_setup = time.perf_counter() - t0
    indptr, _ = S.patch.pattern()
    nnz = int(indptr[-1])
    free = np.ones(S.n, dtype=bool)
    free[fixed] = False
    present = [(p, q) for p in range(d) for q in range(d) if S.present[p][q]]
    vals_bytes = sum(8.0 * _free_nnz(indptr, free[p * N:(p + 1) * N]) for p, _ in present)
    spmv_bytes = vals_bytes + 8.0 * S.n * 2
    for pc in ('kron', 'jacobi'):
        t0 = time.perf_counter()
        S.set_precond(pc)
        t_pc = time.perf_counter() - t0
        S.solve(tol=tol, maxiter=maxiter, precond=pc, timed=True)
        ti = dict(S.info)
        t0 = time.perf_counter()
        u = S.solve(tol=tol, maxiter=maxiter, precond=pc, check_every=10)
        wall = time.perf_counter() - t0
        it = max(1, ti['iterations'])
        spmv_ms = ti['spmv_ms'] / it
        iter_ms = (ti['spmv_ms'] + ti['precond_ms'] + ti['vector_ms']) / it
        out = {'case': name, 'dim': d, 'ncomp': d, 'p': kvs[0].p, 'n': kvs[0].numspans, 'ndofs': S.n, 'n_free': ti['n_free'],
               'nnz_block': nnz, 'blocks_present': len(present), 'block_values': len(present) * nnz,
               'spmv_bytes': spmv_bytes, 'precond': pc, 'tol': tol, 'method': S.method,
               'iterations': ti['iterations'], 'converged': ti['converged'], 'relres': ti['relres'],
               'spmv_ms_per_iter': round(spmv_ms, 4), 'precond_ms_per_iter': round(ti['precond_ms'] / it, 4),
               'vector_ms_per_iter': round(ti['vector_ms'] / it, 4), 'iter_ms': round(iter_ms, 4),
               'spmv_TBps': round(spmv_bytes / (spmv_ms * 1e-3) / 1e12, 3) if spmv_ms > 0 else None,
               'solve_wall_s': round(wall, 4), 'solve_device_ms_timed': round(ti['total_ms'], 2),
               'iterations_untimed': S.info['iterations'], 'precond_setup_s': round(t_pc, 4), 'system_setup_s': round(t_setup, 3),
               'u_max': float(np.abs(u).max()), 'u_finite': bool(np.isfinite(u).all())}
        print(json.dumps(out), flush=True)
    S.close()
    # the yardstick: k_spmv on the scalar stiffness matrix of the same patch, the first component's Dirichlet dofs
    P = solvers.PatchSystem(kvs, geo, np.full(N, 1e-3), (one, np.zeros(one.size)), kind='stiffness')
    P.solve(tol=tol, maxiter=maxiter, precond='kron', timed=True)
    ti = dict(P.info)
    it = max(1, ti['iterations'])
    freeN = np.ones(N, dtype=bool)
    freeN[one] = False
    sbytes = 8.0 * _free_nnz(indptr, freeN) + 16.0 * N
    sms = ti['spmv_ms'] / it
    print(json.dumps({'case': name + '_scalar_stiffness', 'ndofs': N, 'nnz': nnz, 'iterations': ti['iterations'],
                      'spmv_bytes': sbytes, 'spmv_ms_per_iter': round(sms, 4),
                      'spmv_TBps': round(sbytes / (sms * 1e-3) / 1e12, 3) if sms > 0 else None,
                      'spmv_ms_x_present_blocks': round(sms * len(present), 4)}), flush=True)
    P.close()


if __name__ == '__main__':
    for name in sys.argv[1:] or ['elast2d', 'elast3d']:
        run(name)

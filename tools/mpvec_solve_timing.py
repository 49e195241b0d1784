#!/usr/bin/env python3
"""Times of the device solve of vector-valued forms on a multipatch (pyiga_amd.solvers.MultipatchVectorSystem,
igx_solver_create_multipatch_block):
  notebook2d   linear elasticity on the reference's four-patch notebook domain, p=3 n=128 (2 components)
  cubes3d      linear elasticity on two unit cubes glued on a free face, p=3 n=32 (3 components), clamped at the far end of patch 0
with mu = 1, lam = 2 and a constant body force, to a relative residual of 1e-8 by CG, with the Jacobi and the block-diagonal
Schwarz preconditioner.  A timed solve records events between the phases of every iteration: device ms of the block SpMV
(k_csr_block_spmv), of the preconditioner and of the vector kernels per iteration; an untimed solve gives the wall time.  Next to
each case the scalar stiffness matrix of the same multipatch is solved by MultipatchSystem (k_csr_spmv), the yardstick of the
block SpMV's rate.  Run it under `rocprofv3 --kernel-trace --stats -- python3 tools/mpvec_solve_timing.py` for the per-kernel
device times.  Prints one JSON line per (case, preconditioner) and one per scalar yardstick.

Byte budget of one block SpMV: per nonzero of a scalar row with a free component 4 bytes of index, plus 8 bytes per present
block whose test component is free there; plus one read of each of the nc components of x and one write of y (8 * nc * n each).
The scalar CSR SpMV: 12 per nonzero of the free rows plus 16 * n."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyiga_amd import assemble, bspline, geometry, solvers  # noqa: E402

FORM = '(2*mu*inner(0.5*(grad(u)+grad(u).T), 0.5*(grad(v)+grad(v).T)) + lam*div(u)*div(v)) * dx'
STIFF = 'inner(grad(u),grad(v))*dx'


def _case(name):
    """(multipatch, the clamped sides [(patch, bdspec), ...])"""
    if name == 'notebook2d':
        kvs = 2 * (bspline.make_knots(3, 0.0, 1.0, 128),)
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
    kvs = 3 * (bspline.make_knots(3, 0.0, 1.0, 32),)
    cube = geometry.unit_cube()
    MP = assemble.Multipatch([(kvs, cube), (kvs, cube.translate((1, 0, 0)))])
    MP.join_boundaries(0, (2, 1), 1, (2, 0))
    MP.finalize()
    return MP, [(0, (2, 0))]


def f_one(*x):
    return 1.0 + 0.0 * x[0]


def run(name, tol=1e-8, maxiter=20000):
    MP, sides = _case(name)
    nc = len(MP.patches[0][0])
    n = MP.numdofs
    one = np.unique(np.concatenate([MP.patch_to_global_idx(p)[assemble.boundary_dofs(MP.patches[p][0], bd, ravel=True)]
                                    for p, bd in sides]))
    fixed = np.concatenate([one + c * n for c in range(nc)])
    rhs = np.concatenate([np.full(n, 1e-3 * (c + 1)) for c in range(nc)])
    t0 = time.perf_counter()
    S = solvers.MultipatchVectorSystem(MP, FORM, rhs, (fixed, np.zeros(fixed.size)), bfuns=[('u', nc), ('v', nc)], mu=1.0, lam=2.0)
    t_setup = time.perf_counter() - t0
    indptr, _ = MP.pattern()
    lens = np.diff(indptr.astype(np.int64))
    nnz = int(indptr[-1])
    free = np.ones(S.n, dtype=bool)
    free[fixed] = False
    fr = free.reshape(nc, n)
    present = [(p, q) for p in range(nc) for q in range(nc) if S.present[p][q]]
    spmv_bytes = 4.0 * lens[fr.any(axis=0)].sum() + sum(8.0 * lens[fr[p]].sum() for p, _ in present) + 16.0 * S.n
    for pc in ('jacobi', 'schwarz'):
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
        out = {'case': name, 'patches': MP.numpatches, 'ncomp': nc, 'p': MP.patches[0][0][0].p, 'n': MP.patches[0][0][0].numspans,
               'ndofs': S.n, 'n_free': ti['n_free'], 'nnz_block': nnz, 'blocks_present': len(present),
               'block_values': len(present) * nnz, 'spmv_bytes': spmv_bytes, 'precond': pc, 'tol': tol, 'method': S.method,
               'iterations': ti['iterations'], 'converged': ti['converged'], 'relres': ti['relres'],
               'spmv_ms_per_iter': round(spmv_ms, 4), 'precond_ms_per_iter': round(ti['precond_ms'] / it, 4),
               'vector_ms_per_iter': round(ti['vector_ms'] / it, 4), 'iter_ms': round(iter_ms, 4),
               'spmv_TBps': round(spmv_bytes / (spmv_ms * 1e-3) / 1e12, 3) if spmv_ms > 0 else None,
               'solve_wall_s': round(wall, 4), 'solve_device_ms_timed': round(ti['total_ms'], 2),
               'iterations_untimed': S.info['iterations'], 'precond_setup_s': round(t_pc, 4), 'system_setup_s': round(t_setup, 3),
               'u_max': float(np.abs(u).max()), 'u_finite': bool(np.isfinite(u).all())}
        print(json.dumps(out), flush=True)
    S.close()
    # the yardstick: k_csr_spmv on the scalar stiffness matrix of the same multipatch, one component's Dirichlet dofs
    P = solvers.MultipatchSystem(MP, STIFF, 'f*v*dx', bcs=(one, np.zeros(one.size)), f=f_one)
    P.solve(tol=tol, maxiter=maxiter, precond='jacobi', timed=True)
    ti = dict(P.info)
    it = max(1, ti['iterations'])
    freeN = np.ones(n, dtype=bool)
    freeN[one] = False
    sbytes = 12.0 * lens[freeN].sum() + 16.0 * n
    sms = ti['spmv_ms'] / it
    print(json.dumps({'case': name + '_scalar_stiffness', 'ndofs': n, 'nnz': nnz, 'iterations': ti['iterations'],
                      'spmv_bytes': sbytes, 'spmv_ms_per_iter': round(sms, 4),
                      'spmv_TBps': round(sbytes / (sms * 1e-3) / 1e12, 3) if sms > 0 else None,
                      'spmv_ms_x_present_blocks': round(sms * len(present), 4)}), flush=True)
    P.close()
    MP.close()


if __name__ == '__main__':
    for name in sys.argv[1:] or ['notebook2d', 'cubes3d']:
        run(name)

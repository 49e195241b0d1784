#!/usr/bin/env python3
"""Times of the device solve of vector-valued forms on a multipatch with the multigrid preconditioner
(pyiga_amd.solvers.MultipatchVectorSystem.set_multigrid, igx_solver_set_block_mg_*) against Jacobi and the
block-diagonal Schwarz preconditioner, on the two cases of tools/mpvec_solve_timing.py:
  notebook2d   linear elasticity on the reference's four-patch notebook domain, p=3 n=128 (2 components)
  cubes3d      linear elasticity on two unit cubes glued on a free face, p=3 n=32 (3 components), clamped at the far end of patch 0
with mu = 1, lam = 2 and a constant body force, to a relative residual of 1e-8 by CG.  Per preconditioner: the iterations, the wall
time of an untimed solve (the median of five), and from a timed solve the device ms per iteration of the block SpMV, of the
preconditioner and of the vector kernels.  For 'mg' also the set-up time, the levels (mg_info) and the phases of one V-cycle
(mg_profile).  Prints one JSON line per (case, preconditioner)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pyiga_amd import assemble, solvers  # noqa: E402
from mpvec_solve_timing import FORM, _case  # noqa: E402


def run(name, tol=1e-8, maxiter=20000):
    MP, sides = _case(name)
    nc = len(MP.patches[0][0])
    n = MP.numdofs
    one = np.unique(np.concatenate([MP.patch_to_global_idx(p)[assemble.boundary_dofs(MP.patches[p][0], bd, ravel=True)]
                                    for p, bd in sides]))
    fixed = np.concatenate([one + c * n for c in range(nc)])
    rhs = np.concatenate([np.full(n, 1e-3 * (c + 1)) for c in range(nc)])
    S = solvers.MultipatchVectorSystem(MP, FORM, rhs, (fixed, np.zeros(fixed.size)), bfuns=[('u', nc), ('v', nc)], mu=1.0, lam=2.0)
    base = {'case': name, 'patches': MP.numpatches, 'ncomp': nc, 'p': MP.patches[0][0][0].p, 'n': MP.patches[0][0][0].numspans,
            'ndofs': S.n, 'tol': tol}
    for pc in ('jacobi', 'schwarz', 'mg'):
        t0 = time.perf_counter()
        if pc == 'mg':
            S.set_multigrid()
        S.set_precond(pc)
        t_pc = time.perf_counter() - t0
        S.solve(tol=tol, maxiter=maxiter, precond=pc, timed=True)
        ti = dict(S.info)
        walls = []
        for _ in range(5):
            t0 = time.perf_counter()
            u = S.solve(tol=tol, maxiter=maxiter, precond=pc, check_every=10 if pc != 'mg' else 1)
            walls.append(time.perf_counter() - t0)
        it = max(1, ti['iterations'])
        out = dict(base, precond=pc, iterations=ti['iterations'], converged=ti['converged'], relres=ti['relres'],
                   iterations_untimed=S.info['iterations'], solve_wall_ms_median5=round(1e3 * float(np.median(walls)), 3),
                   solve_wall_ms_min=round(1e3 * min(walls), 3), solve_device_ms_timed=round(ti['total_ms'], 2),
                   spmv_ms_per_iter=round(ti['spmv_ms'] / it, 4), precond_ms_per_iter=round(ti['precond_ms'] / it, 4),
                   vector_ms_per_iter=round(ti['vector_ms'] / it, 4), precond_setup_s=round(t_pc, 3),
                   u_max=float(np.abs(u).max()), u_finite=bool(np.isfinite(u).all()))
        if pc == 'mg':
            prof = S.mg_profile(reps=5)
            out['mg_levels'] = [dict(spans=i['spans'][0], dofs=i['dofs'], free=i['free'], nnz=i['nnz'], colours=i['colours'],
                                     dense_inverse=i['dense_inverse']) for i in S.mg_info()]
            out['mg_profile'] = {k: ([round(float(x), 4) for x in v] if isinstance(v, list) else
                                     (round(float(v), 4) if isinstance(v, float) else v)) for k, v in prof.items()}
        print(json.dumps(out), flush=True)
    S.close()
    MP.close()


if __name__ == '__main__':
    for name in sys.argv[1:] or ['notebook2d', 'cubes3d']:
        run(name)

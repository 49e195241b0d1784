#!/usr/bin/env python3
"""Times of the multipatch Dirichlet solve with the multigrid preconditioner (solvers.MultipatchSystem.solve(precond='mg'))
against Jacobi and Schwarz on the same build: the notebook domain (2D, p = 3, n = 64 and 256, the Dirichlet sides of the
reference's notebook) and three cubes around an edge (3D, p = 2, n = 32 and 64, two outer faces fixed), PCG to a relative residual
of 1e-8.  Per (case, preconditioner): the set-up time, the median wall time of five untimed solves, and one timed solve (device
ms per iteration of the SpMV, the preconditioner and the vector kernels); for 'mg' also the hierarchy (free dofs, colours, one-block
sweeps per level) and the device time of the phases of one V-cycle with the kernels it launches (mg_profile).  Without arguments
every (case, preconditioner) runs in a process of its own under a time limit, one after the other, and the run stops at the first
that fails; `mg_timing.py <case> <precond>` runs one.  Prints one JSON line per (case, preconditioner)."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ['notebook_p3_n64', 'notebook_p3_n256', 'cubes_p2_n32', 'cubes_p2_n64']
PRECONDS = ['jacobi', 'schwarz', 'mg']
LIMIT_S = 240


def f2(x, y):
    return np.exp(-5 * ((x - 0.3) ** 2 + (y - 1) ** 2))


def g2(x, y):
    return 1e-1 * np.sin(8 * x)


def f3(x, y, z):
    return 1.0 + x * y - z


def g3(x, y, z):
    return x + 0.5 * y * z


def domain(case):
    from pyiga_amd import assemble, bspline, geometry
    which, p, n = case.split('_')
    p, n = int(p[1:]), int(n[1:])
    if which == 'notebook':
        kvs = 2 * (bspline.make_knots(p, 0.0, 1.0, n),)
        geos = [geometry.quarter_annulus(), geometry.unit_square().translate((-1, 1)),
                geometry.quarter_annulus().rotate_2d(np.pi).translate((-1, 3)),
                geometry.quarter_annulus().rotate_2d(-np.pi / 2).translate((-2, 1))]
        MP = assemble.Multipatch([(kvs, g) for g in geos], automatch=True)
        sides = [(0, 'bottom'), (0, 'right'), (1, 'top'), (2, 'left'), (2, 'bottom'), (3, 'bottom')]
        return MP, f2, [(q, bd, g2) for q, bd in sides]
    kvs = 3 * (bspline.make_knots(p, 0.0, 1.0, n),)
    cube = geometry.unit_cube()
    geos = [cube, cube.translate((1, 0, 0)), cube.scale((-1, 1, 1)).translate((1, 1, 0))]
    MP = assemble.Multipatch([(kvs, g) for g in geos], automatch=True)
    return MP, f3, [(0, (0, 0), g3), (2, (2, 1), g3)]


def run(case, pc, tol=1e-8, maxiter=5000, reps=5):
    from pyiga_amd import solvers
    MP, f, bdconds = domain(case)
    bcs = MP.compute_dirichlet_bcs(bdconds)
    t0 = time.perf_counter()
    S = solvers.MultipatchSystem(MP, 'inner(grad(u),grad(v))*dx', 'f*v*dx', bcs=bcs, f=f)
    t_system = time.perf_counter() - t0
    t0 = time.perf_counter()
    S.set_precond(pc)
    t_pc = time.perf_counter() - t0
    S.solve(tol=tol, maxiter=maxiter, precond=pc)                  # (warm-up: first launches)
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        u = S.solve(tol=tol, maxiter=maxiter, precond=pc, check_every=1 if pc == 'mg' else 10)
        walls.append(time.perf_counter() - t0)
    it_untimed = S.info['iterations']
    S.solve(tol=tol, maxiter=maxiter, precond=pc, timed=True)
    ti = dict(S.info)
    it = max(1, ti['iterations'])
    out = {'case': case, 'precond': pc, 'ndofs': MP.numdofs, 'n_free': ti['n_free'], 'nnz': MP.info()['nnz'], 'tol': tol,
           'iterations': ti['iterations'], 'iterations_untimed': it_untimed, 'converged': ti['converged'], 'relres': ti['relres'],
           'solve_wall_ms_median': round(1e3 * float(np.median(walls)), 3), 'solve_wall_ms_all': [round(1e3 * w, 3) for w in walls],
           'spmv_ms_per_iter': round(ti['spmv_ms'] / it, 4), 'precond_ms_per_iter': round(ti['precond_ms'] / it, 4),
           'vector_ms_per_iter': round(ti['vector_ms'] / it, 4), 'solve_device_ms_timed': round(ti['total_ms'], 2),
           'precond_setup_s': round(t_pc, 3), 'system_setup_s': round(t_system, 3), 'u_max': float(np.abs(u).max())}
    if pc == 'mg':
        pf = S.mg_profile(reps=5)
        out['levels'] = [{k: d[k] for k in ('spans', 'free', 'nnz', 'colours', 'one_block', 'dense_inverse')} | {'spans': d['spans'][0]}
                         for d in S.mg_info()]
        out['vcycle'] = {k: ([round(x, 4) for x in v] if isinstance(v, list) else round(v, 4) if isinstance(v, float) else v)
                         for k, v in pf.items()}
    print(json.dumps(out), flush=True)
    S.close()
    MP.close()


if __name__ == '__main__':
    if len(sys.argv) == 3:
        run(sys.argv[1], sys.argv[2])
    else:
        cases = [c for c in CASES if not sys.argv[1:] or c in sys.argv[1:]]
        for case in cases:
            for pc in PRECONDS:
                try:
                    rc = subprocess.run([sys.executable, os.path.abspath(__file__), case, pc], timeout=LIMIT_S).returncode
                except subprocess.TimeoutExpired:
                    rc = 124
                if rc != 0:
                    print(json.dumps({'case': case, 'precond': pc, 'failed': rc}), flush=True)
                    sys.exit(1)                                    # (nothing more is started on the device after a failure)

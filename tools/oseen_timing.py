#!/usr/bin/env python3
"""Device time of the Oseen solver (`solvers.OseenSystem`, csrc/solve_gmres.hip) on the enclosed problem of
tools/saddle_timing.py (velocity 0 on the whole boundary, right-hand side 1 in every velocity entry, Taylor-Hood p = 3 / 2) with
the rotating wind w = (-y, x) (3D: w = (0, -z, y) in the plane of the annulus, 0.25 along the axis) and viscosity 1:
  nb2d  the quarter annulus, 50 x 25 spans
  th3d  the quarter-annulus cylinder, n = 32 spans per axis
  th0   a small smoke case (printed only)
Per case, with the Kronecker preconditioner in its block-diagonal and its block-triangular form and restart 20 and 40:
`solve(tol=1e-8, maxiter=MAXITER, timed=True)`, median of REPS runs after WARMUP ones, from the solver's device events -- steps,
restarts, the whole solve, and per step the product, the preconditioner and the orthogonalisation (with its bytes/s over the
budget of section 32 at the mean column count), and per cycle the update of x.  The orthogonalisation alone at 10, 20 and 40
columns through `igx_solver_gmres_orth_d`.  For comparison MINRES (`solvers.SaddlePointSystem`) on the same spaces without the
convection term.  One JSON line per case, appended to profiles/oseen_timing.txt (`--out PATH`: elsewhere).  A record, not a
threshold.

One case per process, each under its own time limit, the steps chained so that a failure ends the run:
  timeout -k 10 300 python tools/oseen_timing.py nb2d && timeout -k 10 600 python tools/oseen_timing.py th3d
"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyiga_amd import _lib, assemble, bspline, geometry, solvers  # noqa: E402
from pyiga_amd.operators import DeviceArray  # noqa: E402

REPS, WARMUP = 7, 2
MAXITER = 400
MB = 8
CASES = {'nb2d': (2, (50, 25)), 'th3d': (3, (32, 32, 32)), 'th0': (2, (6, 4))}


def orth_budget(n, c):
    """Bytes of one orthogonalisation against c columns by the budget of DESIGN.md section 32: two k_gm_dots passes of
    8 n (c + ceil(c / MB)) and two k_gm_update passes of 8 n (c + 2 ceil(c / MB))."""
    ch = -(-c // MB)
    return 2 * 8.0 * n * (c + ch) + 2 * 8.0 * n * (c + 2 * ch)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'oseen_timing.txt')
    if '--out' in sys.argv:
        out = sys.argv[sys.argv.index('--out') + 1]
        args.remove(out)
    name = args[0] if args else 'th0'
    dim, n_el = CASES[name]
    ku = tuple(bspline.make_knots(3, 0.0, 1.0, n, mult=2) for n in n_el)
    kp = tuple(bspline.make_knots(2, 0.0, 1.0, n) for n in n_el)
    geo = geometry.quarter_annulus()
    sides = ['bottom', 'top', 'left', 'right']
    wind = lambda x, y: (-y, x)
    if dim == 3:
        geo = geometry.tensor_product(geometry.line_segment(0.0, 1.0), geo)
        sides += ['front', 'back']
        wind = lambda x, y, z: (0.25 + 0.0 * x, -z, y)
    zero = (lambda x, y: (0.0, 0.0)) if dim == 2 else (lambda x, y, z: (0.0, 0.0, 0.0))
    bcs = assemble.compute_dirichlet_bcs(ku, geo, [(s, zero) for s in sides])
    lib = _lib.load()
    S = solvers.OseenSystem((ku, kp), geo, bcs, rhs=1.0, w=wind)
    rec = {'case': name, 'spans': list(n_el), 'unknowns': S.n, 'reps': REPS, 'warmup': WARMUP, 'maxiter': MAXITER, 'solves': []}
    for tri in (False, True):
        for restart in (20, 40):
            runs = []
            for k in range(WARMUP + REPS):
                S.solve(tol=1e-8, maxiter=MAXITER, triangular=tri, restart=restart, timed=True)
                if k >= WARMUP:
                    cm = C.c_float()
                    _lib.check(lib.igx_solver_gmres_timing(S.handle, None, C.byref(cm)), 'igx_solver_gmres_timing')
                    runs.append(dict(S.info, combine_ms=cm.value))
            med = lambda key: float(np.median([r[key] for r in runs]))
            its, restarts = runs[0]['iterations'], runs[0]['restarts']
            # the columns step j of a cycle orthogonalises against: j + 1
            cols = [(j % restart) + 1 for j in range(its)]
            budget = float(np.mean([orth_budget(S.n, c) for c in cols]))
            # (vector_ms holds the orthogonalisations and the updates of x)
            orth_ms = (med('vector_ms') - med('combine_ms') * (restarts + 1)) / its
            rec['solves'].append({
                'triangular': tri, 'restart': restart, 'steps': its, 'restarts': restarts, 'converged': bool(runs[0]['converged']),
                'relres': runs[0]['relres'], 'solve_ms': round(med('total_ms'), 3), 'product_ms_per_step': round(med('spmv_ms') / its, 5),
                'precond_ms_per_step': round(med('precond_ms') / its, 5), 'orth_ms_per_step': round(orth_ms, 5),
                'mean_columns': round(float(np.mean(cols)), 2), 'orth_budget_GBps': round(budget / (orth_ms * 1e-3) / 1e9, 1),
                'update_ms_per_cycle': round(med('combine_ms'), 5)})
    # the orthogonalisation alone
    _lib.check(lib.igx_solver_set_gmres(S.handle, 40, 0), 'igx_solver_set_gmres')
    ctx = S.patch.ctx
    rng = np.random.default_rng(0)
    d_V = DeviceArray.from_host(ctx, rng.standard_normal(41 * S.n) / np.sqrt(S.n))
    rec['orth'] = []
    for c in (10, 20, 40):
        ms = []
        for k in range(WARMUP + REPS):
            d_w = DeviceArray.from_host(ctx, rng.standard_normal(S.n))
            _lib.check(lib.igx_solver_gmres_orth_d(S.handle, d_V.ptr, c, d_w.ptr, None, None), 'igx_solver_gmres_orth_d')
            t = C.c_float()
            _lib.check(lib.igx_solver_gmres_timing(S.handle, C.byref(t), None), 'igx_solver_gmres_timing')
            if k >= WARMUP:
                ms.append(t.value)
        m = float(np.median(ms))
        rec['orth'].append({'columns': c, 'ms': round(m, 5), 'budget_GBps': round(orth_budget(S.n, c) / (m * 1e-3) / 1e9, 1)})
    S.close()
    # MINRES on the same spaces without the convection term
    M = solvers.SaddlePointSystem((ku, kp), geo, bcs, rhs=1.0)
    runs = []
    for k in range(WARMUP + REPS):
        M.solve(tol=1e-8, maxiter=5000, timed=True)
        if k >= WARMUP:
            runs.append(dict(M.info))
    its = runs[0]['iterations']
    med = lambda key: float(np.median([r[key] for r in runs]))
    rec['minres_stokes'] = {'iterations': its, 'converged': bool(runs[0]['converged']), 'solve_ms': round(med('total_ms'), 3),
                            'product_ms_per_iteration': round(med('spmv_ms') / its, 5),
                            'precond_ms_per_iteration': round(med('precond_ms') / its, 5),
                            'vector_ms_per_iteration': round(med('vector_ms') / its, 5)}
    M.close()
    print(json.dumps(rec), flush=True)
    if name != 'th0':
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, 'a') as f:
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()

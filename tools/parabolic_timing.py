#!/usr/bin/env python3
"""Times of the device DIRK integration of the heat equation (pyiga_amd.solvers.ParabolicSystem):
  c2   2D quarter annulus, p=3 n=256
  c4   3D quarter-annulus cylinder, p=4 n=128 (1.59 G values per matrix)
with f = 1, u0 = 0, zero Dirichlet data on every side, tau = 1e-3, 10 steps of sdirk3 and of crank_nicolson, stage solves by CG
with the Kronecker preconditioner to a relative residual of 1e-10.  A timed run records events between the phases of every stage
(igx_dirk_info): device ms of forming C (k_vals_axpby, against its budget of 24 bytes per value), of the M x and F products, of
the stage combinations and of the solves; an untimed run gives the wall time.  Run it under
`rocprofv3 --kernel-trace --stats -- python3 tools/parabolic_timing.py c4` for the per-kernel device times.  Prints one JSON
line per (case, scheme)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyiga_amd import bspline, geometry, solvers  # noqa: E402


def _case(name):
    if name == 'c2':
        return 2 * (bspline.make_knots(3, 0.0, 1.0, 256),), geometry.quarter_annulus()
    return 3 * (bspline.make_knots(4, 0.0, 1.0, 128),), geometry.tensor_product(geometry.line_segment(0.0, 1.0),
                                                                                 geometry.quarter_annulus())


def _boundary(ndofs):
    idx = np.indices(ndofs).reshape(len(ndofs), -1)
    on = np.zeros(idx.shape[1], dtype=bool)
    for k, n in enumerate(ndofs):
        on |= (idx[k] == 0) | (idx[k] == n - 1)
    return np.flatnonzero(on)


def run(name, tau=1e-3, nsteps=10):
    kvs, geo = _case(name)
    ndofs = tuple(kv.numdofs for kv in kvs)
    fixed = _boundary(ndofs)
    t = time.perf_counter()
    S = solvers.ParabolicSystem(kvs, geo, np.full(int(np.prod(ndofs)), 1.0), bcs=(fixed, np.zeros(fixed.size)))
    setup_s = time.perf_counter() - t
    nvals = S.patch.nnz
    u0 = np.zeros(S.n)
    try:
        for scheme in ('sdirk3', 'crank_nicolson'):
            S.integrate(u0, tau, (nsteps - 0.5) * tau, scheme=scheme, save_every=nsteps, timed=True)
            info = dict(S.info)
            t = time.perf_counter()
            S.integrate(u0, tau, (nsteps - 0.5) * tau, scheme=scheme, save_every=nsteps)
            wall = time.perf_counter() - t
            its = info['stage_iterations']
            axpby_gbs = 24.0 * nvals / (info['axpby_ms'] * 1e-3) / 1e9 if info['axpby_ms'] > 0 else None
            print(json.dumps({
                'case': name, 'scheme': scheme, 'ndofs': list(ndofs), 'values': int(nvals), 'steps': int(info['steps']),
                'converged': bool(info['converged']), 'stage_iterations': its.tolist(),
                'mean_iterations_per_stage': float(its.mean()),
                'axpby_ms': round(info['axpby_ms'], 3), 'axpby_GBs': round(axpby_gbs, 1) if axpby_gbs else None,
                'per_step_ms': {k: round(info[k] / info['steps'], 3) for k in ('spmv_ms', 'combine_ms', 'solve_ms')},
                'solve_ms_per_iteration': round(info['solve_ms'] / max(1, int(info['iterations'])), 3),
                'run_wall_s_untimed': round(wall, 3), 'setup_s': round(setup_s, 2)}), flush=True)
    finally:
        S.close()


if __name__ == '__main__':
    for c in (sys.argv[1:] or ['c2', 'c4']):
        run(c)

#!/usr/bin/env python3
"""Times of the adaptive device integration of the heat equation (pyiga_amd.solvers.ParabolicSystem.integrate_adaptive; DESIGN.md
section 18), the twin of tools/parabolic_timing.py:
  c2   2D quarter annulus, p=3 n=256
  c4   3D quarter-annulus cylinder, p=4 n=128 (1.59 G values per matrix)
with f = 1, u0 = 0, zero Dirichlet data on every side, from tau0 = 1e-3 to t_end = 0.05 with tol = 1e-3, by esdirk23 and rodasp,
every solve by CG with the Kronecker preconditioner to a relative residual of 1e-10.  A timed run records events between the
phases of every attempt (igx_step_info); an untimed run gives the wall time.  For comparison the constant-step sdirk3 run with
tau = 1e-3 to the same t_end (the adaptive runs end later: their last step passes t_end).  k_err_norm is timed
alone through igx_solver_error_ratio_d against its budget of (nv + 1) 8 + 1 bytes per dof.  Prints one JSON line per run."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyiga_amd import bspline, geometry, solvers  # noqa: E402
from parabolic_timing import _boundary, _case  # noqa: E402


def run(name, tau0=1e-3, t_end=0.05, tol=1e-3):
    kvs, geo = _case(name)
    ndofs = tuple(kv.numdofs for kv in kvs)
    fixed = _boundary(ndofs)
    S = solvers.ParabolicSystem(kvs, geo, np.full(int(np.prod(ndofs)), 1.0), bcs=(fixed, np.zeros(fixed.size)))
    u0 = np.zeros(S.n)
    try:
        t = time.perf_counter()
        S.integrate(u0, tau0, t_end, scheme='sdirk3', save_every=10 ** 9)
        const_wall = time.perf_counter() - t
        const_info = dict(S.info)
        print(json.dumps({'case': name, 'scheme': 'sdirk3', 'constant_tau': tau0, 'steps': int(const_info['steps']),
                          'iterations': int(const_info['iterations']), 'run_wall_s': round(const_wall, 3)}), flush=True)
        for scheme in ('esdirk23', 'rodasp'):
            S.integrate_adaptive(u0, tau0, t_end, tol, scheme=scheme, save_every=10 ** 9, timed=True)
            info = dict(S.info)
            t = time.perf_counter()
            times, sols = S.integrate_adaptive(u0, tau0, t_end, tol, scheme=scheme, save_every=10 ** 9)
            wall = time.perf_counter() - t
            n = max(1, info['attempts'])
            print(json.dumps({
                'case': name, 'scheme': scheme, 'ndofs': list(ndofs), 'tol': tol, 't_final': float(times[-1]),
                'attempts': int(info['attempts']), 'rejections': int(info['rejections']), 'reformations': int(info['reformations']),
                'tau_first_last': [float(info['tau'][0]), float(info['tau'][-1])],
                'stage_iterations': int(info['stage_iterations'].sum()), 'mass_iterations': int(info['mass_iterations'].sum()),
                'per_attempt_ms': {k: round(info[k] / n, 3) for k in ('axpby_ms', 'spmv_ms', 'combine_ms', 'solve_ms', 'mass_ms',
                                                                        'err_ms', 'total_ms')},
                'run_wall_s_untimed': round(wall, 3), 'constant_sdirk3_wall_s': round(const_wall, 3)}), flush=True)
        # k_err_norm alone (with its finishing kernel and the read-back of one double), 3 vectors
        rng = np.random.default_rng(0)
        V, x = [rng.standard_normal(S.n) for _ in range(3)], rng.standard_normal(S.n)
        from pyiga_amd import _lib
        from pyiga_amd.operators import DeviceArray
        import ctypes as C
        dev = [DeviceArray.from_host(S._ctx, v) for v in V + [x]]
        ptrs = (C.c_void_p * 3)(*[d.ptr for d in dev[:3]])
        coef = np.array([1.0, -1.0, 0.5])
        r = C.c_double()
        fn = _lib.load().igx_solver_error_ratio_d
        fn(S.handle, 3, _lib.dptr(coef), ptrs, dev[3].ptr, 1e-3, C.byref(r))
        reps = 20
        t = time.perf_counter()
        for _ in range(reps):
            fn(S.handle, 3, _lib.dptr(coef), ptrs, dev[3].ptr, 1e-3, C.byref(r))
        ms = (time.perf_counter() - t) / reps * 1e3
        nbytes = (4 * 8 + 1) * S.n
        print(json.dumps({'case': name, 'kernel': 'k_err_norm + k_fin + read-back, 3 vectors', 'dofs': S.n, 'bytes': nbytes,
                          'wall_ms_per_call': round(ms, 4), 'GBs': round(nbytes / ms / 1e6, 1)}), flush=True)
    finally:
        S.close()


if __name__ == '__main__':
    for c in (sys.argv[1:] or ['c2', 'c4']):
        run(c)

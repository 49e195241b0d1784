#!/usr/bin/env python3
"""Device time of a nonlinear step of the stationary Navier-Stokes solver (`solvers.NavierStokesSystem`) on
the enclosed problem of tools/oseen_timing.py (velocity 0 on the whole boundary, right-hand side 1 in every velocity entry,
Taylor-Hood p = 3 / 2, viscosity 1, no pinned pressure dof):
  nb2d  the quarter annulus, 50 x 25 spans
  th3d  the quarter-annulus cylinder, n = 32 spans per axis
  th0   a small smoke case (printed only)
Per case and method (Picard, Newton): `solve(timed=True)` from the Stokes solution, restart 40, triangular Kronecker
preconditioner, at most MAXSTEPS steps; per step the medians over the steps of the wind evaluation (`igx_patch_eval_vspline_d`,
the library's events), of the assemblies (sum of `igx_assemble`'s events over the blocks of the step) and of the correction solve
(`igx_solver_saddle_correct_d`).  Measured apart on the last iterate, medians of REPS runs after WARMUP: the table formation
(`igx_patch_set_form_sum_d` of one diagonal block; HOST wall time of the synchronous call, the library records no event for it),
the residual product (`igx_solver_saddle_product_d`, velocity-row and pressure-row launch), and the fused evaluation of the wind
against nc calls of `igx_patch_eval_spline_d` on the same patch, value alone and with the gradient.  One JSON line per case,
appended to profiles/ns_timing.txt (`--out PATH`: elsewhere).  A record, not a threshold.

One case per process, each under its own time limit, the steps chained so that a failure ends the run:
  timeout -k 10 300 python tools/ns_timing.py nb2d && timeout -k 10 900 python tools/ns_timing.py th3d
"""
import ctypes as C
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyiga_amd import _lib, assemble, bspline, geometry, solvers  # noqa: E402
from pyiga_amd.operators import DeviceArray  # noqa: E402

REPS, WARMUP = 7, 2
MAXSTEPS = 6
CASES = {'nb2d': (2, (50, 25)), 'th3d': (3, (32, 32, 32)), 'th0': (2, (6, 4))}


def med(xs):
    return round(float(np.median(xs)), 5) if len(xs) else None


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'ns_timing.txt')
    if '--out' in sys.argv:
        out = sys.argv[sys.argv.index('--out') + 1]
        args.remove(out)
    name = args[0] if args else 'th0'
    dim, n_el = CASES[name]
    ku = tuple(bspline.make_knots(3, 0.0, 1.0, n, mult=2) for n in n_el)
    kp = tuple(bspline.make_knots(2, 0.0, 1.0, n) for n in n_el)
    geo = geometry.quarter_annulus()
    sides = ['bottom', 'top', 'left', 'right']
    if dim == 3:
        geo = geometry.tensor_product(geometry.line_segment(0.0, 1.0), geo)
        sides += ['front', 'back']
    zero = (lambda x, y: (0.0, 0.0)) if dim == 2 else (lambda x, y, z: (0.0, 0.0, 0.0))
    bcs = assemble.compute_dirichlet_bcs(ku, geo, [(s, zero) for s in sides])
    lib = _lib.load()
    S = solvers.NavierStokesSystem((ku, kp), geo, bcs, rhs=1.0, viscosity=1.0, restart=40)
    nc = S.ncomp
    rec = {'case': name, 'spans': list(n_el), 'unknowns': S.n, 'gauss_points': S.patch.resident_points(), 'reps': REPS, 'warmup': WARMUP,
           'methods': []}
    u = None
    for method in ('picard', 'newton'):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            try:
                u = S.solve(method=method, maxiter=MAXSTEPS, rtol=1e-6, atol=0.0, lin_tol=1e-8, lin_maxiter=400, timed=True)
            except solvers.NoConvergenceError as e:
                u = e.last_iterate
        ph = S.info['phases']
        steps = S.info['iterations']
        wind = [p['wind_ms'] for p in ph if 'wind_ms' in p]
        asm = [p for p in ph if 'assembly_ms' in p]
        # per step: the Picard blocks (every residual) and, for Newton, the group of all blocks that follows
        diag = [p['assembly_ms'] for p in asm if p['blocks'] == nc]
        full = [p['assembly_ms'] for p in asm if p['blocks'] == nc * nc]
        rec['methods'].append({
            'method': method, 'steps': steps, 'converged': bool(S.info['converged']),
            'residual_norms': ['%.3e' % r for r in S.info['residual_norms']], 'inner_iterations': S.info['inner_iterations'],
            'restarts': S.info['restarts'], 'blocks_assembled': S.info['blocks_assembled'],
            'wind_ms': med(wind), 'assembly_ms_diagonal_blocks': med(diag), 'assembly_ms_all_blocks': med(full),
            'solve_ms': med([p['solve_ms'] for p in ph if 'solve_ms' in p]), 'stokes_ms': round(float(S.info['stokes']['total_ms']), 3)})
    # apart, on the last iterate
    ctx = S.patch.ctx
    d_u = DeviceArray.from_host(ctx, u[:nc * S.N])
    atab = S._device_a_tables()
    ms = {'fused': [], 'fused_grad': [], 'scalar': [], 'scalar_grad': [], 'table_host': [], 'product_u': [], 'product_p': []}
    d_x, d_y = DeviceArray.from_host(ctx, u), DeviceArray(ctx, S.n)
    for k in range(WARMUP + REPS):
        t = {}
        for grad in (False, True):
            vals, grads = S.patch.eval_vspline(d_u.ptr, nc, want_grad=grad)
            t['fused_grad' if grad else 'fused'] = S.patch.timing()['total_ms']
            tot = 0.0
            for c in range(nc):
                S.patch.eval_spline(d_u.ptr + 8 * c * S.N, want_grad=grad)
                tot += S.patch.timing()['total_ms']
            t['scalar_grad' if grad else 'scalar'] = tot
        vals, grads = S.patch.eval_vspline(d_u.ptr, nc, want_grad=False)
        b = [[None] * 4 for _ in range(4)]
        for j in range(dim):
            b[0][1 + j] = vals[j]
        t0 = time.perf_counter()
        S.patch.set_form_sum_resident(atab[0][0], S.viscosity, b)
        t['table_host'] = (time.perf_counter() - t0) * 1e3
        _lib.check(lib.igx_solver_saddle_product_d(S.handle, d_x.ptr, None, -1.0, None, d_y.ptr, None), 'igx_solver_saddle_product_d')
        pu, pp = C.c_float(), C.c_float()
        _lib.check(lib.igx_solver_saddle_timing(S.handle, None, C.byref(pu), C.byref(pp)), 'igx_solver_saddle_timing')
        t['product_u'], t['product_p'] = pu.value, pp.value
        if k >= WARMUP:
            for key, v in t.items():
                ms[key].append(v)
    rec['apart'] = {'eval_fused_ms': med(ms['fused']), 'eval_%d_scalar_calls_ms' % nc: med(ms['scalar']),
                    'eval_fused_grad_ms': med(ms['fused_grad']), 'eval_%d_scalar_calls_grad_ms' % nc: med(ms['scalar_grad']),
                    'table_formation_host_ms': med(ms['table_host']), 'residual_product_u_rows_ms': med(ms['product_u']),
                    'residual_product_p_rows_ms': med(ms['product_p'])}
    S.close()
    print(json.dumps(rec), flush=True)
    if name != 'th0':
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, 'a') as f:
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Times of the local multigrid on hierarchical spline spaces (`pyiga_amd.solvers.HierarchicalSystem`, csrc/hmg.hip; DESIGN.md
section 36) on the two cases of tools/bench_hier.py: stiffness on the B-spline quarter annulus, 2D p = 3, HB-splines with
disparity 1 refined towards the diagonal, all sides Dirichlet, right-hand side cos(x) exp(y):

  diag32  base 32 x 32 spans, L = 4
  diag64  base 64 x 64 spans, L = 5   (level 0 keeps more than 2048 dofs: coarse_max is raised to 8192)
  diag8   base 8 x 8 spans, L = 2 (smoke case)

Per case: the assembly (values stay on the device), the set-up of the hierarchy (patterns of the triple products and colourings
on the host, Galerkin products on the device, dense inverse of level 0 on the host), iteration counts and wall-clock times of
`method='iterate'` and `method='cg'` (smoother gs, two steps, tol 1e-8), the device time of one cycle by phase from events, and
the only route the matrix had before: download the values and call scipy's `spsolve` on the host (wall clock, same machine).
`--reference-s SECONDS --reference-its N` records the time and count of the reference's `solve_hmultigrid` (c-f-h/pyiga,
unmodified, one CPU thread, another machine) beside them: a landmark, not a ratio anybody promised.

One JSON line per case on standard output; `--out PATH` also appends it to a file (profiles/hmg_timing.txt was written that
way).  A record, not a threshold.

  timeout -k 10 300 python tools/bench_hmg.py diag32 && timeout -k 10 600 python tools/bench_hmg.py diag64
"""
import json
import os
import sys
import time

import numpy as np
import scipy.sparse
import scipy.sparse.linalg

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyiga_amd import _lib, bspline, geometry, solvers  # noqa: E402
from pyiga_amd.hierarchical import HSpace  # noqa: E402

CASES = {'diag32': (32, 4), 'diag64': (64, 5), 'diag8': (8, 2)}
FORM = 'inner(grad(u),grad(v))*dx'
TOL = 1e-8
REPS = 3


def f_rhs(x, y):
    return np.cos(x) * np.exp(y)


def build(n0, L):
    kv = bspline.make_knots(3, 0.0, 1.0, n0)
    hs = HSpace((kv, kv), truncate=False, disparity=1, bdspecs=[(a, s) for a in range(2) for s in (0, 1)])
    for lv in range(L):
        hs.refine_region(lv, lambda *X: abs(X[0] - X[-1]) < 0.5 ** (lv + 1))
    return hs


def option(name, cast):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else None


def main():
    flags = ('--out', '--reference-s', '--reference-its', '--strategy')
    skip = {sys.argv[i + 1] for i, a in enumerate(sys.argv) if a in flags}
    args = [a for a in sys.argv[1:] if not a.startswith('--') and a not in skip]
    name = args[0] if args else 'diag8'
    strategy = option('--strategy', str) or 'cell_supp'
    n0, L = CASES[name]
    hs = build(n0, L)
    geo = geometry.bspline_quarter_annulus()
    ctx = _lib.context(None)
    free = np.array(hs.non_dirichlet_dofs())
    t0 = time.perf_counter()
    S = solvers.HierarchicalSystem(hs, FORM, geo=geo, f=f_rhs)
    ctx.sync()
    t_asm = time.perf_counter() - t0
    coarse_max = max(2048, min(8192, len(hs.indices_to_smooth(strategy)[0])))
    t0 = time.perf_counter()
    S.setup(strategy=strategy, coarse_max=coarse_max)
    ctx.sync()
    t_setup = time.perf_counter() - t0
    H = S.hierarchy
    rec = {'case': name, 'numdofs': hs.numdofs, 'numactive': list(hs.numactive), 'free': int(free.size), 'strategy': strategy, 'smoother': 'gs',
           'smooth_steps': 2, 'tol': TOL, 'coarse_max': coarse_max, 'assemble_s': round(t_asm, 4), 'setup_s': round(t_setup, 4),
           'levels': [H.level_info(l) for l in range(H.numlevels)]}
    f = S.rhs()
    for method in ('iterate', 'cg'):
        times = []
        for rep in range(1 + REPS):
            t0 = time.perf_counter()
            x = S.solve(strategy=strategy, method=method, tol=TOL, coarse_max=coarse_max, maxiter=2000)
            if rep:
                times.append(time.perf_counter() - t0)
        rec[method + '_iterations'] = S.info['iterations'] if S.info['converged'] else None
        rec[method + '_ratio'] = S.info['ratio']
        rec[method + '_solve_s'] = round(float(np.median(times)), 5)
    prof = H.profile(f, reps=10)
    rec['cycle_ms'] = {k: (round(v, 4) if isinstance(v, float) else [round(t, 4) for t in v] if isinstance(v, list) else v) for k, v in prof.items()}
    # the route before: the values come down, scipy solves on the host
    top = H.numlevels - 1
    times = []
    for rep in range(REPS):
        t0 = time.perf_counter()
        A = H.level_matrix(top)
        u = scipy.sparse.linalg.spsolve(A[free][:, free].tocsc(), f[free])
        times.append(time.perf_counter() - t0)
    rec['host_spsolve_s'] = round(float(np.median(times)), 5)
    rec['nnz'] = int(A.nnz)
    rec['cg_vs_spsolve_error'] = float(np.linalg.norm(x[free] - u) / np.linalg.norm(u))
    for key, cast in (('--reference-s', float), ('--reference-its', int)):
        if option(key, cast) is not None:
            rec['reference_cpu_other_machine_one_thread_' + key.rsplit('-', 1)[1]] = option(key, cast)
    S.close()
    line = json.dumps(rec)
    print(line, flush=True)
    out = option('--out', str)
    if out:
        with open(out, 'a') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()

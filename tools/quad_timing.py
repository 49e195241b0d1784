#!/usr/bin/env python3
"""Times of the fused error-norm pass (approx.error_norms: igx_patch_error_sums_d) against what the library
could do for the same two numbers before it: igx_patch_eval_spline_d with the gradient, 1 + dim arrays down to the host, and
numpy for the exact solution, the weights and the sums.
  c0  a small smoke case (p = 2, 8^3 spans)
  c3  p = 2, 128^3 spans (56.6 M Gauss points)
  c4  p = 4, 128^3 spans (262 M Gauss points)
on the quarter-annulus cylinder with random dofs and g = sin x cos y cos z.  Without arguments every case runs as a child process
under its own time limit, one after the other, and the first failure ends the run; `--case NAME` runs one case here.  Per case
one JSON line: device ms of the generated kernel of the 1 + dim exact arrays and of the error sums (igx_last_timing), wall ms of
error_norms on a patch that is set up (weights resident, code object cached), and device / wall ms of the composition."""
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyiga_amd import approx, assemblers, bspline, geometry  # noqa: E402

CASES = {'c0': (2, 8, 120), 'c3': (2, 128, 420), 'c4': (4, 128, 900)}      # degree, spans per axis, time limit of the child (s)


def g_exact(x, y, z):
    return np.sin(x) * np.cos(y) * np.cos(z)


def g_grad(x, y, z):
    return (np.cos(x) * np.cos(y) * np.cos(z), -np.sin(x) * np.sin(y) * np.cos(z), -np.sin(x) * np.cos(y) * np.sin(z))


def run(name):
    p, n, _ = CASES[name]
    kvs = 3 * (bspline.make_knots(p, 0.0, 1.0, n),)
    geo = geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.quarter_annulus())
    c = np.random.default_rng(0).uniform(-1.0, 1.0, size=tuple(kv.numdofs for kv in kvs))
    P = assemblers.DevicePatch(kvs, geo)
    try:
        approx.error_norms(kvs, geo, c, g_exact, g_grad, patch=P)                # warm-up: weights, code object, workspaces
        srcs = approx._trace_exact(g_exact, g_grad, 3)
        d_ex, _ = P.eval_exprs_inputs(srcs, [], buf='_d_qex')
        expr_ms = P.timing()['total_ms']
        d_c = P.upload_dofs(c, buf='_d_qdofs')
        sums = P.error_sums(d_c, True, d_ex)
        t = P.timing()
        t0 = time.perf_counter()
        l2, h1 = approx.error_norms(kvs, geo, c, g_exact, g_grad, patch=P)
        wall = 1e3 * (time.perf_counter() - t0)
        assert (l2, h1) == tuple(float(np.sqrt(s)) for s in sums)
        out = {'case': name, 'p': p, 'spans': n, 'gauss_points': int(P.resident_points()), 'l2': l2, 'h1': h1,
               'fused': {'exact_arrays_ms': round(expr_ms, 3), 'error_sums_ms': round(t['total_ms'], 3), 'launches': t['n_launches'],
                         'wall_ms': round(wall, 1)}}
        # the composition: spline and gradient to the host, the rest in numpy
        t0 = time.perf_counter()
        arr = P.eval_spline(d_c, want_grad=True, to_host=True)
        spline_ms = P.timing()['total_ms']
        t1 = time.perf_counter()
        W = P.fields('mass')[0]
        X = geo.grid_eval(tuple(P.gauss(k)[0] for k in range(3)))
        xyz = tuple(X[..., k] for k in range(3))
        d = arr[0] - g_exact(*xyz)
        l2n = float(np.sqrt(np.sum(W * d * d)))
        acc = np.zeros_like(W)
        for r, gr in enumerate(g_grad(*xyz)):
            d = arr[1 + r] - gr
            acc += d * d
        h1n = float(np.sqrt(np.sum(W * acc)))
        t2 = time.perf_counter()
        out['composition'] = {'eval_spline_ms': round(spline_ms, 3), 'eval_and_download_wall_ms': round(1e3 * (t1 - t0), 1),
                              'numpy_wall_ms': round(1e3 * (t2 - t1), 1), 'wall_ms': round(1e3 * (t2 - t0), 1),
                              'l2_rel_diff': abs(l2n - l2) / l2, 'h1_rel_diff': abs(h1n - h1) / h1}
        print(json.dumps(out), flush=True)
    finally:
        P.close()


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == '--case':
        run(sys.argv[2])
    else:
        for name in (sys.argv[1:] or ['c0', 'c3', 'c4']):
            rc = subprocess.call(['timeout', '-k', '10', str(CASES[name][2]), sys.executable, os.path.abspath(__file__), '--case', name])
            if rc != 0:
                raise SystemExit('case %s ended with status %d: nothing more is started' % (name, rc))

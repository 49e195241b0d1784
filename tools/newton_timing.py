#!/usr/bin/env python3
"""Times of Newton's method on the device (pyiga_amd.solvers.NewtonSystem) for the cubic problem
-laplace(u) + u**3 = f, f = 10, zero Dirichlet data on every side, from u = 0:
  c0   2D quarter annulus, p=3 n=32 (a smoke run)
  c2   2D quarter annulus, p=3 n=256
  c4   3D quarter-annulus cylinder, p=4 n=128
Device ms (NewtonSystem.solve(timed=True)) per field evaluation (igx_patch_eval_spline_d, with the achieved rate against its
budget of 8 bytes per Gauss point and output array), per coefficient kernel of the residual and of the Jacobian, per Jacobian
assembly and per linear solve with its inner iterations, in the order they ran.  Run it under
`rocprofv3 --kernel-trace --stats -- python3 tools/newton_timing.py c4` for the per-kernel device times.  Prints one JSON line per
case."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyiga_amd import bspline, geometry, solvers  # noqa: E402

RES = '(inner(grad(w),grad(v)) + w**3*v - f*v)*dx'
JAC = '(inner(grad(u),grad(v)) + 3*w**2*u*v)*dx'


def _case(name):
    if name in ('c0', 'c2'):
        return 2 * (bspline.make_knots(3, 0.0, 1.0, 32 if name == 'c0' else 256),), geometry.quarter_annulus()
    return 3 * (bspline.make_knots(4, 0.0, 1.0, 128),), geometry.tensor_product(geometry.line_segment(0.0, 1.0),
                                                                                 geometry.quarter_annulus())


def _boundary(ndofs):
    idx = np.indices(ndofs).reshape(len(ndofs), -1)
    on = np.zeros(idx.shape[1], dtype=bool)
    for k, n in enumerate(ndofs):
        on |= (idx[k] == 0) | (idx[k] == n - 1)
    return np.flatnonzero(on)


def run(name):
    kvs, geo = _case(name)
    ndofs = tuple(kv.numdofs for kv in kvs)
    fixed = _boundary(ndofs)
    S = solvers.NewtonSystem(kvs, geo, RES, JAC, (fixed, np.zeros(fixed.size)), f=10.0)
    t0 = time.perf_counter()
    S.solve(atol=0.0, rtol=1e-8, lin_tol=1e-10, timed=True)
    wall = time.perf_counter() - t0
    npts = S.patch.resident_points()
    nout = 1 + len(kvs) if S._want_grad else 1
    phases = {}
    for ph in S.info['phases']:
        for k, v in ph.items():
            phases.setdefault(k, []).append(round(float(v), 4))
    dev = float(np.median(phases['fields_ms']))
    out = dict(case=name, ndofs=int(np.prod(ndofs)), gauss_points=int(npts), method=S.info['method'], precond=S.info['precond'],
               newton_iterations=S.info['iterations'], residual_norms=S.info['residual_norms'], wall_s=wall, field_outputs=nout,
               field_budget_bytes=8 * nout * npts, fields_ms_median=dev, fields_GBps=8e-6 * nout * npts / dev if dev > 0 else None,
               **phases)
    S.close()
    print(json.dumps(out))


if __name__ == '__main__':
    for name in (sys.argv[1:] or ['c2', 'c4']):
        run(name)

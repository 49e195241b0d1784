#!/usr/bin/env python3
"""Times of the adaptive loop (`pyiga_amd.solvers.adaptive_solve`) and of its residual kernel.

  loop32  base 32 x 32 spans, 4 rounds        the spaces of section 36's table as a starting point: 2D p = 3, HB-splines with
  loop64  base 64 x 64 spans, 5 rounds        disparity 1 on the B-spline quarter annulus, all sides Dirichlet, f = cos(x) exp(y)
  loop8   base 8 x 8 spans, 2 rounds (smoke case)
Per round, wall clock: assembly (HierarchicalSystem), solve, estimate, mark + refine (a warm-up round on the base space comes
first and is not recorded).  On the last round's space: the device ms of the residual pass of every level (igx_last_timing, median
of 5), and for the last round's solution the composition the
library offered for the same indicators before: the level functions on the host, `HSplineFunc.grid_hessian` / `grid_jacobian` and
the geometry's `grid_jacobian` / `grid_hessian` on every level's Gauss grid, geometry terms, weights and per-cell sums in numpy.

  kern3d  p = 2, 128^3 spans on the quarter-annulus cylinder (the C3 size)      k_res12 against k_err12<DIM, true> on the same patch:
  kern2d  p = 3, 512^2 spans on the quarter annulus                             device ms from igx_last_timing, median of 5 after a warm-up

Without arguments every case runs as a child process under its own time limit, one after the other, and the first failure ends
the run; `--case NAME` runs one case here.  One JSON line per case; `--out PATH` appends it to a file.  A record, not a threshold."""
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyiga_amd import _lib, assemblers, bspline, geometry, hierarchical, solvers  # noqa: E402
from pyiga_amd.hierarchical import HSpace  # noqa: E402

LOOPS = {'loop8': (8, 2, 120), 'loop32': (32, 4, 300), 'loop64': (64, 5, 600)}
KERNELS = {'kern2d': (2, 3, 512, 240), 'kern3d': (3, 2, 128, 420)}
FORM = 'inner(grad(u),grad(v))*dx'
TOL = 1e-8


def f_rhs(x, y):
    return np.cos(x) * np.exp(y)


def _gauss(kv, q):
    x, w = np.polynomial.legendre.leggauss(q)
    a, b = kv.mesh[:-1, None], kv.mesh[1:, None]
    return (0.5 * (a + b) + 0.5 * (b - a) * x[None, :]).ravel(), (0.5 * (b - a) * w[None, :]).ravel()


def composition(hs, geo, u):
    """eta_K^2 over the active cells by the route of the parent commit (2D): everything evaluated through the public host
    interface, combined in numpy."""
    fn = hierarchical.HSplineFunc(hs, u)
    out = []
    for lv in range(hs.numlevels):
        mask = hs._cact[lv]
        if not mask.any():
            continue
        kvs = hs.knotvectors(lv)
        q = max(kv.p for kv in kvs) + 1
        rules = [_gauss(kv, q) for kv in kvs]
        grid = tuple(r[0] for r in rules)
        g = fn.grid_jacobian(grid)                                   # (.., 2): d/dx, d/dy of u^ (parametric)
        H = fn.grid_hessian(grid)                                    # (.., 3): xx, xy, yy
        J = geo.grid_jacobian(grid)                                  # (.., r, c)
        G2 = geo.grid_hessian(grid)                                  # (.., m, 3)
        X = geo.grid_eval(grid)
        det = J[..., 0, 0] * J[..., 1, 1] - J[..., 0, 1] * J[..., 1, 0]
        JI = np.empty_like(J)
        JI[..., 0, 0], JI[..., 0, 1], JI[..., 1, 0], JI[..., 1, 1] = J[..., 1, 1] / det, -J[..., 0, 1] / det, -J[..., 1, 0] / det, J[..., 0, 0] / det
        K = np.einsum('...cr,...dr->...cd', JI, JI)
        s = G2[..., 0] * K[..., 0, 0, None] + 2.0 * G2[..., 1] * K[..., 0, 1, None] + G2[..., 2] * K[..., 1, 1, None]   # s_m
        b = -np.einsum('...cm,...m->...c', JI, s)
        lap = K[..., 0, 0] * H[..., 0] + 2.0 * K[..., 0, 1] * H[..., 1] + K[..., 1, 1] * H[..., 2] + b[..., 0] * g[..., 0] + b[..., 1] * g[..., 1]
        W = rules[0][1][:, None] * rules[1][1][None, :] * abs(det)
        r = f_rhs(X[..., 0], X[..., 1]) + lap
        n = [kv.numspans for kv in kvs]
        cell = lambda t: t.reshape(n[0], q, n[1], q).sum(axis=(1, 3))
        out.append((cell(W) * cell(W * r * r))[mask])               # dim = 2: h_K^2 = |K|
    return np.concatenate(out)


def run_loop(name):
    n0, rounds, _ = LOOPS[name]
    kv = bspline.make_knots(3, 0.0, 1.0, n0)
    hs = HSpace((kv, kv), truncate=False, disparity=1, bdspecs=[(a, s) for a in range(2) for s in (0, 1)])
    geo = geometry.bspline_quarter_annulus()
    ctx = _lib.context(None)
    rec = {'case': name, 'base': n0, 'rounds': []}
    for rnd in range(rounds + 1):                                    # round 0 is the warm-up (code objects, allocator) on the base space
        work = hs.copy() if rnd == 0 else hs
        t0 = time.perf_counter()
        coarse_max = max(2048, min(8192, (n0 + 3) ** 2))
        S = solvers.HierarchicalSystem(work, FORM, None, geo=geo, f=f_rhs)
        ctx.sync()
        t1 = time.perf_counter()
        u = S.solve(tol=TOL, coarse_max=coarse_max)
        ctx.sync()
        t2 = time.perf_counter()
        eta, eta2 = S.estimate(u)
        t3 = time.perf_counter()
        its = S.info['iterations']
        S.close()
        t4 = time.perf_counter()
        marked = hierarchical.mark(work, eta2, 0.5)
        if rnd:
            rec['rounds'].append({'dofs': work.numdofs, 'cells': [int(m.sum()) for m in work._cact], 'eta': eta, 'iterations': its,
                                  'assemble_s': round(t1 - t0, 4), 'solve_s': round(t2 - t1, 4), 'estimate_s': round(t3 - t2, 4)})
        if rnd and rnd < rounds:
            work.refine(marked, truncate=work.truncate)
            rec['rounds'][-1]['mark_refine_s'] = round(time.perf_counter() - t4, 4)
    # the residual kernels of the last space, device ms per level
    lvl = []
    u_hb = u                                                         # (HB space: the canonical coefficients are HB coefficients)
    for lv in range(hs.numlevels):
        if not hs._cact[lv].any():
            continue
        P = assemblers.DevicePatch(hs.knotvectors(lv), geo)
        try:
            c = (hs.level_restriction(lv) @ u_hb).reshape(hs.mesh(lv).numdofs)
            d_c = P.upload_dofs(c)
            P.residual_sums(d_c, None, elementwise=True)
            ms = []
            for _ in range(5):
                P.residual_sums(d_c, None, elementwise=True)
                ms.append(P.timing()['total_ms'])
            lvl.append(round(float(np.median(ms)), 4))
        finally:
            P.close()
    rec['residual_kernels_ms_per_level'] = lvl
    t0 = time.perf_counter()
    e2 = composition(hs, geo, u)
    rec['composition_s'] = round(time.perf_counter() - t0, 4)
    S = solvers.HierarchicalSystem(hs, FORM, None, geo=geo, f=f_rhs)
    try:
        S.estimate(u)
        t0 = time.perf_counter()
        eta, eta2 = S.estimate(u)
        rec['estimate_s'] = round(time.perf_counter() - t0, 4)
    finally:
        S.close()
    rec['composition_over_estimate'] = round(rec['composition_s'] / rec['estimate_s'], 2)
    rec['eta2_rel_diff'] = float(abs(e2 - eta2).sum() / eta2.sum())
    return rec


def run_kernel(name):
    dim, p, n, _ = KERNELS[name]
    kvs = dim * (bspline.make_knots(p, 0.0, 1.0, n),)
    geo = geometry.quarter_annulus() if dim == 2 else geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.quarter_annulus())
    c = np.random.default_rng(0).uniform(-1.0, 1.0, size=tuple(kv.numdofs for kv in kvs))
    P = assemblers.DevicePatch(kvs, geo)
    try:
        d_c = P.upload_dofs(c, buf='_d_qdofs')
        t = {}
        for key, call in (('res12', lambda: P.residual_sums(d_c, None, elementwise=True)), ('err12_grad', lambda: P.error_sums(d_c, True, None, elementwise=True))):
            call()
            ms = []
            for _ in range(5):
                call()
                ms.append(P.timing()['total_ms'])
            t[key + '_ms'] = round(float(np.median(ms)), 4)
            t[key + '_spread_ms'] = [round(min(ms), 4), round(max(ms), 4)]
        t.update(case=name, dim=dim, p=p, spans=n, gauss_points=int(P.resident_points()), res12_over_err12=round(t['res12_ms'] / t['err12_grad_ms'], 3))
        return t
    finally:
        P.close()


if __name__ == '__main__':
    argv = sys.argv[1:]
    out = argv[argv.index('--out') + 1] if '--out' in argv else None
    if '--case' in argv:
        name = argv[argv.index('--case') + 1]
        line = json.dumps(run_loop(name) if name in LOOPS else run_kernel(name))
        print(line, flush=True)
        if out:
            with open(out, 'a') as fh:
                fh.write(line + '\n')
    else:
        names = [a for a in argv if a in LOOPS or a in KERNELS] or ['loop32', 'loop64', 'kern2d', 'kern3d']
        for name in names:
            limit = (LOOPS.get(name) or KERNELS[name])[-1]
            cmd = ['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--case', name] + (['--out', out] if out else [])
            rc = subprocess.call(cmd)
            if rc != 0:
                raise SystemExit('case %s ended with status %d: nothing more is started' % (name, rc))

#!/usr/bin/env python3
"""Times of the block product of the device eigen-solver (pyiga_amd.solvers.EigenSystem) against the
single-vector SpMV it replaces, and the per-phase split of one full solve:
  c3d  3D quarter-annulus cylinder, p=3 n=48: 132 651 dofs, 45.5 M values per matrix (364 MB each: K and M together do not fit
       the 256 MB last-level cache, so the products stream HBM)
  c0   a small smoke case
For m = 4, 8, 16 the new path is ONE igx_solver_eig_products_d call (the masked copy of X + k_spmm2 over both matrices), the
baseline 2 m calls of igx_solver_spmv_d (the masked copy of x + k_spmv), m on a stiffness and m on a mass PatchSystem of the same
patch.  Every call is timed on the device by a pair of events on the library's stream (warm-up, then REPS repetitions, the median);
the baseline is m times the sum of the two medians.  The achieved rate of the value stream is 2 nnz 8 bytes over the time of the
block product.  Then EigenSystem.solve(k=6, timed=True) at the same size: iterations and the device ms per phase.  Prints one
JSON line per measurement.
  mp   the multipatch eigen-solver (solvers.MultipatchEigenSystem) on two unit cubes joined on a face,
       p=3 n=40: 157 165 dofs, about 45 M values per matrix over the general CSR pattern (values and indices pass the last-level
       cache).  One igx_solver_eig_products_d call (the masked copy of X + k_csr_spmm2 over both matrices) against 2 m calls of
       igx_solver_spmv_d on the same solver (the masked copy of x + k_csr_spmv over the same pattern; the mass product runs the
       same kernel over the same pattern, so it is counted at the time of the stiffness product), then one solve with 'mg' and
       one with 'jacobi': iterations, restarts, device ms per phase and wall time.
  mp0  the same on a small domain (a smoke case)
  vec3d  the vector-valued eigen-solver (solvers.VectorEigenSystem): linear elasticity (mu = 1, lam = 2),
       three components, on the quarter-annulus cylinder, p=2 n=50: 52^3 scalar dofs, nine blocks and the mass matrix, clamped
       on the lower side of axis 0.  One igx_solver_eig_products_d call (the masked copy of X + k_block_spmm2 over the nine
       blocks and M; `one_matrix_ms`: over the blocks alone) against m calls of igx_solver_spmv_d on a VectorFormSystem of the
       same patch (the masked copy of x + k_block_spmv: the only product of blocked vectors there was, K alone).  The rate of the
       value stream counts (blocks + nc) nnz 8 bytes per block product.  Then one solve, k=6.  The lines also go to
       profiles/veceig_timing.txt (`--out PATH`: elsewhere)
  vec0   the same on a small patch (a smoke case; printed only)"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyiga_amd import _lib, bspline, geometry, solvers  # noqa: E402
from pyiga_amd.operators import DeviceArray  # noqa: E402

REPS, WARMUP = 30, 5


def _case(name):
    if name == 'c3d':
        p, n = 3, 48
    elif name == 'c0':
        p, n = 2, 8
    else:
        raise SystemExit('unknown case %r' % name)
    kvs = 3 * (bspline.make_knots(p, 0.0, 1.0, n),)
    return kvs, geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.quarter_annulus())


def _boundary(ndofs):
    idx = np.arange(int(np.prod(ndofs))).reshape(ndofs)
    on = np.zeros(ndofs, dtype=bool)
    for k, n in enumerate(ndofs):
        for e in (0, n - 1):
            s = [slice(None)] * len(ndofs)
            s[k] = e
            on[tuple(s)] = True
    return np.sort(idx[on])


class DeviceTimer:
    """Device time of a call by two events on the library's stream (the HIP runtime the library itself uses)."""

    def __init__(self, ctx):
        self.hip = C.CDLL('libamdhip64.so')
        self.stream = C.c_void_p(_lib.load().igx_stream(ctx.handle))
        self.ev = [C.c_void_p(), C.c_void_p()]
        for e in self.ev:
            assert self.hip.hipEventCreate(C.byref(e)) == 0

    def ms(self, call):
        assert self.hip.hipEventRecord(self.ev[0], self.stream) == 0
        call()
        assert self.hip.hipEventRecord(self.ev[1], self.stream) == 0
        assert self.hip.hipEventSynchronize(self.ev[1]) == 0
        t = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(t), self.ev[0], self.ev[1]) == 0
        return t.value

    def median(self, call):
        for _ in range(WARMUP):
            call()
        return float(np.median([self.ms(call) for _ in range(REPS)]))


def run(name):
    kvs, geo = _case(name)
    ndofs = tuple(kv.numdofs for kv in kvs)
    n = int(np.prod(ndofs))
    fixed = _boundary(ndofs)
    bcs = (fixed, np.zeros(fixed.size))
    lib = _lib.load()
    rng = np.random.default_rng(0)
    S = solvers.EigenSystem(kvs, geo, bcs)
    PK = solvers.PatchSystem(kvs, geo, np.zeros(n), bcs, kind='stiffness')
    PM = solvers.PatchSystem(kvs, geo, np.zeros(n), bcs, kind='mass')
    try:
        nnz = int(PK.patch.nnz)
        T = DeviceTimer(S._ctx)
        d_x, d_y = DeviceArray.from_host(S._ctx, rng.standard_normal(n)), DeviceArray(S._ctx, n)
        t_k = T.median(lambda: _lib.check(lib.igx_solver_spmv_d(PK.handle, d_x.ptr, d_y.ptr), 'igx_solver_spmv_d'))
        t_m = T.median(lambda: _lib.check(lib.igx_solver_spmv_d(PM.handle, d_x.ptr, d_y.ptr), 'igx_solver_spmv_d'))
        print(json.dumps({'case': name, 'ndofs': list(ndofs), 'nnz': nnz, 'baseline': 'igx_solver_spmv_d', 'reps': REPS,
                          'stiffness_ms': round(t_k, 4), 'mass_ms': round(t_m, 4),
                          'GBs': round(8e-6 * nnz / t_k, 1)}), flush=True)
        for m in (4, 8, 16):
            mb = solvers.eig_width(m)
            d_X = DeviceArray.from_host(S._ctx, rng.standard_normal((n, mb)))
            d_K, d_M = DeviceArray(S._ctx, n * mb), DeviceArray(S._ctx, n * mb)
            t2 = T.median(lambda: _lib.check(lib.igx_solver_eig_products_d(S.handle, mb, d_X.ptr, d_K.ptr, d_M.ptr), 'igx_solver_eig_products_d'))
            t1 = T.median(lambda: _lib.check(lib.igx_solver_eig_products_d(S.handle, mb, d_X.ptr, d_K.ptr, None), 'igx_solver_eig_products_d'))
            base = m * (t_k + t_m)
            print(json.dumps({'case': name, 'm': m, 'block_product_ms': round(t2, 4), 'single_products_ms': round(base, 4),
                              'ratio_single_over_block': round(base / t2, 2), 'one_matrix_ms': round(t1, 4),
                              'value_stream_GBs': round(16e-6 * nnz / t2, 1)}), flush=True)
        lam, _ = S.solve(k=6, tol=1e-8, timed=True)
        info = S.info
        print(json.dumps({'case': name, 'solve': 'k=6 tol=1e-8', 'block': int(info['block']), 'precond': info['precond'],
                          'iterations': int(info['iterations']), 'converged': bool(info['converged'].all()),
                          'restarts': int(info['restarts']), 'lam': [round(float(v), 9) for v in lam],
                          'phase_ms': {k: round(float(v), 3) for k, v in info.items() if k.endswith('_ms')}}), flush=True)
    finally:
        S.close()
        PK.close()
        PM.close()


def run_mp(name):
    import time
    from pyiga_amd import assemble
    p, n = (3, 40) if name == 'mp' else (2, 6)
    kvs = 3 * (bspline.make_knots(p, 0.0, 1.0, n),)
    cube = geometry.unit_cube()
    MP = assemble.Multipatch([(kvs, cube), (kvs, cube.translate((1, 0, 0)))])
    MP.join_boundaries(0, (2, 1), 1, (2, 0))
    MP.finalize()
    fixed = []
    for q in (0, 1):
        for ax in range(3):
            for sd in (0, 1):
                if (q, ax, sd) not in ((0, 2, 1), (1, 2, 0)):                 # every face but the interface
                    fixed.append(MP.patch_to_global_idx(q)[assemble.boundary_dofs(kvs, (ax, sd), ravel=True)])
    fixed = np.unique(np.concatenate(fixed))
    lib = _lib.load()
    rng = np.random.default_rng(0)
    S = solvers.MultipatchEigenSystem(MP, (fixed, np.zeros(fixed.size)))
    try:
        nrows, nnz = MP.numdofs, int(MP.info()['nnz'])
        T = DeviceTimer(S._ctx)
        d_x, d_y = DeviceArray.from_host(S._ctx, rng.standard_normal(nrows)), DeviceArray(S._ctx, nrows)
        t_k = T.median(lambda: _lib.check(lib.igx_solver_spmv_d(S.handle, d_x.ptr, d_y.ptr), 'igx_solver_spmv_d'))
        print(json.dumps({'case': name, 'dofs': nrows, 'nnz': nnz, 'baseline': 'igx_solver_spmv_d (k_csr_spmv)', 'reps': REPS,
                          'spmv_ms': round(t_k, 4), 'GBs': round(12e-6 * nnz / t_k, 1)}), flush=True)
        for m in (4, 8, 16):
            mb = solvers.eig_width(m)
            d_X = DeviceArray.from_host(S._ctx, rng.standard_normal((nrows, mb)))
            d_K, d_M = DeviceArray(S._ctx, nrows * mb), DeviceArray(S._ctx, nrows * mb)
            t2 = T.median(lambda: _lib.check(lib.igx_solver_eig_products_d(S.handle, mb, d_X.ptr, d_K.ptr, d_M.ptr), 'igx_solver_eig_products_d'))
            t1 = T.median(lambda: _lib.check(lib.igx_solver_eig_products_d(S.handle, mb, d_X.ptr, d_K.ptr, None), 'igx_solver_eig_products_d'))
            base = 2 * m * t_k
            print(json.dumps({'case': name, 'm': m, 'block_product_ms': round(t2, 4), 'single_products_ms': round(base, 4),
                              'ratio_single_over_block': round(base / t2, 2), 'one_matrix_ms': round(t1, 4),
                              'stream_GBs': round(20e-6 * nnz / t2, 1)}), flush=True)
        for precond in ('mg', 'jacobi'):
            t0 = time.perf_counter()
            if precond == 'mg':
                S.set_multigrid()
            t1 = time.perf_counter()
            lam, _ = S.solve(k=6, tol=1e-8, precond=precond, maxiter=1000, timed=True)
            t2 = time.perf_counter()
            info = S.info
            print(json.dumps({'case': name, 'solve': 'k=6 tol=1e-8', 'block': int(info['block']), 'precond': info['precond'],
                              'levels': info.get('levels'), 'iterations': int(info['iterations']),
                              'converged': bool(info['converged'].all()), 'restarts': int(info['restarts']),
                              'lam': [round(float(v), 9) for v in lam], 'setup_s': round(t1 - t0, 3), 'wall_s': round(t2 - t1, 3),
                              'phase_ms': {k: round(float(v), 3) for k, v in info.items() if k.endswith('_ms')}}), flush=True)
    finally:
        S.close()
        MP.close()


ELASTICITY = '(2*mu*inner(0.5*(grad(u)+grad(u).T), 0.5*(grad(v)+grad(v).T)) + lam*div(u)*div(v)) * dx'


def run_vec(name, out=None):
    """The vector-valued eigen-solver: every line is printed and, for `vec3d`, written to `out` (default
    profiles/veceig_timing.txt)."""
    p, n = (2, 50) if name == 'vec3d' else (2, 6)        # (make_knots has the reference's extra sliver span at n = 49)
    nc = 3
    kvs = 3 * (bspline.make_knots(p, 0.0, 1.0, n),)
    geo = geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.quarter_annulus())
    ndofs = tuple(kv.numdofs for kv in kvs)
    N = int(np.prod(ndofs))
    nrows = nc * N
    side = np.arange(N).reshape(ndofs)[0].ravel()                       # the lower side of axis 0, every component: a cantilever
    fixed = np.concatenate([side + c * N for c in range(nc)])
    bcs = (fixed, np.zeros(fixed.size))
    lib = _lib.load()
    rng = np.random.default_rng(0)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    bf = [('u', nc), ('v', nc)]
    S = solvers.VectorEigenSystem(ELASTICITY, kvs, bcs, bfuns=bf, geo=geo, mu=1.0, lam=2.0)
    P = solvers.VectorFormSystem(ELASTICITY, kvs, 0.0, bcs, bfuns=bf, geo=geo, mu=1.0, lam=2.0)
    try:
        nnz = int(S.patch.nnz)
        nblk = sum(sum(r) for r in S.present)
        T = DeviceTimer(S._ctx)
        d_x, d_y = DeviceArray.from_host(S._ctx, rng.standard_normal(nrows)), DeviceArray(S._ctx, nrows)
        t_k = T.median(lambda: _lib.check(lib.igx_solver_spmv_d(P.handle, d_x.ptr, d_y.ptr), 'igx_solver_spmv_d'))
        emit({'case': name, 'ndofs': list(ndofs), 'ncomp': nc, 'nnz': nnz, 'blocks': nblk, 'baseline': 'igx_solver_spmv_d (k_block_spmv)',
              'reps': REPS, 'stiffness_ms': round(t_k, 4), 'GBs': round(8e-6 * nblk * nnz / t_k, 1)})
        for m in (4, 8, 16):
            mb = solvers.eig_width(m)
            d_X = DeviceArray.from_host(S._ctx, rng.standard_normal((nrows, mb)))
            d_K, d_M = DeviceArray(S._ctx, nrows * mb), DeviceArray(S._ctx, nrows * mb)
            t2 = T.median(lambda: _lib.check(lib.igx_solver_eig_products_d(S.handle, mb, d_X.ptr, d_K.ptr, d_M.ptr), 'igx_solver_eig_products_d'))
            t1 = T.median(lambda: _lib.check(lib.igx_solver_eig_products_d(S.handle, mb, d_X.ptr, d_K.ptr, None), 'igx_solver_eig_products_d'))
            base = m * t_k                                               # (the parent's path has no mass product of blocked vectors: K alone)
            emit({'case': name, 'm': m, 'block_product_ms': round(t2, 4), 'one_matrix_ms': round(t1, 4), 'single_products_ms': round(base, 4),
                  'ratio_single_over_block': round(base / t2, 2), 'ratio_single_over_one_matrix': round(base / t1, 2),
                  'value_stream_GBs': round(8e-6 * (nblk + nc) * nnz / t2, 1), 'one_matrix_value_stream_GBs': round(8e-6 * nblk * nnz / t1, 1)})
        lam, _ = S.solve(k=6, tol=1e-8, maxiter=1000, timed=True)
        info = S.info
        emit({'case': name, 'solve': 'k=6 tol=1e-8 maxiter=1000', 'block': int(info['block']), 'precond': info['precond'],
              'iterations': int(info['iterations']), 'converged': bool(info['converged'].all()), 'restarts': int(info['restarts']),
              'lam': [round(float(v), 9) for v in lam], 'phase_ms': {k: round(float(v), 3) for k, v in info.items() if k.endswith('_ms')}})
    finally:
        S.close()
        P.close()
    if name == 'vec3d':
        path = out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'veceig_timing.txt')
        with open(path, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    args = sys.argv[1:]
    out = None
    if '--out' in args:
        i = args.index('--out')
        out = args[i + 1]
        del args[i:i + 2]
    for c in (args or ['c3d']):
        if c in ('vec3d', 'vec0'):
            run_vec(c, out)
        else:
            (run_mp if c in ('mp', 'mp0') else run)(c)

#!/usr/bin/env python3
"""Device time of the saddle-point solver (`solvers.SaddlePointSystem`, csrc/solve_saddle.hip) on the
enclosed Stokes problem (velocity 0 on the whole boundary, right-hand side 1 in every velocity entry) over a Taylor-Hood pair,
velocity p = 3 with interior knots of multiplicity 2 against pressure p = 2:
  nb2d  the quarter annulus at the size of the reference's solve-stokes notebook, 50 x 25 spans
  th3d  the quarter-annulus cylinder, n = 32 spans per axis (the 3D size of tools/pair_timing.py)
  th0   a small smoke case (printed only)
Every figure is a median of REPS runs after WARMUP ones, from device events of the library:
  assembly   one block of A (`igx_assemble` IGX_FORM, `igx_last_timing` total_ms) and one block of B (`igx_pair_assemble`,
             `igx_pair_last_timing` total_ms); a system has nc blocks of each
  transpose  `k_pair_transpose` of one block (`igx_solver_take_pair_block` on a solver made for it, `igx_solver_saddle_timing`)
  product    one product with the velocity-row and the pressure-row launch timed apart (`igx_solver_saddle_product_d`), each with
             its bytes (8 per stored value it streams: A and B^T; B) over its time
  solve      `solve(tol=1e-8, timed=True)`: iterations, the whole solve, and per iteration the preconditioner and the vector
             kernels (the solver's events)
nb2d also takes the host wall clock of scipy's spsolve of the same system (one run); the sparse LU of the 3D system is not run
(fill-in).  One JSON line per case, appended to profiles/saddle_timing.txt (`--out PATH`: elsewhere).  A record, not a threshold.

One case per process, each under its own time limit, the steps chained so that a failure ends the run:
  timeout -k 10 300 python tools/saddle_timing.py nb2d && timeout -k 10 900 python tools/saddle_timing.py th3d
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyiga_amd import _lib, assemble, bspline, geometry, solvers  # noqa: E402
from pyiga_amd.form_assemblers import _full_table  # noqa: E402
from pyiga_amd.operators import DeviceArray  # noqa: E402

REPS, WARMUP = 7, 2
CASES = {'nb2d': (2, (50, 25)), 'th3d': (3, (32, 32, 32)), 'th0': (2, (6, 4))}


def median_of(run):
    """Median of REPS values of run() after WARMUP calls."""
    vals = [run() for _ in range(WARMUP + REPS)][WARMUP:]
    return float(np.median(vals))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'saddle_timing.txt')
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
    S = solvers.SaddlePointSystem((ku, kp), geo, bcs, rhs=1.0)
    lib = _lib.load()
    nblocks_a = sum(1 for row in S.present for p in row if p)
    nnz_a, nnz_b = nblocks_a * S.patch.nnz, dim * S.pair.nnz

    # the solve first: the assembly and transpose runs below reuse the system's patch and pair
    runs = []
    for k in range(WARMUP + REPS):
        S.solve(tol=1e-8, maxiter=5000, timed=True)
        if k >= WARMUP:
            runs.append(dict(S.info))
    med = lambda key: float(np.median([r[key] for r in runs]))
    its = runs[0]['iterations']

    # one product, its two launches apart
    ctx = S.patch.ctx
    rng = np.random.default_rng(0)
    d_x, d_y = DeviceArray.from_host(ctx, rng.standard_normal(S.n)), DeviceArray(ctx, S.n)
    tu, tp = C.c_float(), C.c_float()
    prod = []
    for k in range(WARMUP + REPS):
        _lib.check(lib.igx_solver_saddle_product_d(S.handle, d_x.ptr, None, 1.0, None, d_y.ptr, None), 'igx_solver_saddle_product_d')
        _lib.check(lib.igx_solver_saddle_timing(S.handle, None, C.byref(tu), C.byref(tp)), 'igx_solver_saddle_timing')
        if k >= WARMUP:
            prod.append((tu.value, tp.value))
    u_ms, p_ms = float(np.median([a for a, _ in prod])), float(np.median([b for _, b in prod]))
    bytes_u, bytes_p = 8.0 * (nnz_a + nnz_b), 8.0 * nnz_b

    # assembly of one block of A and of one block of B
    def assemble_a():
        S.patch.set_form(_full_table(S.asm_a._table[0][0], dim))
        S.patch.assemble('form', to_host=False)
        return S.patch.timing()['total_ms']

    def assemble_b():
        S.patch.set_form(_full_table(S.asm_b._table[0][0], dim))
        S.pair.assemble('form', to_host=False)
        return S.pair.timing()['total_ms']
    a_ms = median_of(assemble_a)
    b_ms = median_of(assemble_b)

    # the transpose of one block: a solver made for it takes the values the pair holds
    def transpose():
        S.pair.assemble('form', to_host=False)
        h = C.c_void_p()
        _lib.check(lib.igx_solver_create_saddle(S.patch.handle, S.pair.handle, dim, None, 0, C.byref(h)), 'igx_solver_create_saddle')
        try:
            _lib.check(lib.igx_solver_take_pair_block(h, S.pair.handle, 0), 'igx_solver_take_pair_block')
            t = C.c_float()
            _lib.check(lib.igx_solver_saddle_timing(h, C.byref(t), None, None), 'igx_solver_saddle_timing')
        finally:
            lib.igx_solver_destroy(h)
        return t.value
    t_ms = median_of(transpose)

    rec = {'case': name, 'spans': list(n_el), 'unknowns': S.n, 'velocity_dofs': S.ncomp * S.N, 'pressure_dofs': S.Np,
           'blocks_A': nblocks_a, 'values_A': int(nnz_a), 'blocks_B': dim, 'values_B': int(nnz_b),
           'assemble_A_block_ms': round(a_ms, 4), 'assemble_B_block_ms': round(b_ms, 4), 'transpose_block_ms': round(t_ms, 4),
           'product_u_rows_ms': round(u_ms, 5), 'product_u_rows_GBps': round(bytes_u / (u_ms * 1e-3) / 1e9, 1),
           'product_p_rows_ms': round(p_ms, 5), 'product_p_rows_GBps': round(bytes_p / (p_ms * 1e-3) / 1e9, 1),
           'iterations': its, 'converged': bool(runs[0]['converged']), 'relres': runs[0]['relres'], 'precond': runs[0]['precond'],
           'solve_ms': round(med('total_ms'), 3), 'precond_ms_per_iteration': round(med('precond_ms') / its, 5),
           'vector_ms_per_iteration': round(med('vector_ms') / its, 5), 'reps': REPS, 'warmup': WARMUP}
    if name != 'th3d':
        import scipy.sparse
        import scipy.sparse.linalg
        A = assemble.assemble('inner(grad(u), grad(v)) * dx', ku, bfuns=[('u', dim), ('v', dim)], geo=geo)
        B = assemble.assemble('div(u) * p * dx', (ku, kp), bfuns=[('u', dim, 0), ('p', 1, 1)], geo=geo)
        K = scipy.sparse.bmat([[A, B.T], [B, None]], format='csr')
        pin = (np.append(bcs[0], dim * S.N), np.append(bcs[1], 0.0))
        LS = assemble.RestrictedLinearSystem(K, S.b, pin)
        t0 = time.perf_counter()
        scipy.sparse.linalg.spsolve(LS.A, LS.b)
        rec['host_spsolve_s'] = round(time.perf_counter() - t0, 3)
    print(json.dumps(rec), flush=True)
    S.close()
    if name != 'th0':
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, 'a') as f:
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()

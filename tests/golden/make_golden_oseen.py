#!/usr/bin/env python3
"""Golden vectors for the device Oseen solver (GMRES on saddle-point systems), from the REAL reference (c-f-h/pyiga).

Run where an unmodified build of the reference is importable (see the header of make_golden.py):

    PYTHONPATH=/path/to/built/reference python3 tests/golden/make_golden_oseen.py

Writes tests/golden/golden_oseen.npz -- data only.  Two cases, built as the reference's solve-navier-stokes notebook builds each
of its linear systems, with the wind given as data:

    oseen2   spaces, geometry and bcs of the `stokes` case of make_golden_pair.py (the solve-stokes notebook at n_el = (6, 4),
             328 unknowns, the first pressure dof pinned), wind w(x, y) = (-y, x)
    oseen3   those of the `stokes3` case of make_golden_saddle.py (561 unknowns), wind w(x, y, z) = (-y, x, 0.25)

assemble.assemble for A_grad, A_div and A_conv = assemble('grad(u).dot(w).dot(v) * dx', kvs_u, bfuns=[('u', nc), ('v', nc)],
geo=geo, w=wind); bmat([[nu A_grad + A_conv, A_div.T], [A_div, None]]); RestrictedLinearSystem; spsolve.  Per case: the knot
vectors, the three matrices, the bcs, nu, u and `<case>_amp`, measured as `stokes3_amp` is (the stored values of the three
matrices times 1 + 1e-13 N(0, 1), seeded, solved again; the largest relative change of u over five seeds, divided by 1e-13).

nu starts at 0.1 and is doubled until the host model of the device solver (tests/_gmres_model.py) with the block-diagonal
Kronecker preconditioner, unrestarted, converges to tol = 1e-10 in at most 200 steps -- a condition on the case, not a
measurement; nu and that count (`<case>_model_steps`) are written with the case.
"""
import os
import sys

import numpy as np
import scipy.sparse
import scipy.sparse.linalg

import pyiga
from pyiga import assemble, bspline, geometry

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import _gmres_model as gm       # noqa: E402

pyiga.set_max_threads(1)
OUT = os.path.dirname(os.path.abspath(__file__))
mk = bspline.make_knots
MAX_STEPS = 200


def put_csr(out, name, A):
    A = scipy.sparse.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    assert A.has_canonical_format
    out[name + '_data'], out[name + '_indices'], out[name + '_indptr'] = A.data, A.indices, A.indptr
    out[name + '_shape'] = np.array(A.shape)


def model_steps(A, B, nc, bcs, kvs_u, kvs_p, nu):
    """Steps of the unrestarted model with the block-diagonal Kronecker preconditioner at tol 1e-10 (MAX_STEPS + 1: none)."""
    n = A.shape[0] + B.shape[0]
    free = np.ones(n, dtype=bool)
    free[bcs[0]] = False
    mats_u = [(assemble.bsp_stiffness_1d(kv), assemble.bsp_mass_1d(kv)) for kv in kvs_u]
    mats_p = [(None, assemble.bsp_mass_1d(kv)) for kv in kvs_p]
    P = gm.block_preconditioner(tuple(kv.numdofs for kv in kvs_u), tuple(kv.numdofs for kv in kvs_p), nc, free, mats_u, mats_p,
                                scale=nu, viscosity=nu)
    _, info = gm.solve(A, B, nc, bcs, P=P, tol=1e-10, maxiter=MAX_STEPS, restart=MAX_STEPS)
    return info['iterations'] if info['converged'] else MAX_STEPS + 1


def case(out, name, geo, kvs_u, kvs_p, sides, wind):
    nc = len(kvs_u)
    for s, kvs in enumerate((kvs_u, kvs_p)):
        for k, kv in enumerate(kvs):
            out['%s_kv%d_%d' % (name, s, k)] = kv.kv
            out['%s_p%d_%d' % (name, s, k)] = np.array(kv.p)
    bf = [('u', nc), ('v', nc)]
    A_grad = scipy.sparse.csr_matrix(assemble.assemble('inner(grad(u), grad(v)) * dx', kvs_u, bfuns=bf, geo=geo))
    A_div = scipy.sparse.csr_matrix(assemble.assemble('div(u) * p * dx', (kvs_u, kvs_p), bfuns=[('u', nc, 0), ('p', 1, 1)], geo=geo))
    A_conv = scipy.sparse.csr_matrix(assemble.assemble('grad(u).dot(w).dot(v) * dx', kvs_u, bfuns=bf, geo=geo, w=wind))
    bcs = assemble.compute_dirichlet_bcs(kvs_u, geo, sides)
    N = int(np.prod(tuple(kv.numdofs for kv in kvs_u)))
    bcs = (np.append(bcs[0], nc * N), np.append(bcs[1], 0.0))
    nu = 0.1
    while True:
        steps = model_steps(nu * A_grad + A_conv, A_div, nc, bcs, kvs_u, kvs_p, nu)
        print('%s: nu = %g: the model takes %s steps' % (name, nu, steps if steps <= MAX_STEPS else 'more than %d' % MAX_STEPS))
        if steps <= MAX_STEPS:
            break
        nu *= 2.0
    assert steps <= MAX_STEPS

    def solve(Ag, Ac, Ad):
        A = scipy.sparse.bmat([[nu * Ag + Ac, Ad.T], [Ad, None]], format='csr')
        LS = assemble.RestrictedLinearSystem(A, 0.0, bcs)
        return LS.complete(scipy.sparse.linalg.spsolve(LS.A, LS.b))
    u = solve(A_grad, A_conv, A_div)
    put_csr(out, name + '_A_grad', A_grad)
    put_csr(out, name + '_A_div', A_div)
    put_csr(out, name + '_A_conv', A_conv)
    out[name + '_bcs_idx'], out[name + '_bcs_val'] = np.asarray(bcs[0]), np.asarray(bcs[1])
    out[name + '_nu'], out[name + '_model_steps'] = np.array(nu), np.array(steps)
    out[name + '_u'] = u
    amp = 0.0
    for seed in range(5):
        r = np.random.default_rng(seed)
        pert = []
        for M in (A_grad, A_conv, A_div):
            M = M.copy()
            M.data = M.data * (1 + 1e-13 * r.standard_normal(M.data.shape))
            pert.append(M)
        a = abs(solve(*pert) - u).max() / abs(u).max() / 1e-13
        print('%s_amp, seed %d: %.2f' % (name, seed, a))
        amp = max(amp, a)
    print('%s: %d unknowns, nu = %g, amp = %.2f' % (name, u.size, nu, amp))
    out[name + '_amp'] = np.array(amp)


def main():
    out = {}

    def lid2(x, y):
        return (x * y * -y, x * y * x)

    def zero2(x, y):
        return (0.0, 0.0)

    def wind2(x, y):
        return (-y, x)
    case(out, 'oseen2', geometry.quarter_annulus(), tuple(mk(3, 0.0, 1.0, n, mult=2) for n in (6, 4)),
         tuple(mk(2, 0.0, 1.0, n, mult=1) for n in (6, 4)),
         [('bottom', zero2), ('top', zero2), ('left', lid2), ('right', zero2)], wind2)
    assert out['oseen2_u'].shape == (328,)

    def lid3(x, y, z):
        return (x * y * -y, x * y * x, 0.0 * z)

    def zero3(x, y, z):
        return (0.0, 0.0, 0.0)

    def wind3(x, y, z):
        return (-y, x, 0.25 + 0.0 * z)
    case(out, 'oseen3', geometry.twisted_box(), (mk(2, 0., 1., 2, mult=2), mk(2, 0., 1., 3, mult=2), mk(2, 0., 1., 2, mult=2)),
         (mk(1, 0., 1., 2), mk(1, 0., 1., 3), mk(1, 0., 1., 2)),
         [('bottom', zero3), ('top', zero3), ('left', lid3), ('right', zero3), ('front', zero3), ('back', zero3)], wind3)
    assert out['oseen3_u'].shape == (3 * 175 + 36,)
    path = os.path.join(OUT, 'golden_oseen.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Golden vectors for the device saddle-point solver, from the REAL reference (c-f-h/pyiga).

Run where an unmodified build of the reference is importable (see the header of make_golden.py):

    PYTHONPATH=/path/to/built/reference python3 tests/golden/make_golden_saddle.py

Writes tests/golden/golden_saddle.npz -- data only: the 3D lid-driven cavity on the spaces and the geometry of case `th3` of
make_golden_pair.py (Taylor-Hood p = 2 / 1 on the twisted box, 3 x 175 velocity and 36 pressure dofs), built as the reference's
solve-stokes notebook builds its 2D system: assemble.assemble for both forms, compute_dirichlet_bcs on all six sides (`left`
carries the lid velocity), the first pressure dof pinned, scipy.sparse.bmat, RestrictedLinearSystem, spsolve.  It holds the
knot vectors, both matrices, the bcs, the solution and `stokes3_amp`, measured exactly as `stokes_amp` of golden_pair.npz: the
stored values of both matrices are multiplied by 1 + 1e-13 N(0, 1) (seeded), the system is solved again, and the largest
relative change of u over five seeds is divided by 1e-13.
"""
import os

import numpy as np
import scipy.sparse
import scipy.sparse.linalg

import pyiga
from pyiga import assemble, bspline, geometry

pyiga.set_max_threads(1)
OUT = os.path.dirname(os.path.abspath(__file__))
mk = bspline.make_knots


def put_csr(out, name, A):
    A = scipy.sparse.csr_matrix(A)
    assert A.has_canonical_format
    out[name + '_data'], out[name + '_indices'], out[name + '_indptr'] = A.data, A.indices, A.indptr
    out[name + '_shape'] = np.array(A.shape)


def main():
    out = {}
    geo = geometry.twisted_box()
    kvs_u = (mk(2, 0., 1., 2, mult=2), mk(2, 0., 1., 3, mult=2), mk(2, 0., 1., 2, mult=2))
    kvs_p = (mk(1, 0., 1., 2), mk(1, 0., 1., 3), mk(1, 0., 1., 2))
    for s, kvs in enumerate((kvs_u, kvs_p)):
        for k, kv in enumerate(kvs):
            out['stokes3_kv%d_%d' % (s, k)] = kv.kv
            out['stokes3_p%d_%d' % (s, k)] = np.array(kv.p)
    A_grad = assemble.assemble('inner(grad(u), grad(v)) * dx', kvs_u, bfuns=[('u', 3), ('v', 3)], geo=geo)
    A_div = assemble.assemble('div(u) * p * dx', (kvs_u, kvs_p), bfuns=[('u', 3, 0), ('p', 1, 1)], geo=geo)

    def g_lid(x, y, z):
        return (x * y * -y, x * y * x, 0.0 * z)

    def g_zero(x, y, z):
        return (0.0, 0.0, 0.0)
    bcs = assemble.compute_dirichlet_bcs(kvs_u, geo, [('bottom', g_zero), ('top', g_zero), ('left', g_lid), ('right', g_zero),
                                                      ('front', g_zero), ('back', g_zero)])
    N = np.prod(tuple(kv.numdofs for kv in kvs_u))
    bcs = (np.append(bcs[0], 3 * N), np.append(bcs[1], 0.0))

    def solve(Ag, Ad):
        A = scipy.sparse.bmat([[Ag, Ad.T], [Ad, None]], format='csr')
        LS = assemble.RestrictedLinearSystem(A, 0.0, bcs)
        return LS.complete(scipy.sparse.linalg.spsolve(LS.A, LS.b))
    A_grad, A_div = scipy.sparse.csr_matrix(A_grad), scipy.sparse.csr_matrix(A_div)
    u = solve(A_grad, A_div)
    assert u.shape == (3 * 175 + 36,)
    put_csr(out, 'stokes3_A_grad', A_grad)
    put_csr(out, 'stokes3_A_div', A_div)
    out['stokes3_bcs_idx'], out['stokes3_bcs_val'] = np.asarray(bcs[0]), np.asarray(bcs[1])
    out['stokes3_u'] = u
    amp = 0.0
    for seed in range(5):
        r = np.random.default_rng(seed)
        Ag, Ad = A_grad.copy(), A_div.copy()
        Ag.data = Ag.data * (1 + 1e-13 * r.standard_normal(Ag.data.shape))
        Ad.data = Ad.data * (1 + 1e-13 * r.standard_normal(Ad.data.shape))
        a = abs(solve(Ag, Ad) - u).max() / abs(u).max() / 1e-13
        print('stokes3_amp, seed %d: %.2f' % (seed, a))
        amp = max(amp, a)
    print('stokes3_amp = %.2f' % amp)
    out['stokes3_amp'] = np.array(amp)
    path = os.path.join(OUT, 'golden_saddle.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()

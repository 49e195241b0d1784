#!/usr/bin/env python3
"""Golden vectors for bilinear forms over TWO spline spaces, from the REAL reference (c-f-h/pyiga).

Run where an unmodified build of the reference is importable (see the header of make_golden.py):

    PYTHONPATH=/path/to/built/reference python3 tests/golden/make_golden_pair.py

Writes tests/golden/golden_pair.npz -- data only: knot vectors, matrices, picked entries, the Stokes system of the
reference's solve-stokes notebook at n_el = (6, 4), p = 3 (328 unknowns) and `stokes_amp`.  Every array comes from the
reference's public API: assemble.assemble / instantiate_assembler with kvs = (kvs0, kvs1) and bfuns = [(name, nc, space)],
assemble.bsp_mixed_deriv_biform_1d_asym, assemble.compute_dirichlet_bcs, assemble.RestrictedLinearSystem, spsolve.

Facts about the reference this file relies on (checked on it): rows come from space 1 and columns from space 0; the Gauss rule
has max(p over BOTH spaces) + 1 points per span of the mesh of space 0; the CSR is canonical and holds the full product
pattern.

The coefficient functions of case hi2 are those of `_vec_inputs` in tests/test_gpu_parity.py (c, K; the convection vector b is
its `gv`).

stokes_amp: how strongly the Stokes solution reacts to the rounding of the assembled values -- the stored values of A_grad and
A_div are multiplied by 1 + 1e-13 N(0, 1) (seeded), the system is solved again, and the largest relative change of u over five
seeds is divided by 1e-13.  The device test accepts 10 * stokes_amp * 1e-12.
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

INPUTS = {'c': lambda x, y: 1.0 + x * y,
          'K': lambda x, y: np.stack([np.stack([1.0 + x, 0.5 * y], -1), np.stack([0 * x, 2.0 - y], -1)], -2),
          'b': lambda x, y: (y, -x)}
FULL = '(inner(dot(K,grad(u)),grad(q)) + inner(b,grad(u))*q + u*inner(b,grad(q)) + c*u*q)*dx'

# id -> (trial space, test space, geometry, [(name, form, bfuns, layouts)])
CASES = {
    'th2': ((mk(3, 0., 1., 4, mult=2), mk(3, 0., 1., 3, mult=2)), (mk(2, 0., 1., 4), mk(2, 0., 1., 3)), 'quarter_annulus',
            [('div', 'div(u) * p * dx', [('u', 2, 0), ('p', 1, 1)], ('blocked', 'packed')),
             ('mass', 'u * p * dx', [('u', 1, 0), ('p', 1, 1)], ('blocked',))]),
    'th2t': ((mk(2, 0., 1., 4), mk(2, 0., 1., 3)), (mk(3, 0., 1., 4, mult=2), mk(3, 0., 1., 3, mult=2)), 'quarter_annulus',
             [('divt', 'p * div(v) * dx', [('p', 1, 0), ('v', 2, 1)], ('blocked',))]),
    'th3': ((mk(2, 0., 1., 2, mult=2), mk(2, 0., 1., 3, mult=2), mk(2, 0., 1., 2, mult=2)), (mk(1, 0., 1., 2), mk(1, 0., 1., 3), mk(1, 0., 1., 2)),
            'twisted_box', [('div', 'div(u) * p * dx', [('u', 3, 0), ('p', 1, 1)], ('blocked', 'packed'))]),
    'q1p0': ((mk(1, 0., 1., 3), mk(1, 0., 1., 1)), (mk(0, 0., 1., 3), mk(0, 0., 1., 1)), 'quarter_annulus',
             [('div', 'div(u) * p * dx', [('u', 2, 0), ('p', 1, 1)], ('blocked', 'packed'))]),
    'hi2': ((mk(1, 0., 1., 3), mk(2, 0., 1., 2, mult=2)), (mk(4, 0., 1., 3, mult=3), mk(3, 0., 1., 2)), 'quarter_annulus',
            [('full', FULL, [('u', 1, 0), ('q', 1, 1)], ('blocked',))]),
    'lo2': ((mk(4, 0., 1., 5, mult=3), mk(3, 0., 1., 3)), (mk(1, 0., 1., 5), mk(2, 0., 1., 3, mult=2)), 'quarter_annulus',
            [('rd', '(inner(grad(u),grad(q)) + u*q)*dx', [('u', 1, 0), ('q', 1, 1)], ('blocked',))]),
}


def put_csr(out, name, A):
    A = scipy.sparse.csr_matrix(A)
    assert A.has_canonical_format
    out[name + '_data'], out[name + '_indices'], out[name + '_indptr'] = A.data, A.indices, A.indptr
    out[name + '_shape'] = np.array(A.shape)


def main():
    out = {}
    rng = np.random.default_rng(20240607)
    for cid, (kvs0, kvs1, gname, forms) in CASES.items():
        geo = getattr(geometry, gname)()
        for s, kvs in enumerate((kvs0, kvs1)):
            for k, kv in enumerate(kvs):
                out['%s_kv%d_%d' % (cid, s, k)] = kv.kv
                out['%s_p%d_%d' % (cid, s, k)] = np.array(kv.p)
        for name, form, bfuns, layouts in forms:
            args = INPUTS if form == FULL else {}
            for layout in layouts:
                A = assemble.assemble(form, (kvs0, kvs1), bfuns=bfuns, geo=geo, layout=layout, **args)
                put_csr(out, '%s_%s_%s' % (cid, name, layout), A)
                print(cid, name, layout, A.shape, A.nnz)
            # picked entries through the assembler object: pattern entries and a few pairs outside of it
            asm = assemble.instantiate_assembler(form, (kvs0, kvs1), dict(args, geo=geo), bfuns, None)
            ncu, ncv = bfuns[0][1], bfuns[1][1]
            B = scipy.sparse.csr_matrix(assemble.assemble(form, (kvs0, kvs1), bfuns=bfuns, geo=geo, layout='packed', **args))
            n1, n0 = B.shape[0] // ncv, B.shape[1] // ncu
            I = rng.integers(0, n1, 24)
            J = np.array([rng.choice(B[i * ncv:(i + 1) * ncv].indices // ncu) for i in I])
            I, J = np.concatenate((I, rng.integers(0, n1, 6))), np.concatenate((J, rng.integers(0, n0, 6)))
            idx = np.stack((I, J), axis=1).astype(np.uintp)
            out['%s_%s_idx' % (cid, name)] = idx
            if ncu == ncv == 1:                # (the reference makes a scalar assembler: entry / multi_entries, no blocks)
                out['%s_%s_entries' % (cid, name)] = np.array([asm.entry(int(i), int(j)) for i, j in idx])
            else:
                out['%s_%s_numcomp' % (cid, name)] = np.array(asm.num_components())
                out['%s_%s_blocks' % (cid, name)] = np.asarray(asm.multi_blocks(idx))

    # 1D matrices relating two bases
    kv1, kv2 = mk(3, 0., 1., 4, mult=2), mk(2, 0., 1., 4)
    out['asym_kv1'], out['asym_kv2'] = kv1.kv, kv2.kv
    for du in (0, 1):
        for dv in (0, 1):
            out['asym_%d%d' % (du, dv)] = assemble.bsp_mixed_deriv_biform_1d_asym(kv1, kv2, du, dv).toarray()
    assert np.array_equal(out['asym_00'], assemble.bsp_mass_1d_asym(kv1, kv2).toarray())
    assert np.array_equal(out['asym_11'], assemble.bsp_stiffness_1d_asym(kv1, kv2).toarray())

    # the cells of notebooks/solve-stokes.ipynb at n_el = (6, 4)
    geo = geometry.quarter_annulus()
    p, n_el = 3, (6, 4)
    kvs_u = tuple(mk(p, 0.0, 1.0, n, mult=2) for n in n_el)
    kvs_p = tuple(mk(p - 1, 0.0, 1.0, n, mult=1) for n in n_el)
    A_grad = assemble.assemble('inner(grad(u), grad(v)) * dx', kvs_u, bfuns=[('u', 2), ('v', 2)], geo=geo)
    A_div = assemble.assemble('div(u) * p * dx', (kvs_u, kvs_p), bfuns=[('u', 2, 0), ('p', 1, 1)], geo=geo)

    def g_lid(x, y):
        return (x * y * -y, x * y * x)

    def g_zero(x, y):
        return (0.0, 0.0)
    bcs = assemble.compute_dirichlet_bcs(kvs_u, geo, [('bottom', g_zero), ('top', g_zero), ('left', g_lid), ('right', g_zero)])
    N = np.prod(tuple(kv.numdofs for kv in kvs_u))
    bcs = (np.append(bcs[0], 2 * N), np.append(bcs[1], 0.0))

    def solve(Ag, Ad):
        A = scipy.sparse.bmat([[Ag, Ad.T], [Ad, None]], format='csr')
        LS = assemble.RestrictedLinearSystem(A, 0.0, bcs)
        return LS.complete(scipy.sparse.linalg.spsolve(LS.A, LS.b))
    A_grad, A_div = scipy.sparse.csr_matrix(A_grad), scipy.sparse.csr_matrix(A_div)
    u = solve(A_grad, A_div)
    assert u.shape == (328,)
    put_csr(out, 'stokes_A_grad', A_grad)
    put_csr(out, 'stokes_A_div', A_div)
    out['stokes_bcs_idx'], out['stokes_bcs_val'] = np.asarray(bcs[0]), np.asarray(bcs[1])
    out['stokes_u'] = u
    amp = 0.0
    for seed in range(5):
        r = np.random.default_rng(seed)
        Ag, Ad = A_grad.copy(), A_div.copy()
        Ag.data = Ag.data * (1 + 1e-13 * r.standard_normal(Ag.data.shape))
        Ad.data = Ad.data * (1 + 1e-13 * r.standard_normal(Ad.data.shape))
        a = abs(solve(Ag, Ad) - u).max() / abs(u).max() / 1e-13
        print('stokes_amp, seed %d: %.2f' % (seed, a))
        amp = max(amp, a)
    print('stokes_amp = %.2f' % amp)
    out['stokes_amp'] = np.array(amp)

    path = os.path.join(OUT, 'golden_pair.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()

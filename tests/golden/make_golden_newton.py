#!/usr/bin/env python3
"""Golden vectors for Newton's method on the device (tests/test_newton_cpu.py, tests/test_newton_gpu.py) from the REAL reference,
built outside the repository as the header of make_golden.py describes:

    PYTHONPATH=/tmp/pyiga_oracle python3 tests/golden/make_golden_newton.py

Public API only: assemble.Assembler(..., updatable=['w']), assemble.assemble, compute_dirichlet_bcs, RestrictedLinearSystem,
solvers.newton.  The data of the cases (f, g, nu) are those of tests/_newton_model.py.  Stored: inputs and recorded results --
per case the Dirichlet data and x0, every Newton iterate completed with g and ||R F(x_k)||, F(x0), F at a non-smooth random w,
and for the 2D cases the values of J(x0) and J(w_rand) (3D: vectors and iterates only).

The script asserts that every run takes between 3 and 10 steps and that its last two iterates differ by less than 1e-11
(relative): f and the scale of g were chosen so that they hold.  The reference's updatable FUNCTIONAL does not follow an update
of w where the form contains w * grad(w) (it differs from a fresh assembly); the residuals of such a case are assembled afresh
with assemble.assemble(residual, ..., w=...), which the script decides by comparing the two at a random w.
"""
import os
import sys

import numpy as np

import pyiga
from pyiga import approx, bspline, geometry, assemble, solvers

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import _newton_model as model  # noqa: E402  (numpy only: the data of the cases)

pyiga.set_max_threads(1)
OUT = os.path.dirname(os.path.abspath(__file__))


def run(G, name, kvs, geo, f, g, start, freeze=(1,), store_matrix=False):
    residual, jacobian, extra = model.forms(name)
    N = tuple(kv.numdofs for kv in kvs)
    n = int(np.prod(N))
    spline = lambda x: bspline.BSplineFunc(kvs, np.asarray(x).reshape(N))
    w0 = spline(np.zeros(n))
    Fa = assemble.Assembler(residual, kvs, geo=geo, w=w0, f=f, updatable=['w'], **extra)
    Ja = assemble.Assembler(jacobian, kvs, geo=geo, w=w0, updatable=['w'], **extra)
    Fupd = lambda x: np.asarray(Fa.assemble(w=spline(x))).ravel()
    Ffresh = lambda x: np.asarray(assemble.assemble(residual, kvs, geo=geo, w=spline(x), f=f, **extra)).ravel()
    probe = np.random.default_rng(1).uniform(-1.0, 1.0, size=n)
    stale = abs(Fupd(probe) - Ffresh(probe)).max() > 1e-12 * abs(Ffresh(probe)).max()
    if stale:
        print(name, 'the updatable functional differs from a fresh assembly: residuals are assembled afresh')
    Ffull = Ffresh if stale else Fupd
    Jfull = lambda x: Ja.assemble(w=spline(x)).tocsr()
    Jprobe = assemble.assemble(jacobian, kvs, geo=geo, w=spline(probe), **extra)
    assert abs(Jfull(probe) - Jprobe).max() <= 1e-12 * abs(Jprobe).max(), 'the updatable Jacobian differs from a fresh assembly'
    idx, vals = assemble.compute_dirichlet_bcs(kvs, geo, ('all', g))
    idx = np.asarray(idx).ravel()
    vals = np.broadcast_to(np.asarray(vals, dtype=float), idx.shape).copy()
    LS = assemble.RestrictedLinearSystem(Jfull(np.zeros(n)), np.zeros(n), (idx, vals))
    F = lambda xf: LS.restrict_rhs(Ffull(LS.complete(xf)))
    J = lambda xf: LS.restrict_matrix(Jfull(LS.complete(xf)))
    x0 = np.zeros(n) if start == 'zero' else np.asarray(approx.interpolate(kvs, g, geo=geo)).ravel().copy()
    x0[idx] = vals
    xf0 = LS.restrict(x0)
    G[name + 'bc_idx'], G[name + 'bc_val'], G[name + 'x0'] = idx.astype(np.int64), vals, x0
    G[name + 'F_x0'] = Ffull(x0)
    wr = np.random.default_rng(20261018).uniform(-1.0, 1.0, size=n)          # non-smooth on purpose
    G[name + 'w_rand'], G[name + 'F_rand'] = wr, Ffull(wr)
    if store_matrix:
        A0, Ar = Jfull(x0), Jfull(wr)
        A0.sort_indices()
        Ar.sort_indices()
        assert np.array_equal(A0.indices, Ar.indices) and np.array_equal(A0.indptr, Ar.indptr)
        G[name + 'J_indptr'], G[name + 'J_indices'] = A0.indptr.astype(np.int32), A0.indices.astype(np.int32)
        G[name + 'J_x0_data'], G[name + 'J_rand_data'] = A0.data, Ar.data
    nF0 = np.linalg.norm(F(xf0))
    for fj in freeze:
        iterates, norms = [], []

        def Frec(xf):
            r = F(xf)
            iterates.append(LS.complete(xf).copy())
            norms.append(np.linalg.norm(r))
            return r
        solvers.newton(Frec, J, xf0, atol=1e-12 * nF0, rtol=0.0, maxiter=20, freeze_jac=fj)
        its = len(iterates) - 1
        assert 3 <= its <= 10, (name, fj, its, norms)
        last2 = np.linalg.norm(iterates[-1] - iterates[-2]) / np.linalg.norm(iterates[-1])
        assert last2 < 1e-11, (name, fj, last2)
        tag = model.run_key(name, fj)
        G[tag + 'iterates'], G[tag + 'norms'] = np.array(iterates), np.array(norms)
        print('%s freeze_jac=%d: %d iterations, ||F|| %s, last two differ by %.1e' % (name, fj, its, ' '.join('%.2e' % v for v in norms), last2))


G = {}
geo2 = geometry.quarter_annulus()
kvs2 = 2 * (bspline.make_knots(3, 0.0, 1.0, 16),)
geo3 = geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.quarter_annulus())
kvs3 = 3 * (bspline.make_knots(2, 0.0, 1.0, 6),)
run(G, 'cubic2_', kvs2, geo2, *model.CASES['cubic2_'][4:7], freeze=(1, 2), store_matrix=True)
run(G, 'burg2_', kvs2, geo2, *model.CASES['burg2_'][4:7], store_matrix=True)
run(G, 'cubic3_', kvs3, geo3, *model.CASES['cubic3_'][4:7])
G['desc'] = np.array('Newton goldens: cubic2_ / burg2_ on 2 x make_knots(3,0,1,16), quarter_annulus(); cubic3_ on 3 x make_knots(2,0,1,6), '
                     'tensor_product(line_segment(0,1), quarter_annulus()); data in tests/_newton_model.py; atol = 1e-12 ||R F(x0)||, rtol = 0')
path = os.path.join(OUT, 'golden_newton.npz')
np.savez_compressed(path, **G)
print('wrote', path, os.path.getsize(path), 'bytes')

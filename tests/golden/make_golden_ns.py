#!/usr/bin/env python3
"""Golden vectors for the device Navier-Stokes solver (Picard and Newton steps on saddle-point systems), from the REAL reference
(c-f-h/pyiga).

Run where an unmodified build of the reference is importable (see the header of make_golden.py):

    PYTHONPATH=/path/to/built/reference python3 tests/golden/make_golden_ns.py

Writes tests/golden/golden_ns.npz, golden_ns3_stokes.npz and golden_ns3_rand.npz -- data only; the wind-dependent matrices of the
3D case are files of their own, which keeps every file below the size limit of the repository; entries that are exactly zero
(the blocks a form does not couple) are not stored.  Two cases, the stationary problem of the reference's solve-navier-stokes
notebook:

    ns2   spaces, geometry and bcs of `oseen2` / `stokes` (328 unknowns, the first pressure dof pinned)
    ns3   those of `oseen3` / `stokes3` (561 unknowns)

Only the reference's public API: assemble.assemble for A_grad and A_div, A_conv = assemble('grad(u).dot(w).dot(v) * dx', kvs_u,
bfuns=[('u', nc), ('v', nc)], geo=geo, w=BSplineFunc(kvs_u, U)) and A_newt = assemble('grad(w).dot(u).dot(v) * dx', ...) with
the same w; bmat; RestrictedLinearSystem; spsolve.  Both methods start from the Stokes solution and run in correction form, as
the device does: r = b - K_picard(x) x on the free dofs; x += K^-1 r with K = K_picard(x) (Picard) or K_picard(x) + A_newt(x)
(Newton), zero Dirichlet values for the correction; the loop stops when ||r|| < 1e-10 ||r_0||.

Per case: knots, A_grad, A_div, bcs, nu; per method every iterate and ||R F|| before every step and after the last; A_conv and
A_newt at the Stokes start and at one non-smooth random w (coefficients N(0, 1), seeded), with that w.

Two conditions on the cases, asserted here -- conditions, not measurements:
  * the residual falls to 1e-10 of its first value within 30 Picard and 6 Newton steps; nu starts at 0.1 and is doubled until
    that holds;
  * every linear system of both runs converges in the host model of the device solver (tests/_gmres_model.py) in one cycle of
    at most 128 steps: triangular Kronecker preconditioner, restart 128, tol 1e-10.  The counts are written with the case.
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
MAX_STEPS = {'picard': 30, 'newton': 6}
MODEL_MAX = 128
RTOL = 1e-10


def put_csr(out, name, A):
    A = scipy.sparse.csr_matrix(A)
    A.sum_duplicates()
    A.eliminate_zeros()                          # (the blocks a form does not couple are stored as explicit zeros)
    A.sort_indices()
    assert A.has_canonical_format
    out[name + '_data'], out[name + '_indices'], out[name + '_indptr'] = A.data, A.indices, A.indptr
    out[name + '_shape'] = np.array(A.shape)


class Case:
    def __init__(self, geo, kvs_u, kvs_p, sides):
        self.geo, self.kvs_u, self.kvs_p = geo, kvs_u, kvs_p
        self.nc = nc = len(kvs_u)
        self.bf = [('u', nc), ('v', nc)]
        self.ndofs = tuple(kv.numdofs for kv in kvs_u)
        self.N = int(np.prod(self.ndofs))
        self.nv = nc * self.N
        self.A_grad = scipy.sparse.csr_matrix(assemble.assemble('inner(grad(u), grad(v)) * dx', kvs_u, bfuns=self.bf, geo=geo))
        self.A_div = scipy.sparse.csr_matrix(assemble.assemble('div(u) * p * dx', (kvs_u, kvs_p), bfuns=[('u', nc, 0), ('p', 1, 1)],
                                                               geo=geo))
        bcs = assemble.compute_dirichlet_bcs(kvs_u, geo, sides)
        self.bcs = (np.append(bcs[0], self.nv), np.append(bcs[1], 0.0))
        self.n = self.nv + self.A_div.shape[0]
        self.free = np.ones(self.n, dtype=bool)
        self.free[self.bcs[0]] = False

    def wind(self, x):
        U = np.stack([x[c * self.N:(c + 1) * self.N].reshape(self.ndofs) for c in range(self.nc)], axis=-1)
        return bspline.BSplineFunc(self.kvs_u, U)

    def conv(self, x):
        return scipy.sparse.csr_matrix(assemble.assemble('grad(u).dot(w).dot(v) * dx', self.kvs_u, bfuns=self.bf, geo=self.geo,
                                                         w=self.wind(x)))

    def newt(self, x):
        return scipy.sparse.csr_matrix(assemble.assemble('grad(w).dot(u).dot(v) * dx', self.kvs_u, bfuns=self.bf, geo=self.geo,
                                                         w=self.wind(x)))

    def saddle(self, A):
        return scipy.sparse.bmat([[A, self.A_div.T], [self.A_div, None]], format='csr')

    def stokes(self, nu):
        LS = assemble.RestrictedLinearSystem(self.saddle(nu * self.A_grad), 0.0, self.bcs)
        return LS.complete(scipy.sparse.linalg.spsolve(LS.A, LS.b))

    def model_steps(self, A, r, nu):
        """Steps of the model on the correction system, or MODEL_MAX + 1."""
        mats_u = [(assemble.bsp_stiffness_1d(kv), assemble.bsp_mass_1d(kv)) for kv in self.kvs_u]
        mats_p = [(None, assemble.bsp_mass_1d(kv)) for kv in self.kvs_p]
        P = gm.block_preconditioner(self.ndofs, tuple(kv.numdofs for kv in self.kvs_p), self.nc, self.free, mats_u, mats_p,
                                    scale=nu, viscosity=nu)
        zero = (self.bcs[0], np.zeros_like(self.bcs[1]))
        _, info = gm.solve(A, self.A_div, self.nc, zero, b=r, P=P, tol=1e-10, maxiter=MODEL_MAX, restart=MODEL_MAX, triangular=True)
        return info['iterations'] if info['converged'] and info['restarts'] == 0 else MODEL_MAX + 1

    def run(self, method, nu, x0):
        """(iterates, norms, model steps per solve) or None if the run misses the step bound."""
        x = x0.copy()
        iterates, norms, steps = [x.copy()], [], []
        zero = (self.bcs[0], np.zeros_like(self.bcs[1]))
        for it in range(MAX_STEPS[method] + 1):
            Ap = nu * self.A_grad + self.conv(x)
            r = np.where(self.free, -(self.saddle(Ap) @ x), 0.0)
            norms.append(float(np.linalg.norm(r)))
            if norms[-1] < RTOL * norms[0]:
                return np.array(iterates), np.array(norms), steps
            if it == MAX_STEPS[method] or not np.isfinite(norms[-1]):
                return None
            A = Ap + self.newt(x) if method == 'newton' else Ap
            steps.append(self.model_steps(A, r, nu))
            LS = assemble.RestrictedLinearSystem(self.saddle(A), r, zero)
            x = x + LS.complete(scipy.sparse.linalg.spsolve(LS.A, LS.b))
            iterates.append(x.copy())
        return None


def case(out, name, geo, kvs_u, kvs_p, sides, winds=None):
    """`winds`: {tag: dict} that receives the wind-dependent matrices instead of `out`."""
    c = Case(geo, kvs_u, kvs_p, sides)
    for s, kvs in enumerate((kvs_u, kvs_p)):
        for k, kv in enumerate(kvs):
            out['%s_kv%d_%d' % (name, s, k)] = kv.kv
            out['%s_p%d_%d' % (name, s, k)] = np.array(kv.p)
    nu = 0.1
    while True:
        x0 = c.stokes(nu)
        runs = {m: c.run(m, nu, x0) for m in ('picard', 'newton')}
        ok = all(r is not None and max(r[2]) <= MODEL_MAX for r in runs.values())
        print('%s: nu = %g: %s' % (name, nu, {m: None if r is None else (len(r[2]), r[2]) for m, r in runs.items()}))
        if ok:
            break
        nu *= 2.0
    for m, (iterates, norms, steps) in runs.items():
        assert norms[-1] < RTOL * norms[0] and len(steps) <= MAX_STEPS[m] and max(steps) <= MODEL_MAX
        out['%s_%s_iterates' % (name, m)], out['%s_%s_norms' % (name, m)] = iterates, norms
        out['%s_%s_model_steps' % (name, m)] = np.array(steps)
    put_csr(out, name + '_A_grad', c.A_grad)
    put_csr(out, name + '_A_div', c.A_div)
    out[name + '_bcs_idx'], out[name + '_bcs_val'] = np.asarray(c.bcs[0]), np.asarray(c.bcs[1])
    out[name + '_nu'] = np.array(nu)
    w = np.zeros(c.n)
    w[:c.nv] = np.random.default_rng(20261020).standard_normal(c.nv)
    (out if winds is None else winds['rand'])[name + '_w_rand'] = w[:c.nv]
    for tag, x in (('stokes', x0), ('rand', w)):
        dst = out if winds is None else winds[tag]
        put_csr(dst, '%s_A_conv_%s' % (name, tag), c.conv(x))
        put_csr(dst, '%s_A_newt_%s' % (name, tag), c.newt(x))
    print('%s: %d unknowns, nu = %g, Picard %d steps, Newton %d steps' % (name, c.n, nu, len(runs['picard'][2]), len(runs['newton'][2])))


def main():
    out = {}

    def lid2(x, y):
        return (x * y * -y, x * y * x)

    def zero2(x, y):
        return (0.0, 0.0)
    case(out, 'ns2', geometry.quarter_annulus(), tuple(mk(3, 0.0, 1.0, n, mult=2) for n in (6, 4)),
         tuple(mk(2, 0.0, 1.0, n, mult=1) for n in (6, 4)),
         [('bottom', zero2), ('top', zero2), ('left', lid2), ('right', zero2)])
    assert out['ns2_picard_iterates'].shape[1] == 328

    def lid3(x, y, z):
        return (x * y * -y, x * y * x, 0.0 * z)

    def zero3(x, y, z):
        return (0.0, 0.0, 0.0)
    winds3 = {'stokes': {}, 'rand': {}}
    case(out, 'ns3', geometry.twisted_box(), (mk(2, 0., 1., 2, mult=2), mk(2, 0., 1., 3, mult=2), mk(2, 0., 1., 2, mult=2)),
         (mk(1, 0., 1., 2), mk(1, 0., 1., 3), mk(1, 0., 1., 2)),
         [('bottom', zero3), ('top', zero3), ('left', lid3), ('right', zero3), ('front', zero3), ('back', zero3)], winds=winds3)
    assert out['ns3_picard_iterates'].shape[1] == 3 * 175 + 36
    for fname, arrays in (('golden_ns.npz', out), ('golden_ns3_stokes.npz', winds3['stokes']), ('golden_ns3_rand.npz', winds3['rand'])):
        path = os.path.join(OUT, fname)
        np.savez_compressed(path, **arrays)
        print('wrote', path, os.path.getsize(path), 'bytes,', len(arrays), 'arrays')
        assert os.path.getsize(path) < 1024 * 1024


if __name__ == '__main__':
    main()

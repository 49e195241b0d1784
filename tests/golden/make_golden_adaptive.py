#!/usr/bin/env python3
"""Golden runs of parabolic problems with adaptive steps and Rosenbrock methods from the REAL reference (c-f-h/pyiga).

Build the unmodified reference outside the repository as the header of make_golden.py describes, then

    PYTHONPATH=/tmp/pyiga_oracle python3 tests/golden/make_golden_adaptive.py

Writes `tests/golden/golden_adaptive.npz`: inputs and outputs of the reference's public API only (assemble.mass / stiffness /
assemble, inner_products, compute_dirichlet_bcs, approx.project_L2, RestrictedLinearSystem, solvers.coeffs_* and the adaptive
methods solvers.sdirk21 / esdirk23 / esdirk34 / ros3p / ros3pw / rowdaind2 / rodasp / rosi2p1; no reference source).  The three
problems are those of make_golden_parabolic.py (heat2_, heat3_, cd2_) with the same inputs but for the scale of f.  Stored:
  tab_<scheme>_A [_Gamma _b _bhat] _order   the arrays the reference's coeffs_<scheme>() return
  <prefix>rhs bc_idx bc_val u0              the inputs (u0 completed with g)
  tau0 t_end tol const_tau const_t_end      the parameters of the adaptive and of the constant-step (tol=None) runs
  <prefix><scheme>_times _u                 every accepted time and completed state of the reference's adaptive run
  <prefix><scheme>_log                      the attempts (tau, r, accepted) of a direct numpy restatement of the run in this script
  <prefix><scheme>_const_times _u           the reference's constant-step run
The restatement must reproduce the reference's (times, solutions) to 1e-10.  Asserted, not measured: every adaptive run but ros3p
has at least 8 accepted steps and 2 rejections; every attempt has |r - 1| >= 0.01 (a 1e-8 perturbation cannot flip a decision);
every DIRK stage starts above the reference's Newton threshold (rmin > 1e-3, see make_golden_parabolic.py); ros3p has r < 1e-6 on
every attempt (its estimate vanishes for an affine right-hand side).  If one fails: change TOL, TAU0 or the scale of f, not the
assert.  Values chosen: TAU0 = 2^-6, T_END = 0.25, TOL = 1e-3 and F_SCALE = 100 times the f of make_golden_parabolic.py.  (With that
f itself the DIRK stages of all three problems start as low as 5e-4 once the transient has decayed, and with 10 f the rodasp run
of heat2_ has an attempt with |r - 1| = 0.0023; with 100 f the smallest stage residual is 2.0e-2 and the smallest |r - 1| 0.0127.)
"""
import os

import numpy as np

import pyiga
from pyiga import approx, assemble, bspline, geometry, solvers

pyiga.set_max_threads(1)
OUT = os.path.dirname(os.path.abspath(__file__))
G = {}
TAU0 = 2.0 ** -6
T_END = 0.25
TOL = 1e-3
STEP_FACTOR = 0.9
CONST_TAU = 2.0 ** -6
CONST_STEPS = 5
F_SCALE = 100.0

CD2_FORM = '(inner(diff_coeff*grad(u),grad(v))+inner((x[1],-x[0]),grad(u))*v)*dx'
DIRK = ('sdirk21', 'dirk34', 'esdirk23', 'esdirk34')
ROS = ('ros3p', 'ros3pw', 'rowdaind2', 'rodasp', 'rosi2p1')


def kappa2(x, y):
    return 0.2 + 0.1 * x * y


# the tableaux, as the reference returns them
TAB = {}
for name in DIRK:
    A, order = getattr(solvers, 'coeffs_' + name)()
    TAB[name] = (np.array(A, dtype=float), int(order))
    G['tab_%s_A' % name], G['tab_%s_order' % name] = TAB[name]
for name in ROS:
    A, Gam, b, bh, order = getattr(solvers, 'coeffs_' + name)()
    TAB[name] = tuple(np.array(a, dtype=float) for a in (A, Gam, b, bh)) + (int(order),)
    for key, a in zip(('A', 'Gamma', 'b', 'bhat', 'order'), TAB[name]):
        G['tab_%s_%s' % (name, key)] = a


class Direct:
    """One attempt of either family on the restricted system with dense solves; rmin: the smallest absolute residual a DIRK
    stage starts with."""

    def __init__(self, M, K, b):
        self.M, self.K, self.b, self.rmin = M, K, b, np.inf

    def F(self, z):
        return self.b - self.K @ z

    def dirk(self, A, x, tau, Fx):
        s = A.shape[1]
        M = self.M
        ys, Fy = [], []
        for i in range(s):
            aii = A[i, i]
            if aii == 0:
                ys.append(x)
                Fy.append(Fx if Fx is not None else self.F(x))
                continue
            rhs = M @ x + tau * sum(A[i, j] * Fy[j] for j in range(i))
            z = x if i == 0 else ys[-1]
            self.rmin = min(self.rmin, np.linalg.norm(M @ z - tau * aii * self.F(z) - rhs))
            y = np.linalg.solve(M + tau * aii * self.K, rhs + tau * aii * self.b)
            ys.append(y)
            Fy.append(self.F(y))
        x_est = np.linalg.solve(M, M @ x + tau * sum(A[s + 1, i] * Fy[i] for i in range(s)))
        return ys[-1], x_est, Fy[-1]

    def rosenbrock(self, T, x, tau, Fx):
        A, Gam, b, bh, _ = T
        s = len(b)
        C = self.M + tau * Gam[0, 0] * self.K
        ks = []
        for i in range(s):
            y = x + tau * sum((A[i, j] * ks[j] for j in range(i)), np.zeros_like(x))
            rhs = self.F(y)
            if i > 0:
                rhs = rhs - tau * (self.K @ sum(Gam[i, j] * ks[j] for j in range(i)))
            ks.append(np.linalg.solve(C, rhs))
        return x + tau * sum(b[i] * ks[i] for i in range(s)), x + tau * sum(bh[i] * ks[i] for i in range(s)), None


def controlled(step, order, x, tau, t_end, tol):
    """The accept/reject loop; returns times, states and the attempts (tau, r, accepted)."""
    t, Fx = 0.0, None
    times, sols, log = [t], [x], []
    while t < t_end:
        xnew, xhat, Fnew = step(x, tau, Fx)
        r = np.linalg.norm((xhat - xnew) / (tol + tol * abs(x))) / np.sqrt(len(x))
        if r == 0:
            r = 1e-15
        ok = r <= 1
        log.append((tau, r, float(ok)))
        if ok:
            t += tau
            x, Fx = xnew, Fnew
            times.append(t)
            sols.append(x)
        tau *= min(5.0, max(0.2, STEP_FACTOR * r ** (-1 / order)))
    return times, sols, np.array(log)


def run(prefix, kvs, geo, Kmat, f, u0fun, bcs, adaptive, constant):
    M = assemble.mass(kvs, geo)
    rhs = assemble.inner_products(kvs, f, f_physical=True, geo=geo).ravel()
    LSK = assemble.RestrictedLinearSystem(Kmat, rhs, bcs)
    LSM = assemble.RestrictedLinearSystem(M, np.zeros(M.shape[0]), bcs)
    Kf, Mf, bf = LSK.A, LSM.A, LSK.b
    u0 = approx.project_L2(kvs, u0fun, f_physical=True, geo=geo).ravel()
    x0 = LSK.restrict(u0)
    G[prefix + 'rhs'] = rhs
    G[prefix + 'bc_idx'], G[prefix + 'bc_val'] = np.asarray(bcs[0]), np.asarray(bcs[1])
    G[prefix + 'u0'] = np.asarray(LSK.complete(x0)).ravel()
    F, J = (lambda x: bf - Kf @ x), (lambda x: -Kf)
    complete = lambda sols: np.array([np.asarray(LSK.complete(x)).ravel() for x in sols])
    for name in adaptive:
        times, sols = getattr(solvers, name)(Mf, F, J, x0, TAU0, T_END, TOL, step_factor=STEP_FACTOR)
        D = Direct(Mf.toarray(), Kf.toarray(), bf)
        T = TAB[name]
        if name in DIRK:
            rt, rs, log = controlled(lambda x, tau, Fx: D.dirk(T[0], x, tau, Fx), T[1], x0, TAU0, T_END, TOL)
            assert D.rmin > 1e-3, (prefix, name, 'a stage starts below the Newton threshold', D.rmin)
        else:
            rt, rs, log = controlled(lambda x, tau, Fx: D.rosenbrock(T, x, tau, Fx), T[4], x0, TAU0, T_END, TOL)
        assert len(rt) == len(times), (prefix, name, len(rt), len(times))
        scale = max(np.abs(b).max() for b in rs)
        err = max(np.abs(a - b).max() for a, b in zip(sols, rs)) / scale
        terr = np.abs(np.array(times) - np.array(rt)).max()
        assert err < 1e-10 and terr < 1e-10, (prefix, name, err, terr)
        nacc, nrej = int(log[:, 2].sum()), int((1 - log[:, 2]).sum())
        gap = np.abs(log[:, 1] - 1).min()
        if name == 'ros3p':
            assert log[:, 1].max() < 1e-6, (prefix, name, log[:, 1].max())
        else:
            assert nacc >= 8 and nrej >= 2, (prefix, name, nacc, nrej)
        assert gap >= 0.01, (prefix, name, gap)
        G[prefix + name + '_times'] = np.array(times)
        G[prefix + name + '_u'] = complete(sols)
        G[prefix + name + '_log'] = log
        print(prefix, name, 'attempts', len(log), 'accepted', nacc, 'rejected', nrej, 'min |r - 1| %.4f' % gap,
              'min stage residual %.2e' % D.rmin, 'vs restatement %.1e' % err)
    for name in constant:
        t_end = CONST_STEPS * CONST_TAU
        times, sols = getattr(solvers, name)(Mf, F, J, x0, CONST_TAU, t_end, None)
        assert len(sols) == CONST_STEPS + 1, (prefix, name, len(sols))
        D = Direct(Mf.toarray(), Kf.toarray(), bf)
        x, ref = x0, [x0]
        for _ in range(CONST_STEPS):
            x = D.rosenbrock(TAB[name], x, CONST_TAU, None)[0]
            ref.append(x)
        err = max(np.abs(a - b).max() for a, b in zip(sols, ref)) / max(np.abs(b).max() for b in ref)
        assert err < 1e-10, (prefix, name, err)
        G[prefix + name + '_const_times'] = np.array(times)
        G[prefix + name + '_const_u'] = complete(sols)
        print(prefix, name, 'constant steps', len(sols) - 1, 'vs restatement %.1e' % err)


G['tau0'], G['t_end'], G['tol'], G['step_factor'] = np.array(TAU0), np.array(T_END), np.array(TOL), np.array(STEP_FACTOR)
G['const_tau'], G['const_t_end'] = np.array(CONST_TAU), np.array(CONST_STEPS * CONST_TAU)

geo2 = geometry.quarter_annulus()
kvs2 = 2 * (bspline.make_knots(3, 0.0, 1.0, 16),)
run('heat2_', kvs2, geo2, assemble.stiffness(kvs2, geo2),
    lambda x, y: F_SCALE * 20.0 * (1.0 + x * y), lambda x, y: np.sin(2 * x) * np.cos(y) + 0.5,
    assemble.compute_dirichlet_bcs(kvs2, geo2, [('left', lambda x, y: 1.0 + 0.3 * x), ('top', lambda x, y: 0.5 + 0.2 * y)]),
    ('esdirk23', 'sdirk21', 'esdirk34', 'rodasp', 'rosi2p1', 'rowdaind2', 'ros3p'), ('rodasp', 'ros3pw'))

geo3 = geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.quarter_annulus())
kvs3 = 3 * (bspline.make_knots(2, 0.0, 1.0, 6),)
run('heat3_', kvs3, geo3, assemble.stiffness(kvs3, geo3),
    lambda x, y, z: F_SCALE * 30.0 * (1.0 + x - np.sin(z)), lambda x, y, z: np.cos(x + 0.5 * y) * (1 + z),
    assemble.compute_dirichlet_bcs(kvs3, geo3, ('all', lambda x, y, z: np.cos(x + 0.5 * y) + np.exp(0.3 * z - y))),
    ('esdirk23', 'rodasp'), ())

run('cd2_', kvs2, geo2, assemble.assemble(CD2_FORM, kvs2, geo=geo2, diff_coeff=kappa2),
    lambda x, y: F_SCALE * 20.0 * (1.0 + np.cos(x) * y), lambda x, y: np.exp(-x * y) + x,
    assemble.compute_dirichlet_bcs(kvs2, geo2, ('all', lambda x, y: x - 0.5 * y)),
    ('esdirk34', 'rodasp'), ())

path = os.path.join(OUT, 'golden_adaptive.npz')
np.savez_compressed(path, **G)
print('wrote', path, os.path.getsize(path), 'bytes')

#!/usr/bin/env python3
"""Golden trajectories of parabolic problems from the REAL reference (c-f-h/pyiga).

Build the unmodified reference outside the repository as the header of make_golden.py describes, then

    PYTHONPATH=/tmp/pyiga_oracle python3 tests/golden/make_golden_parabolic.py

Writes `tests/golden/golden_parabolic.npz`: inputs and outputs of the reference's public API only (assemble.mass / stiffness /
assemble, inner_products, compute_dirichlet_bcs, approx.project_L2, RestrictedLinearSystem, solvers.crank_nicolson / sdirk3 /
esdirk34(..., tol=None); no reference source).  The problem is  M_ff x' = (f_f - K_fd g) - K_ff x  on the free dofs (the
restricted system); the trajectories are stored completed with g.  Cases (prefix_):
  heat2_  2D quarter annulus, p = 3, n = 16, stiffness, Dirichlet data on the left and top sides, schemes cn / sdirk3 / esdirk34
  heat3_  3D quarter-annulus cylinder, p = 2, n = 6, stiffness, Dirichlet data on every side, schemes sdirk3 / cn
  cd2_    2D convection-diffusion form on the quarter annulus, p = 3, n = 16, every side fixed, schemes sdirk3 / esdirk34
The reference's stage Newton stops without solving when the residual is below an absolute 1e-4 (pyiga/solvers.py:351-356 with
atol=1e-4): |f|, tau and t_end are chosen so that every stage starts above 1e-3, which this script asserts, and the
trajectories must equal a direct numpy DIRK of the restricted system to 1e-10.
"""
import os

import numpy as np

import pyiga
from pyiga import approx, assemble, bspline, geometry, solvers

pyiga.set_max_threads(1)
OUT = os.path.dirname(os.path.abspath(__file__))
G = {}
TAU = 2.0 ** -6
NSTEPS = 5

CD2_FORM = '(inner(diff_coeff*grad(u),grad(v))+inner((x[1],-x[0]),grad(u))*v)*dx'


def kappa2(x, y):
    return 0.2 + 0.1 * x * y


def direct_dirk(A, M, K, b, x, tau, nsteps):
    """The DIRK of the restricted system with dense solves; also the smallest absolute residual any stage starts with."""
    s = A.shape[1]
    F = lambda z: b - K @ z
    out, rmin = [x], np.inf
    Fx = None
    for _ in range(nsteps):
        ys, Fy = [], []
        for i in range(s):
            aii = A[i, i]
            if aii == 0:
                ys.append(x)
                Fy.append(Fx if Fx is not None else F(x))
                continue
            rhs = M @ x + tau * sum(A[i, j] * Fy[j] for j in range(i))
            z = x if i == 0 else ys[-1]
            rmin = min(rmin, np.linalg.norm(M @ z - tau * aii * F(z) - rhs))
            y = np.linalg.solve(M + tau * aii * K, rhs + tau * aii * b)
            ys.append(y)
            Fy.append(F(y))
        x, Fx = ys[-1], Fy[-1]
        out.append(x)
    return out, rmin


def run(prefix, kvs, geo, Kmat, f, u0fun, bcs, schemes):
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
    G[prefix + 'tau'] = np.array(TAU)
    G[prefix + 't_end'] = np.array(NSTEPS * TAU)
    for name, method, A in schemes:
        times, sols = method(Mf, lambda x: bf - Kf @ x, lambda x: -Kf, x0, TAU, NSTEPS * TAU)
        assert len(sols) == NSTEPS + 1, (prefix, name, len(sols))
        ref, rmin = direct_dirk(A, Mf.toarray(), Kf.toarray(), bf, x0, TAU, NSTEPS)
        assert rmin > 1e-3, (prefix, name, 'a stage starts below the Newton threshold', rmin)
        err = max(np.abs(a - b).max() for a, b in zip(sols, ref)) / max(np.abs(b).max() for b in ref)
        assert err < 1e-10, (prefix, name, err)
        G[prefix + name + '_times'] = np.array(times)
        G[prefix + name + '_u'] = np.array([np.asarray(LSK.complete(x)).ravel() for x in sols])
        print(prefix, name, 'steps', len(sols) - 1, 'min stage residual %.2e' % rmin, 'vs direct DIRK %.1e' % err)


def esdirk34(M, F, J, x, tau, t_end):
    return solvers.esdirk34(M, F, J, x, tau, t_end, None)


# the main rules, written out to check the reference against the direct DIRK (the device takes them from dirk_tableau)
g3 = 0.43586652150845899942
b2 = (6 * g3 * g3 - 20 * g3 + 5) / 4
SDIRK3 = np.array([[g3, 0, 0], [(1 - g3) / 2, g3, 0], [1 - b2 - g3, b2, g3], [1 - b2 - g3, b2, g3]])
CN = np.array([[0, 0], [0.5, 0.5], [0.5, 0.5]])
bb = [0.10239940061991099768, -0.3768784522555561061, 0.83861253012718610911, g3]
ESDIRK34 = np.array([[0, 0, 0, 0], [g3, g3, 0, 0], [0.14073777472470619619, -0.1083655513813208000, g3, 0], bb, bb])

geo2 = geometry.quarter_annulus()
kvs2 = 2 * (bspline.make_knots(3, 0.0, 1.0, 16),)
run('heat2_', kvs2, geo2, assemble.stiffness(kvs2, geo2),
    lambda x, y: 20.0 * (1.0 + x * y), lambda x, y: np.sin(2 * x) * np.cos(y) + 0.5,
    assemble.compute_dirichlet_bcs(kvs2, geo2, [('left', lambda x, y: 1.0 + 0.3 * x), ('top', lambda x, y: 0.5 + 0.2 * y)]),
    [('cn', solvers.crank_nicolson, CN), ('sdirk3', solvers.sdirk3, SDIRK3), ('esdirk34', esdirk34, ESDIRK34)])

geo3 = geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.quarter_annulus())
kvs3 = 3 * (bspline.make_knots(2, 0.0, 1.0, 6),)
run('heat3_', kvs3, geo3, assemble.stiffness(kvs3, geo3),
    lambda x, y, z: 30.0 * (1.0 + x - np.sin(z)), lambda x, y, z: np.cos(x + 0.5 * y) * (1 + z),
    assemble.compute_dirichlet_bcs(kvs3, geo3, ('all', lambda x, y, z: np.cos(x + 0.5 * y) + np.exp(0.3 * z - y))),
    [('sdirk3', solvers.sdirk3, SDIRK3), ('cn', solvers.crank_nicolson, CN)])

run('cd2_', kvs2, geo2, assemble.assemble(CD2_FORM, kvs2, geo=geo2, diff_coeff=kappa2),
    lambda x, y: 20.0 * (1.0 + np.cos(x) * y), lambda x, y: np.exp(-x * y) + x,
    assemble.compute_dirichlet_bcs(kvs2, geo2, ('all', lambda x, y: x - 0.5 * y)),
    [('sdirk3', solvers.sdirk3, SDIRK3), ('esdirk34', esdirk34, ESDIRK34)])

path = os.path.join(OUT, 'golden_parabolic.npz')
np.savez_compressed(path, **G)
print('wrote', path, os.path.getsize(path), 'bytes')

"""A numpy restatement of the Newton problems of tests/golden/golden_newton.npz (dense solves): the data of the three cases, the
residual F(w) and the Jacobian J(w) by quadrature with the tables of the CPU oracle (oracle/iga_oracle.py), and the reference's
loop (pyiga/solvers.py:335-361) on the restricted system.  Used by the CPU tests (the model against the golden iterates, the
sensitivity measurement) and by the GPU tests (the tolerance T).

The data were chosen so that every reference run takes between 3 and 10 steps and ends with its last two iterates within 1e-11
of each other (tests/golden/make_golden_newton.py asserts both)."""
import numpy as np

from oracle import iga_oracle as orc

RES_CUBIC = '(inner(grad(w),grad(v)) + w**3*v - f*v)*dx'
JAC_CUBIC = '(inner(grad(u),grad(v)) + 3*w**2*u*v)*dx'
RES_BURG = '(nu*inner(grad(w),grad(v)) + w*grad(w)[0]*v - f*v)*dx'
JAC_BURG = '(nu*inner(grad(u),grad(v)) + w*grad(u)[0]*v + grad(w)[0]*u*v)*dx'
NU = 0.1

# What a relative residual of lin_tol = 1e-10 in every linear solve does to the golden runs: the largest deviation of any
# iterate, relative to the largest entry, over all runs and 3 random disturbances each (measure_sensitivity(); test_newton_cpu.py
# checks that the measurement does not exceed it).  The GPU comparison allows T = min(10 x that, 1e-6): ten times because the
# device's rounding and its true residuals differ from one synthetic disturbance.
SENSITIVITY_MEASURED = 4.1e-10
T = min(10 * SENSITIVITY_MEASURED, 1e-6)

# case -> (dim, degree, spans, problem, f, g, start); the spaces are those of the parabolic goldens.  start: x0 on the free dofs,
# 'zero' or 'g' (the interpolant of the function g on the whole patch: the frozen-Jacobian run of cubic2_ ends with a last
# increment below 1e-11 only from a start whose residual is small against the iterate).  The golden file stores x0.
CASES = {
    'cubic2_': (2, 3, 16, 'cubic', lambda x, y: 1.03 * (10.0 * np.sin(2 * x) * np.cos(y) + 6.0),
                lambda x, y: 2.1783 * (1.0 + 0.53 * x - 0.3 * y), 'g'),
    'burg2_': (2, 3, 16, 'burg', lambda x, y: 0.2 * (10.0 * np.sin(2 * x) * np.cos(y) + 5.0), lambda x, y: 0.5 * (1.0 + 0.5 * x - 0.3 * y),
               'zero'),
    'cubic3_': (3, 2, 6, 'cubic', lambda x, y, z: 10.0 * np.cos(x + 0.5 * y) * (1 + z),
                lambda x, y, z: 2.5 * (np.cos(x + 0.5 * y) + np.exp(0.3 * z - y)), 'zero'),
}
RUNS = [('cubic2_', 1), ('cubic2_', 2), ('burg2_', 1), ('cubic3_', 1)]


def forms(case):
    """(residual string, jacobian string, extra inputs) of a case."""
    return (RES_CUBIC, JAC_CUBIC, {}) if CASES[case][3] == 'cubic' else (RES_BURG, JAC_BURG, dict(nu=NU))


def run_key(case, freeze):
    return case if freeze == 1 else case + 'freeze%d_' % freeze


class Problem:
    """Quadrature tables of a case: Phi (points x dofs), its physical derivatives, the weights W = gw |det J| and f."""

    def __init__(self, case):
        dim, p, n, self.kind, f, _ = CASES[case][:6]
        kvs = [orc.make_knots(p, 0.0, 1.0, n) for _ in range(dim)]
        geo = orc.geo_quarter_annulus() if dim == 2 else orc.geo_cylinder()
        grid, gw = orc.make_tensor_quadrature([kv.mesh for kv in kvs], p + 1)
        B = [orc.collocation_derivs_dense(kv, g, 1) for kv, g in zip(kvs, grid)]

        def tensor(orders):
            out = np.ones((1, 1))
            for k in range(dim):
                out = np.kron(out, B[k][orders[k]])
            return out
        self.N = tuple(kv.numdofs for kv in kvs)
        self.n = int(np.prod(self.N))
        self.Phi = tensor((0,) * dim)
        # parametric derivatives in (x, y, z) order: x belongs to the LAST grid axis
        par = [tensor(tuple(1 if k == dim - 1 - c else 0 for k in range(dim))) for c in range(dim)]
        Jm = orc.grid_jacobian(geo, grid).reshape(-1, dim, dim)          # [r][c] = d G_r / d xi_c
        JI = np.linalg.inv(Jm)                                            # [c][r] = d xi_c / d x_r
        self.D = [sum(JI[:, c, r][:, None] * par[c] for c in range(dim)) for r in range(dim)]
        W = np.ones(())
        for w in gw:
            W = np.multiply.outer(W, w)
        self.W = W.ravel() * np.abs(np.linalg.det(Jm))
        X = orc.grid_eval(geo, grid).reshape(-1, dim)
        self.f = np.broadcast_to(f(*(X[:, k] for k in range(dim))), self.W.shape)
        self.dim = dim

    def F(self, x):
        x = np.asarray(x).ravel()
        w = self.Phi @ x
        g = [D @ x for D in self.D]
        if self.kind == 'cubic':
            c0, cg = w ** 3 - self.f, g
        else:
            c0, cg = w * g[0] - self.f, [NU * gr for gr in g]
        return self.Phi.T @ (self.W * c0) + sum(D.T @ (self.W * c) for D, c in zip(self.D, cg))

    def J(self, x):
        x = np.asarray(x).ravel()
        w = self.Phi @ x
        if self.kind == 'cubic':
            A = sum(D.T @ (self.W[:, None] * D) for D in self.D) + self.Phi.T @ ((self.W * 3 * w ** 2)[:, None] * self.Phi)
        else:
            wx = self.D[0] @ x
            A = NU * sum(D.T @ (self.W[:, None] * D) for D in self.D)
            A = A + self.Phi.T @ ((self.W * w)[:, None] * self.D[0]) + self.Phi.T @ ((self.W * wx)[:, None] * self.Phi)
        return A


def newton(prob, bc_idx, x0, atol, rtol, maxiter, freeze_jac=1, lin_tol=0.0, rng=None):
    """The reference's loop on the restricted system with dense solves; every iterate completed with g, and ||R F|| at each.
    lin_tol > 0: every linear solve is disturbed to that relative residual (a random direction)."""
    free = np.ones(prob.n, dtype=bool)
    free[np.asarray(bc_idx, dtype=np.int64)] = False
    x = np.array(x0, dtype=float).ravel()
    res = prob.F(x)[free]
    iterates, norms = [x.copy()], [np.linalg.norm(res)]
    target = max(atol, rtol * norms[0])
    for it in range(maxiter):
        if norms[-1] < target:
            return iterates, norms, True
        if it % freeze_jac == 0:
            Jff = prob.J(x)[np.ix_(free, free)]
        rhs = res
        if lin_tol > 0.0:
            u = rng.standard_normal(res.size)
            rhs = res + lin_tol * norms[-1] * u / np.linalg.norm(u)
        x[free] -= np.linalg.solve(Jff, rhs)
        res = prob.F(x)[free]
        iterates.append(x.copy())
        norms.append(np.linalg.norm(res))
    return iterates, norms, False


def measure_sensitivity(golden, lin_tol=1e-10, samples=3):
    """Largest deviation of any iterate, relative to the largest entry of the golden iterates, when every linear solve of the
    golden runs is disturbed to the relative residual lin_tol."""
    worst = 0.0
    probs = {}
    for case, freeze in RUNS:
        prob = probs.setdefault(case, Problem(case))
        gold = golden[run_key(case, freeze) + 'iterates']
        nF0 = golden[run_key(case, freeze) + 'norms'][0]
        for s in range(samples):
            its, _, _ = newton(prob, golden[case + 'bc_idx'], golden[case + 'x0'], 1e-12 * nF0, 0.0, len(gold) - 1, freeze,
                               lin_tol=lin_tol, rng=np.random.default_rng(100 + s))
            m = min(len(its), len(gold))
            worst = max(worst, abs(np.array(its[:m]) - gold[:m]).max() / abs(gold).max())
    return worst

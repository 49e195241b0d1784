"""Host models of the adaptive time stepping on the device (solvers.ParabolicSystem.integrate_adaptive, igx_solver_step_*;
DESIGN.md section 18).

- ``Restricted``: the reference's embedded DIRK step and Rosenbrock step (pyiga/solvers.py:366-435, 684-707) with exact solves on
  the restricted system ``M_ff x' = (f_f - K_fd g) - K_ff x``.
- ``Lifted``: the formulation the device runs, on full vectors with g on the fixed dofs (masked products, the lifting of g, the
  Rosenbrock stages written with ``B = A + Gamma``).
- ``controller`` / ``run``: the accept/reject loop (pyiga/solvers.py:505-531) with the bound ``max_attempts``.
- ``stability_rosenbrock``: ``R(z) = 1 + z b^T (I - z (A + Gamma))^-1 1``; ``stability_weights`` the same for any weights (the
  embedded rule); ``rosenbrock_order_conditions``: the residuals of orders 1 and 2 with ``B = A + Gamma``.

Every model takes ``perturb``: a relative size by which the right-hand side of every solve is disturbed (a residual of that
size, as an iterative solve stopped at ``||r|| <= perturb ||rhs||`` leaves), from a seeded generator.
"""
import numpy as np
import scipy.sparse
import scipy.sparse.linalg

# What a relative residual of 1e-10 (the device's solve_tol) in every solve does to the golden runs of golden_adaptive.npz: the
# largest deviation of the accepted times (relative to t_end) and states (relative to the largest state entry) from the
# unperturbed model, measured by tests/test_adaptive_cpu.py::test_sensitivity_to_the_solve_tolerance over the 11 adaptive runs
# in the device's formulation (Lifted(difference=True)): 4.25e-7 (cd2_ rodasp; heat3_ rodasp 4.1e-7, heat2_ rodasp 2.2e-7, the
# DIRK runs 2.2e-9 to 1.8e-7, ros3p 3.8e-11; no decision flips).  The estimate is of the order tol |x| = 1e-3 |x|, so a residual
# in a stage solve reaches r amplified by 1 / tol.  (With the DIRK stages solved for y_i to a residual relative to ||b_i||, and not
# for the increment from y_{i-1}, the DIRK runs moved by up to 2.5e-6.)  The GPU comparison allows T = min(10 x that, 1e-6): ten
# times because the device's rounding and its true residuals differ from one synthetic disturbance; the cap of 1e-6 holds here.
SENSITIVITY_MEASURED = 4.3e-7
T = min(10 * SENSITIVITY_MEASURED, 1e-6)


def _split(n, bc_idx):
    fixed = np.zeros(n, dtype=bool)
    fixed[np.asarray(bc_idx, dtype=np.int64)] = True
    return np.flatnonzero(~fixed), np.flatnonzero(fixed)


class _Solves:
    """Exact solves with C = M + tg K (factorized once per tg) and with M, the right-hand side disturbed by `perturb`."""

    def __init__(self, Mf, Kf, perturb, seed):
        self.Mf, self.Kf, self.perturb = scipy.sparse.csc_matrix(Mf), scipy.sparse.csc_matrix(Kf), perturb
        self.rng = np.random.default_rng(seed)
        self.lu = {}

    def _rhs(self, r):
        if not self.perturb:
            return r
        e = self.rng.standard_normal(r.size)
        return r + self.perturb * np.linalg.norm(r) / np.linalg.norm(e) * e

    def solve(self, tg, r):
        if tg not in self.lu:
            if len(self.lu) > 4:
                self.lu.clear()
            self.lu[tg] = scipy.sparse.linalg.splu(self.Mf if tg is None else scipy.sparse.csc_matrix(self.Mf + tg * self.Kf))
        return self.lu[tg].solve(self._rhs(r))


class Restricted:
    """One attempt on the restricted system; ``dirk(A, x, tau, Fx)`` (A of shape (s + 2, s)) and ``rosenbrock((A, Gamma, b, b_hat),
    x, tau, Fx)`` return ``(x_new, x_est, F_new)``; ``complete(x)`` the full vector."""

    def __init__(self, M, K, f, bc_idx, bc_val, perturb=0.0, seed=0):
        M, K = scipy.sparse.csr_matrix(M), scipy.sparse.csr_matrix(K)
        self.fr, fx = _split(M.shape[0], bc_idx)
        self.g = np.zeros(M.shape[0])
        self.g[bc_idx] = bc_val
        self.Mf, self.Kf = M[self.fr][:, self.fr], K[self.fr][:, self.fr]
        self.bf = f[self.fr] - K[self.fr][:, fx] @ self.g[fx]
        self.S = _Solves(self.Mf, self.Kf, perturb, seed)

    def start(self, u0):
        return np.asarray(u0, dtype=float)[self.fr].copy()

    def complete(self, x):
        u = self.g.copy()
        u[self.fr] = x
        return u

    def weight(self, x):
        return x

    def F(self, z):
        return self.bf - self.Kf @ z

    def dirk(self, A, x, tau, Fx):
        s = A.shape[1]
        gamma = max(A[i, i] for i in range(s))
        ys, Fy = [], []
        for i in range(s):
            if A[i, i] == 0:
                ys.append(x)
                Fy.append(Fx if Fx is not None else self.F(x))
                continue
            rhs = self.Mf @ x + tau * sum((A[i, j] * Fy[j] for j in range(i)), np.zeros_like(x)) + tau * gamma * self.bf
            ys.append(self.S.solve(tau * gamma, rhs))
            Fy.append(self.F(ys[-1]))
        x_est = None
        if A.shape[0] == s + 2:
            x_est = self.S.solve(None, self.Mf @ x + tau * sum(A[s + 1, i] * Fy[i] for i in range(s)))
        return ys[-1], x_est, Fy[-1]

    def rosenbrock(self, T, x, tau, Fx=None):
        A, Gam, b, bh = T[:4]
        s = len(b)
        tg = tau * Gam[0, 0]
        ks = []
        for i in range(s):
            y = x + tau * sum((A[i, j] * ks[j] for j in range(i)), np.zeros_like(x))
            rhs = self.F(y)
            if i > 0:
                rhs = rhs - tau * (self.Kf @ sum(Gam[i, j] * ks[j] for j in range(i)))
            ks.append(self.S.solve(tg, rhs))
        x_est = None if bh is None else x + tau * sum(bh[i] * ks[i] for i in range(s))
        return x + tau * sum(b[i] * ks[i] for i in range(s)), x_est, None


class Lifted(Restricted):
    """The same attempts as the device forms them: full vectors, R the mask of the free dofs, w = ext(g).  `difference`: as
    the device runs it, every DIRK stage is solved for its increment from the guess y_{i-1} (so that a
    disturbance is relative to the residual the guess leaves) and the embedded estimate by the mass solve for x_est - x_new
    itself; else stages and x_est as the reference writes them."""

    def __init__(self, M, K, f, bc_idx, bc_val, perturb=0.0, seed=0, difference=False):
        Restricted.__init__(self, M, K, f, bc_idx, bc_val, perturb, seed)
        self.difference = difference
        self.M, self.K, self.f = scipy.sparse.csr_matrix(M), scipy.sparse.csr_matrix(K), np.asarray(f, dtype=float)
        self.free = np.zeros(self.M.shape[0])
        self.free[self.fr] = 1.0
        self.bc_idx, self.bc_val = bc_idx, bc_val

    def start(self, u0):
        x = np.asarray(u0, dtype=float).copy()
        x[self.bc_idx] = self.bc_val
        return x

    def complete(self, x):
        return x

    def weight(self, x):
        return x[self.fr]

    def _lifted_solve(self, tg, b, lift):
        """R A R^T y = R (b - A w) (w = ext(g) if `lift`), y zero on the fixed dofs."""
        Amat = self.M if tg is None else self.M + tg * self.K
        r = self.free * (b - Amat @ self.g) if lift else self.free * b
        y = np.zeros_like(b)
        y[self.fr] = self.S.solve(tg, r[self.fr])
        return y

    def dirk(self, A, x, tau, Fx):
        s = A.shape[1]
        gamma = max(A[i, i] for i in range(s))
        free, f, K = self.free, self.f, self.K
        Mx = free * (self.M @ x)
        F = [None] * s
        last = x
        for i in range(s):
            if A[i, i] == 0:
                F[0] = Fx if Fx is not None else free * (f - K @ x)
                continue
            b = Mx + tau * sum((A[i, j] * F[j] for j in range(i)), np.zeros_like(x)) + tau * gamma * f
            if self.difference:
                # what the device solves: the increment from the guess y_{i-1}, to a residual relative to the one the guess leaves
                guess = free * last
                Cm = self.M + tau * gamma * self.K
                last = guess + self._lifted_solve(tau * gamma, b - Cm @ (self.g + guess), False) + self.g
            else:
                last = self._lifted_solve(tau * gamma, b, True) + self.g
            F[i] = free * (f - K @ last)
        x_est = None
        if A.shape[0] == s + 2 and self.difference:
            # what the device solves: M x_new = M x + tau sum b_i F_i (the last stage), so M e = tau sum (b^_i - b_i) F_i
            x_est = last + self._lifted_solve(None, tau * sum((A[s + 1, i] - A[s, i]) * F[i] for i in range(s)), False)
        elif A.shape[0] == s + 2:
            b = Mx + tau * sum(A[s + 1, i] * F[i] for i in range(s))
            x_est = self._lifted_solve(None, b, True) + self.g
        return last, x_est, F[s - 1]

    def rosenbrock(self, T, x, tau, Fx=None):
        A, Gam, b, bh = T[:4]
        s = len(b)
        B = A + Gam
        tg = tau * Gam[0, 0]
        ks = []
        for i in range(s):
            y = x + tau * sum((B[i, j] * ks[j] for j in range(i)), np.zeros_like(x))
            ks.append(self._lifted_solve(tg, self.free * (self.f - self.K @ y), False))
        x_est = None if bh is None else x + tau * sum(bh[i] * ks[i] for i in range(s))
        return x + tau * sum(b[i] * ks[i] for i in range(s)), x_est, None


def error_ratio(x_est, x_new, x, tol):
    """r of the reference: || (x_est - x_new) / (tol + tol |x|) ||_2 / sqrt(len(x)) (vectors of the free dofs)."""
    return np.linalg.norm((x_est - x_new) / (tol + tol * np.abs(x))) / np.sqrt(len(x))


def controller(tau, r, converged, step_factor, err_order):
    """(accepted, next tau) after one attempt: r == 0 counts as 1e-15, accepted iff r <= 1, the step changes by
    min(5, max(0.2, step_factor r^(-1/err_order))) either way; an attempt that did not converge is rejected and halves the step."""
    if not converged:
        return False, 0.5 * tau
    if r == 0:
        r = 1e-15
    return bool(r <= 1), tau * min(5.0, max(0.2, step_factor * r ** (-1 / err_order)))


def run(step, model, u0, tau0, t_end, tol, err_order, t0=0.0, step_factor=0.9, max_attempts=10000):
    """The adaptive loop ``while t < t_end`` over ``step(x, tau, Fx) -> (x_new, x_est, F_new)`` (a NoConvergence raised by it
    rejects the attempt).  Returns ``(times, full states, log of (tau, r, accepted), finished)``."""
    x = model.start(u0)
    t, tau, Fx = t0, tau0, None
    times, sols, log = [t], [model.complete(x)], []
    while t < t_end:
        if len(log) >= max_attempts:
            return times, sols, np.array(log).reshape(-1, 3), False
        try:
            x_new, x_est, F_new = step(x, tau, Fx)
            r = error_ratio(model.weight(x_est), model.weight(x_new), model.weight(x), tol)
            ok, nxt = controller(tau, r, True, step_factor, err_order)
        except NoConvergence:
            r, (ok, nxt) = np.nan, controller(tau, None, False, step_factor, err_order)
        log.append((tau, 1e-15 if r == 0 else r, float(ok)))
        if ok:
            t += tau
            x, Fx = x_new, F_new
            times.append(t)
            sols.append(model.complete(x))
        tau = nxt
    return times, sols, np.array(log).reshape(-1, 3), True


class NoConvergence(Exception):
    pass


def stability_weights(B, w, z):
    """1 + z w^T (I - z B)^-1 1: the stability function of the weights w over the stage matrix B (s x s)."""
    s = len(w)
    return 1.0 + z * np.asarray(w) @ np.linalg.solve(np.eye(s) - z * np.asarray(B), np.ones(s))


def stability_rosenbrock(A, Gamma, b, z):
    """R(z) = 1 + z b^T (I - z (A + Gamma))^-1 1; z = -inf: the limit 1 - b^T (A + Gamma)^-1 1."""
    B = np.asarray(A) + np.asarray(Gamma)
    if np.isinf(z):
        return 1.0 - np.asarray(b) @ np.linalg.solve(B, np.ones(len(b)))
    return stability_weights(B, b, z)


def rosenbrock_order_conditions(A, Gamma, b):
    """Residuals {1: sum b - 1, 2: b.(A + Gamma).1 - 1/2} of the order conditions of an autonomous problem."""
    B = np.asarray(A) + np.asarray(Gamma)
    return {1: float(np.sum(b) - 1), 2: float(np.asarray(b) @ B.sum(axis=1) - 0.5)}

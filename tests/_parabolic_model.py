"""Host models of the device DIRK time stepping (solvers.ParabolicSystem, igx_solver_dirk_run).

- ``restricted_dirk``: the reference's DIRK (pyiga/solvers.py:366-439 with exact stage solves) on the restricted system
  ``M_ff x' = (f_f - K_fd g) - K_ff x``.
- ``lifted_dirk``: the formulation the device runs, on full vectors with g on the fixed dofs: ``b_i = M x + tau sum a_ij F_j +
  tau gamma f``, ``R C R^T y = R (b_i - C ext(g))``, ``F_i = R (f - K y_i)``.
- ``stability``: ``R(z) = 1 + z b^T (I - z A)^-1 1``; ``order_conditions``: the residuals of the conditions up to order 3.
"""
import numpy as np
import scipy.sparse
import scipy.sparse.linalg


def _split(n, bc_idx):
    fixed = np.zeros(n, dtype=bool)
    fixed[np.asarray(bc_idx, dtype=np.int64)] = True
    return np.flatnonzero(~fixed), np.flatnonzero(fixed)


def stage_solver(M, K, bc_idx, tau, gamma):
    """The exact stage solve of restricted_dirk, y = (M_ff + tau gamma K_ff)^-1 r, factorized once: for several integrations with
    one tau and gamma at a size where the factorization is most of the model's time (minimum-degree ordering on the symmetric
    pattern: a third of the default's time at 264 k dofs)."""
    M, K = scipy.sparse.csr_matrix(M), scipy.sparse.csr_matrix(K)
    fr, _ = _split(M.shape[0], bc_idx)
    C = scipy.sparse.csc_matrix(M[fr][:, fr] + tau * gamma * K[fr][:, fr])
    return scipy.sparse.linalg.splu(C, permc_spec='MMD_AT_PLUS_A').solve


def restricted_dirk(A, M, K, f, bc_idx, bc_val, u0, tau, nsteps, solve=None):
    """Full state vectors (g on the fixed dofs) after 0 .. nsteps steps.  `solve`: the stage solve of stage_solver, if it was
    factorized already."""
    M, K = scipy.sparse.csr_matrix(M), scipy.sparse.csr_matrix(K)
    fr, fx = _split(M.shape[0], bc_idx)
    g = np.zeros(M.shape[0])
    g[bc_idx] = bc_val
    Mf, Kf = M[fr][:, fr], K[fr][:, fr]
    bf = f[fr] - K[fr][:, fx] @ g[fx]
    s = A.shape[1]
    gamma = max(A[i, i] for i in range(s))
    if solve is None:
        solve = scipy.sparse.linalg.factorized(scipy.sparse.csc_matrix(Mf + tau * gamma * Kf))
    x = np.asarray(u0, dtype=float)[fr].copy()
    Fx = None
    out = [x]
    for _ in range(nsteps):
        ys, Fy = [], []
        for i in range(s):
            if A[i, i] == 0:
                ys.append(x)
                Fy.append(Fx if Fx is not None else bf - Kf @ x)
                continue
            rhs = Mf @ x + tau * sum((A[i, j] * Fy[j] for j in range(i)), np.zeros_like(x)) + tau * gamma * bf
            y = solve(rhs)
            ys.append(y)
            Fy.append(bf - Kf @ y)
        x, Fx = ys[-1], Fy[-1]
        out.append(x)
    full = []
    for x in out:
        u = g.copy()
        u[fr] = x
        full.append(u)
    return full


def lifted_dirk(A, M, K, f, bc_idx, bc_val, u0, tau, nsteps):
    """The same integration in the device's full-vector formulation (masked products, the lifting of g)."""
    M, K = scipy.sparse.csr_matrix(M), scipy.sparse.csr_matrix(K)
    n = M.shape[0]
    fr, fx = _split(n, bc_idx)
    free = np.zeros(n)
    free[fr] = 1.0
    w = np.zeros(n)
    w[bc_idx] = bc_val
    s = A.shape[1]
    gamma = max(A[i, i] for i in range(s))
    Cm = M + tau * gamma * K
    solve = scipy.sparse.linalg.factorized(scipy.sparse.csc_matrix(Cm[fr][:, fr]))
    x = np.asarray(u0, dtype=float).copy()
    x[bc_idx] = bc_val
    F0 = free * (f - K @ x) if A[0, 0] == 0 else None
    out = [x.copy()]
    for _ in range(nsteps):
        Mx = free * (M @ x)
        F = [None] * s
        F[0] = F0
        for i in range(s):
            if A[i, i] == 0:
                continue
            b = Mx + tau * sum((A[i, j] * F[j] for j in range(i)), np.zeros(n)) + tau * gamma * f
            r = free * (b - Cm @ w)
            y = w.copy()
            y[fr] = solve(r[fr])
            F[i] = free * (f - K @ y)
            last = y
        x = last
        F0 = F[s - 1]
        out.append(x.copy())
    return out


def stability(A, z):
    """R(z) = 1 + z b^T (I - z A)^-1 1 of the tableau A ((s + 1) x s, b the last row)."""
    s = A.shape[1]
    if np.isinf(z):
        # the limit z -> -inf of the rational form det(I - z (A - 1 b^T)) / det(I - z A), to O(1e-8)
        z = -1e8
        E = np.eye(s)
        return np.linalg.det(E - z * (A[:s] - np.outer(np.ones(s), A[s]))) / np.linalg.det(E - z * A[:s])
    return 1.0 + z * A[s] @ np.linalg.solve(np.eye(s) - z * A[:s], np.ones(s))


def order_conditions(A):
    """Residuals of the order conditions: {1: [sum b - 1], 2: [b.c - 1/2], 3: [b.c^2 - 1/3, b.A.c - 1/6]}."""
    s = A.shape[1]
    b, a = A[s], A[:s]
    c = a.sum(axis=1)
    return {1: [b.sum() - 1], 2: [b @ c - 0.5], 3: [b @ c ** 2 - 1 / 3, b @ a @ c - 1 / 6]}

"""The block kernels of the eigen-solver alone, against numpy on the CSR matrices the device assembles for the same patch
(tests/_eig_cases.py: every (GW, MB) instantiation of k_spmm2, every width of the other kernels, every grid-stride wrap).

Tolerance 1e-12 relative to the largest entry of the result: the same sums as numpy's in another order (the bound
tests/test_solver_kernels_gpu.py uses for the SpMV)."""
import numpy as np
import pytest

import _eig_cases as EC
import _eig_model as EM

pytestmark = pytest.mark.gpu

TOL = 1e-12
SHIFTED = '(inner(grad(u), grad(v)) + u*v) * dx'          # K + M: the operator of the case without any fixed dof


def geo_for(dim):
    from pyiga_amd import geometry
    return geometry.bspline_quarter_annulus() if dim == 2 else geometry.tensor_product(geometry.line_segment(0.0, 1.0),
                                                                                         geometry.bspline_quarter_annulus())


def close(got, want):
    scale = np.abs(want).max()
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= TOL * (scale if scale > 0 else 1.0), np.abs(got - want).max() / scale


def masks(ndofs):
    n = int(np.prod(ndofs))
    rng = np.random.default_rng(n)
    return {'sides': EM.boundary_dofs(ndofs), 'scattered': np.sort(rng.choice(n, size=max(1, n // 5), replace=False)),
            'none': np.zeros(0, dtype=np.int64)}


def host_matrices(kvs, geo):
    from pyiga_amd import assemble
    return assemble.stiffness(kvs, geo).tocsr(), assemble.mass(kvs, geo).tocsr()


def restricted(A, free, X):
    """R A R^T X on full-length blocks."""
    Xm = np.where(free[:, None], X, 0.0)
    return np.where(free[:, None], A @ Xm, 0.0)


def check_products(S, K, M, fixed, columns, seed):
    n = K.shape[0]
    free = np.ones(n, dtype=bool)
    free[fixed] = False
    rng = np.random.default_rng(seed)
    for m in columns:
        X = rng.standard_normal((n, m))                    # (not masked: the product masks its input)
        YK, YM = S.block_products(X)
        close(YK, restricted(K, free, X))
        close(YM, restricted(M, free, X))
        assert np.all(YK[fixed] == 0.0) and np.all(YM[fixed] == 0.0)
    m = columns[-1]
    X = rng.standard_normal((n, m))
    close(S.block_product(X, 'K'), restricted(K, free, X))     # the one-matrix form
    close(S.block_product(X, 'M'), restricted(M, free, X))


@pytest.mark.parametrize('case', EC.SMALL_CASES, ids=lambda c: c.id)
def test_block_products_every_width_and_mask(case):
    from pyiga_amd import solvers
    kvs, geo = case.patch.kvs(), geo_for(case.patch.dim)
    K, M = host_matrices(kvs, geo)
    ndofs = tuple(kv.numdofs for kv in kvs)
    for name, fixed in masks(ndofs).items():
        S = solvers.EigenSystem(kvs, geo, fixed, problem=SHIFTED if name == 'none' else None)
        try:
            check_products(S, K + M if name == 'none' else K, M, fixed, case.columns, len(name))
        finally:
            S.close()


@pytest.mark.parametrize('case', EC.WRAP_CASES, ids=lambda c: c.id)
def test_block_products_past_one_pass(case):
    from pyiga_amd import solvers
    kvs, geo = case.patch.kvs(), geo_for(case.patch.dim)
    K, M = host_matrices(kvs, geo)
    ndofs = tuple(kv.numdofs for kv in kvs)
    assert K.shape[0] > EC.spmm_pass_rows(case.patch.gw)
    fixed = EM.boundary_dofs(ndofs)
    S = solvers.EigenSystem(kvs, geo, fixed)
    try:
        check_products(S, K, M, fixed, case.columns, 5)
    finally:
        S.close()


@pytest.mark.parametrize('case', EC.ROWS_CASES, ids=lambda c: c.id)
def test_gram_combine_residuals_precond(case):
    """The other block kernels at every width: Gram matrices of one to three blocks a side, combinations of one to three
    blocks, the fused residual with its column norms, and the three preconditioners column by column against the
    single-vector PatchSystem.apply_precond of the same patch."""
    from pyiga_amd import geometry, solvers
    kvs, geo = case.kvs(), geometry.unit_square()
    ndofs = tuple(kv.numdofs for kv in kvs)
    n = int(np.prod(ndofs))
    assert n == case.rows()
    fixed = EM.boundary_dofs(ndofs)
    free = np.ones(n, dtype=bool)
    free[fixed] = False
    rng = np.random.default_rng(n)
    S = solvers.EigenSystem(kvs, geo, fixed)
    P = solvers.PatchSystem(kvs, geo, np.zeros(n), (fixed, np.zeros(fixed.size)), kind='stiffness')
    try:
        for m in case.columns:
            blocks = [rng.standard_normal((n, m)) for _ in range(6)]
            for na, nb in ((1, 1), (2, 3), (3, 3)):
                A, B = blocks[:na], blocks[3:3 + nb]
                want = np.hstack(A)[free].T @ np.hstack(B)[free]
                close(S.gram(A, B), want)
            close(S.gram(blocks[0], blocks[1]), blocks[0][free].T @ blocks[1][free])
            for ns in (1, 2, 3):
                coeffs = [rng.standard_normal((m, m)) for _ in range(ns)]
                close(S.combine(blocks[:ns], coeffs), sum(b @ c for b, c in zip(blocks[:ns], coeffs)))
            lam = rng.standard_normal(m)
            R, rn, kn = S.residuals(blocks[0], blocks[1], lam)
            want = np.where(free[:, None], blocks[0] - blocks[1] * lam[None, :], 0.0)
            close(R, want)
            close(rn, np.sqrt((want ** 2).sum(axis=0)))
            close(kn, np.sqrt((blocks[0][free] ** 2).sum(axis=0)))
            assert np.array_equal(S.gram(A, B), S.gram(A, B))           # fixed order: the same bits
            for precond in ('kron', 'jacobi', None):
                Z = S.apply_precond(blocks[2], precond)
                cols = (0, m - 1) if n > 100000 else range(m)          # (the single-vector reference is one call per column)
                for j in cols:
                    close(Z[:, j], P.apply_precond(blocks[2][:, j], precond=precond if precond else 'none'))
                assert np.all(Z[fixed] == 0.0)
    finally:
        S.close()
        P.close()

"""The block kernels of the multipatch eigen-solver alone, against numpy on the CSR matrices
``MP.assemble_system`` returns for stiffness and mass (tests/_mp_eig_cases.py: every (GW, MB, NM) instantiation of k_csr_spmm2,
one multipatch past the pass bound per group width), the block preconditioners, and Gram / combine / residuals over global dofs.

Tolerance 1e-12 relative to the largest entry of the result: the same sums as numpy's in another order (the bound
tests/test_eig_kernels_gpu.py uses)."""
import numpy as np
import pytest

import _mp_eig_cases as MC
import _mpsolve_model as M

pytestmark = pytest.mark.gpu

TOL = 1e-12
STIFF, MASS = 'inner(grad(u), grad(v)) * dx', 'u * v * dx'
_HOST = {}


def close(got, want):
    scale = np.abs(want).max()
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= TOL * (scale if scale > 0 else 1.0), np.abs(got - want).max() / scale


def host_matrices(case):
    """(K, M) of the case as ``MP.assemble_system`` returns them: assembled once per case and left unchanged."""
    if case.id not in _HOST:
        MP = case.build()
        try:
            _HOST[case.id] = (MP.assemble_system(STIFF, None)[0].tocsr(), MP.assemble_system(MASS, None)[0].tocsr())
        finally:
            MP.close()
    return _HOST[case.id]


def restricted(A, free, X):
    """R A R^T X on full-length blocks."""
    Xm = np.where(free[:, None], X, 0.0)
    return np.where(free[:, None], A @ Xm, 0.0)


def check_products(S, K, Mm, fixed, columns, seed):
    n = K.shape[0]
    free = np.ones(n, dtype=bool)
    free[fixed] = False
    rng = np.random.default_rng(seed)
    for m in columns:
        X = rng.standard_normal((n, m))                    # (not masked: the product masks its input)
        YK, YM = S.block_products(X)
        close(YK, restricted(K, free, X))
        close(YM, restricted(Mm, free, X))
        assert np.all(YK[fixed] == 0.0) and np.all(YM[fixed] == 0.0)
        YK1, YM1 = S.block_product(X, 'K'), S.block_product(X, 'M')     # the one-matrix forms
        close(YK1, restricted(K, free, X))
        close(YM1, restricted(Mm, free, X))
        assert np.all(YK1[fixed] == 0.0) and np.all(YM1[fixed] == 0.0)


@pytest.mark.parametrize('mask', MC.MASKS)
@pytest.mark.parametrize('case', MC.SMALL_CASES, ids=lambda c: c.id)
def test_block_products_every_width_and_mask(case, mask):
    from pyiga_amd import solvers
    K, Mm = host_matrices(case.mp)
    MP = case.mp.build()
    fixed = MC.mask_dofs(MP, case.mp.domain, mask)
    try:
        S = solvers.MultipatchEigenSystem(MP, fixed, problem=MC.SHIFTED_FORM if mask == 'none' else None)
        assert S.n == K.shape[0] and np.array_equal(S.bc_indices, fixed)
        check_products(S, K + Mm if mask == 'none' else K, Mm, fixed, case.columns, len(mask))
    finally:
        MP.close()                                         # (destroys the solver as well)


@pytest.mark.parametrize('case', MC.WRAP_CASES, ids=lambda c: c.id)
def test_block_products_past_one_pass(case):
    from pyiga_amd import solvers
    K, Mm = host_matrices(case.mp)
    _HOST.pop(case.mp.id)                                  # (large: not kept)
    assert K.shape[0] > MC.spmm_pass_rows(case.mp.gw)
    MP = case.mp.build()
    fixed = MC.outer_dofs(MP, case.mp.domain)
    try:
        S = solvers.MultipatchEigenSystem(MP, (fixed, np.zeros(fixed.size)))
        check_products(S, K, Mm, fixed, case.columns, 5)
    finally:
        MP.close()


@pytest.mark.parametrize('m', [1, 5, 16])
def test_block_preconditioners(m, notebook16):
    """'mg': every column bit-identical to the V-cycle on that column alone, padding columns 0; Jacobi and None against numpy."""
    from pyiga_amd import _lib
    from pyiga_amd.operators import DeviceArray
    S, K, fixed = notebook16
    n = S.n
    free = np.ones(n, dtype=bool)
    free[fixed] = False
    R = np.random.default_rng(m).standard_normal((n, m))
    assert S.mg_info()[0]['free'] == n - fixed.size and len(S.mg_info()) == 3
    Z = S.apply_precond(R, 'mg')
    assert Z.shape == (n, m) and np.all(Z[fixed] == 0.0)
    for j in range(m):
        assert np.array_equal(Z[:, j], S.vcycle(R[:, j])), j
    mb = MC.eig_width(m)
    d_r, d_z = S._padded(R, mb), DeviceArray(S._ctx, n * mb)
    _lib.check(_lib.load().igx_solver_eig_precond_d(S.handle, mb, d_r.ptr, d_z.ptr), 'igx_solver_eig_precond_d')
    full = d_z.download().reshape(n, mb)
    assert np.array_equal(full[:, :m], Z) and np.all(full[:, m:] == 0.0)
    d = K.diagonal()
    close(S.apply_precond(R, 'jacobi'), np.where(free[:, None], R / d[:, None], 0.0))
    none = S.apply_precond(R, None)
    assert np.array_equal(none, np.where(free[:, None], R, 0.0))


@pytest.fixture(scope='module')
def notebook16():
    """The notebook domain at p = 3, n = 16 with a hierarchy of three levels: (system, K, fixed), made once."""
    from pyiga_amd import solvers
    MP = M.notebook(p=3, n=16)
    fixed = MC.outer_dofs(MP, 'notebook')
    S = solvers.MultipatchEigenSystem(MP, fixed)
    try:
        S.set_multigrid(levels=3)
        yield S, S.matrix(), fixed
    finally:
        S.close()
        MP.close()


def test_gram_combine_residuals_over_global_dofs():
    from pyiga_amd import solvers
    MP = MC.ROWS_CASE.build()
    n = MP.numdofs
    assert n % 256 != 0
    fixed = MC.outer_dofs(MP, 'notebook')
    free = np.ones(n, dtype=bool)
    free[fixed] = False
    rng = np.random.default_rng(n)
    try:
        S = solvers.MultipatchEigenSystem(MP, fixed)
        for m in MC.ROWS_COLUMNS:
            blocks = [rng.standard_normal((n, m)) for _ in range(6)]
            for na, nb in ((1, 1), (2, 3), (3, 3)):
                A, B = blocks[:na], blocks[3:3 + nb]
                close(S.gram(A, B), np.hstack(A)[free].T @ np.hstack(B)[free])
            assert np.array_equal(S.gram(A, B), S.gram(A, B))           # fixed order: the same bits
            for ns in (1, 2, 3):
                coeffs = [rng.standard_normal((m, m)) for _ in range(ns)]
                close(S.combine(blocks[:ns], coeffs), sum(b @ c for b, c in zip(blocks[:ns], coeffs)))
            lam = rng.standard_normal(m)
            R, rn, kn = S.residuals(blocks[0], blocks[1], lam)
            want = np.where(free[:, None], blocks[0] - blocks[1] * lam[None, :], 0.0)
            close(R, want)
            close(rn, np.sqrt((want ** 2).sum(axis=0)))
            close(kn, np.sqrt((blocks[0][free] ** 2).sum(axis=0)))
    finally:
        MP.close()

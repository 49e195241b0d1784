"""The block kernels of the vector-valued eigen-solver alone (solvers.VectorEigenSystem), against numpy on
the blocked CSR matrix the device assembles for the same form (``assemble(..., layout='blocked')``) and
``block_diag([mass] * nc)``: every (GW, MB, NM, NC) instantiation of k_block_spmm2 and a grid-stride wrap per group width
(tests/_veceig_cases.py), the three preconditioners column by column against VectorFormSystem, and the shared block kernels on
the longer vectors.

Tolerance 1e-12 relative to the largest entry of the result: the same sums as numpy's in another order (the bound
tests/test_eig_kernels_gpu.py uses)."""
import numpy as np
import pytest
import scipy.sparse

import _eig_cases as EC
import _eig_model as EM
import _veceig_cases as VC
from test_eig_kernels_gpu import close, geo_for, restricted

pytestmark = pytest.mark.gpu


def host_matrices(form, kvs, geo, nc):
    from pyiga_amd import assemble
    K = assemble.assemble(form, kvs, geo=geo, bfuns=VC.bfuns(nc), layout='blocked').tocsr()
    M = scipy.sparse.block_diag([assemble.mass(kvs, geo)] * nc, format='csr')
    return K, M


def masks(ndofs, nc):
    """The fixed dofs (blocked numbering) of the three masks: whole sides in every component, different sides per component,
    and scattered dofs with a row that is fixed in component 0 only."""
    d, N = len(ndofs), int(np.prod(ndofs))
    idx = np.arange(N).reshape(ndofs)
    sides = EM.boundary_dofs(ndofs)
    per = []
    for c, (ax, last) in enumerate(((0, False), (d - 1, True), (0, True))[:nc]):     # a side of its own per component
        per.append(np.take(idx, ndofs[ax] - 1 if last else 0, axis=ax).ravel() + c * N)
    rng = np.random.default_rng(N + nc)
    scat = rng.choice(nc * N, size=max(1, nc * N // 5), replace=False)
    row = N // 2
    scat = np.union1d(scat[(scat % N) != row], [row])            # row N // 2: fixed in component 0, free in the others
    return {'sides': np.concatenate([sides + c * N for c in range(nc)]), 'per_component': np.sort(np.concatenate(per)),
            'scattered': np.sort(scat)}


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
        close(S.block_product(X, 'K'), restricted(K, free, X))     # the one-matrix forms
        close(S.block_product(X, 'M'), restricted(M, free, X))
    YK2, YM2 = S.block_products(X)
    assert np.array_equal(YK, YK2) and np.array_equal(YM, YM2)     # fixed order: the same bits
    assert np.array_equal(S.block_product(X, 'K'), S.block_product(X, 'K'))


@pytest.mark.parametrize('case', VC.SMALL_CASES, ids=lambda c: c.id)
def test_block_products_every_width_mask_and_form(case):
    from pyiga_amd import solvers
    kvs, geo, nc = case.patch.kvs(), geo_for(case.patch.dim), case.nc
    ndofs = tuple(kv.numdofs for kv in kvs)
    for form in (VC.FULL[nc], VC.LAPLACE):
        K, M = host_matrices(form, kvs, geo, nc)
        for name, fixed in masks(ndofs, nc).items():
            S = solvers.VectorEigenSystem(form, kvs, fixed, bfuns=VC.bfuns(nc), geo=geo)
            try:
                assert all(all(r) for r in S.present) == (form != VC.LAPLACE)
                assert all(S.present[c][c] for c in range(nc))
                check_products(S, K, M, fixed, case.columns, len(name))
            finally:
                S.close()


def test_scattered_mask_has_a_row_fixed_in_one_component_only():
    for nc in VC.NCS:
        ndofs = (10, 8)
        N = 80
        fixed = masks(ndofs, nc)['scattered']
        row = N // 2
        assert row in fixed and all(c * N + row not in fixed for c in range(1, nc))


@pytest.mark.parametrize('case', VC.WRAP_CASES, ids=lambda c: c.id)
def test_block_products_past_one_pass(case):
    from pyiga_amd import solvers
    kvs, geo, nc = case.patch.kvs(), geo_for(case.patch.dim), case.nc
    form = VC.PAIR[nc]
    K, M = host_matrices(form, kvs, geo, nc)
    ndofs = tuple(kv.numdofs for kv in kvs)
    N = int(np.prod(ndofs))
    assert N > VC.spmm_pass_rows(case.patch.gw) and K.shape[0] == nc * N
    fixed = masks(ndofs, nc)['sides']
    S = solvers.VectorEigenSystem(form, kvs, fixed, bfuns=VC.bfuns(nc), geo=geo)
    try:
        check_products(S, K, M, fixed, case.columns, 5)
    finally:
        S.close()


@pytest.mark.parametrize('case', EC.ROWS_CASES, ids=lambda c: c.id)
def test_preconditioners_and_shared_kernels_on_blocked_vectors(case):
    """The three preconditioners column by column against VectorFormSystem.apply_precond on the same patch and fixed dofs (two
    components with different boxes), and gram, combine and residuals once on vectors of nc N rows."""
    from pyiga_amd import geometry, solvers
    kvs, geo, nc = case.kvs(), geometry.unit_square(), 2
    ndofs = tuple(kv.numdofs for kv in kvs)
    N = int(np.prod(ndofs))
    n = nc * N
    assert N == case.rows()
    idx = np.arange(N).reshape(ndofs)
    # component 0: every side; component 1: the two sides of axis 0 only
    fixed = np.sort(np.concatenate([EM.boundary_dofs(ndofs), np.concatenate([idx[0], idx[-1]]) + N]))
    free = np.ones(n, dtype=bool)
    free[fixed] = False
    rng = np.random.default_rng(n)
    form = VC.FULL[nc]
    S = solvers.VectorEigenSystem(form, kvs, fixed, bfuns=VC.bfuns(nc), geo=geo)
    P = solvers.VectorFormSystem(form, kvs, 0.0, (fixed, np.zeros(fixed.size)), bfuns=VC.bfuns(nc), geo=geo)
    try:
        assert S.default_precond == 'kron' and S.boxes[0] != S.boxes[1]
        for i, m in enumerate(case.columns):
            blocks = [rng.standard_normal((n, m)) for _ in range(6)]
            for precond in ('kron', 'jacobi', None):
                Z = S.apply_precond(blocks[2], precond)
                cols = (0, m - 1) if n > 100000 else range(m)          # (the single-vector reference is one call per column)
                for j in cols:
                    close(Z[:, j], P.apply_precond(blocks[2][:, j], precond=precond if precond else 'none'))
                assert np.all(Z[fixed] == 0.0)
            if i:
                continue
            A, B = blocks[:2], blocks[3:6]
            close(S.gram(A, B), np.hstack(A)[free].T @ np.hstack(B)[free])
            assert np.array_equal(S.gram(A, B), S.gram(A, B))           # fixed order: the same bits
            coeffs = [rng.standard_normal((m, m)) for _ in range(3)]
            close(S.combine(blocks[:3], coeffs), sum(b @ c for b, c in zip(blocks[:3], coeffs)))
            lam = rng.standard_normal(m)
            R, rn, kn = S.residuals(blocks[0], blocks[1], lam)
            want = np.where(free[:, None], blocks[0] - blocks[1] * lam[None, :], 0.0)
            close(R, want)
            close(rn, np.sqrt((want ** 2).sum(axis=0)))
            close(kn, np.sqrt((blocks[0][free] ** 2).sum(axis=0)))
    finally:
        S.close()
        P.close()

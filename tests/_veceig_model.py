"""Host model of the vector-valued eigen-solver (solvers.VectorEigenSystem): the controller
``solvers.lobpcg_loop`` runs on ``_eig_model.NumpyOps`` with the blocked K and ``I (x) M``, preconditioned by the block-diagonal
Kronecker model below.  A plain helper module (no GPU needed): tests/test_veceig_cpu.py runs it on the golden matrices,
tests/test_veceig_gpu.py compares the device solve with it.
"""
import numpy as np
import scipy.sparse

import _eig_model as EM


def golden_csr(g, name):
    return scipy.sparse.csr_matrix((g[name + '_data'], g[name + '_indices'], g[name + '_indptr']), shape=tuple(g[name + '_shape']))


def block_mass(M1, nc):
    return scipy.sparse.block_diag([M1] * nc, format='csr')


def block_kron_precond(factors, ndofs):
    """diag(P_0, .., P_{nc-1}) on blocked blocks of shape ``(nc * N, m)``: P_c the fast-diagonalization inverse of
    ``_eig_model.kron_precond`` on the free box of component c.  `factors`: per component ``(lo, hi, U, lam, mode)`` as
    ``kron_factors()`` of the device systems gives them (mode: the sum of the lam_k)."""
    N = int(np.prod(ndofs))
    parts = []
    for lo, hi, U, lam, mode in factors:
        assert mode == 1
        parts.append(EM.kron_precond(U, lam, (lo, hi), ndofs))

    def apply(R):
        return np.vstack([P(R[c * N:(c + 1) * N]) for c, P in enumerate(parts)])
    return apply


def component_factors(kvs, fixed, nc, mats1d=None):
    """``kron_factors()`` without a device: the boxes of the fixed dofs per component and their factors (no floating component).
    `mats1d`: as ``solvers.fastdiag_factors`` takes it (the oracle's 1D matrices where there is no device)."""
    from pyiga_amd import solvers
    ndofs = tuple(kv.numdofs for kv in kvs)
    N = int(np.prod(ndofs))
    fixed = np.asarray(fixed, dtype=np.int64)
    out = []
    for c in range(nc):
        box = solvers.dirichlet_box(ndofs, fixed[(fixed >= c * N) & (fixed < (c + 1) * N)] - c * N)
        assert box is not None and any(a > 0 for a in box[0])
        out.append(box + tuple(solvers.fastdiag_factors(kvs, box[0], box[1], True, mats1d=mats1d)))
    return out


def annulus2_kvs():
    from pyiga_amd import bspline
    return (bspline.make_knots(3, 0.0, 1.0, 10),) * 2


def run_model(g, k, block, seed, factors, tol=1e-9, maxiter=200):
    """The controller on the golden `annulus2` matrices with the Kronecker `factors` of its two components:
    ``(lam, info, X0)``."""
    from pyiga_amd import solvers
    ndofs = tuple(kv.numdofs for kv in annulus2_kvs())
    K, M = golden_csr(g, 'annulus2_K'), block_mass(golden_csr(g, 'annulus2_M1'), 2)
    fixed = g['annulus2_fixed']
    X0 = EM.start_block(K.shape[0], block, seed)
    ops = EM.NumpyOps(K, M, fixed, X0, block_kron_precond(factors, ndofs))
    lam, info = solvers.lobpcg_loop(ops, block, k, tol, maxiter)
    return lam, info, X0

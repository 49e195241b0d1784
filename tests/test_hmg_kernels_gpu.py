"""The two stateless kernels of the local multigrid on seeded synthetic CSR matrices: ``igx_csr_rap_d`` (C = P^T A P on a given
pattern) and ``igx_csr_rect_spmv_d`` against long-double sums (tests/_hmg_model.py).

Bound: 1e-12 relative to the largest entry (`rel_maxdiff`).  The entries here are uniform in [-1, 1]; an
output entry has at most 25 x 25 terms of magnitude at most 1, so double rounding stays below 625 x 2^-53 = 7e-14 of the
largest term -- the bound leaves a factor of ten.  Two runs and a grid capped at two blocks must give identical bits."""
import numpy as np
import pytest
import scipy.sparse

import _hier_cases as hc
import _hmg_model as mm

from pyiga_amd import _lib, solvers

pytestmark = pytest.mark.gpu

RTOL = 1e-12


def rand_csr(rng, nrows, ncols, row_lengths):
    """CSR with the given number of entries per row at random ascending columns, values uniform in [-1, 1] (never 0)."""
    indptr = np.concatenate(([0], np.cumsum(row_lengths))).astype(np.int32)
    indices = np.concatenate([np.sort(rng.choice(ncols, size=int(m), replace=False)) for m in row_lengths] + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    data = rng.uniform(0.1, 1.0, indices.size) * rng.choice([-1.0, 1.0], indices.size)
    return scipy.sparse.csr_matrix((data, indices, indptr), shape=(nrows, ncols))


def rap_device(A, PT, pat, max_blocks=None):
    """The device values of PT A PT^T on the pattern `pat` (a CSR matrix whose values are ignored)."""
    ctx = _lib.context(None)
    buf, d_cv = solvers.csr_rap_device(ctx, A, PT, (pat.indptr, pat.indices), max_blocks=max_blocks)
    try:
        vals = np.empty(pat.nnz)
        _lib.check(_lib.load().igx_dev_download(ctx.handle, vals.ctypes.data, d_cv, vals.nbytes), 'igx_dev_download')
    finally:
        buf.free()
    return vals


def check_rap(A, P, pattern=None):
    """Device against long double on the structural pattern (or `pattern`); run to run and capped grid bit for bit."""
    pat = mm.structural_pattern(A, P) if pattern is None else mm.csr(pattern)
    PT = mm.csr(P.T)
    ref = mm.rap_longdouble(A, P, pat)
    got = rap_device(A, PT, pat)
    err = abs(got - ref.data).max() / abs(ref.data).max()
    print('rap %s -> %s, %d values, longest P^T row %d: %.2e' % (A.shape, ref.shape, pat.nnz, np.diff(PT.indptr).max(), err))
    assert err <= RTOL
    assert np.array_equal(got, rap_device(A, PT, pat)), 'two runs differ'
    # two blocks: with the narrowest lane group a pass covers 128 values, so every case with more values wraps the grid
    assert np.array_equal(got, rap_device(A, PT, pat, max_blocks=2)), 'the capped grid differs'
    return scipy.sparse.csr_matrix((got, pat.indices, pat.indptr), shape=pat.shape), ref


def test_rap_single_coarse_dof():
    rng = np.random.default_rng(1)
    A = rand_csr(rng, 40, 40, rng.integers(1, 9, 40))             # non-symmetric
    P = rand_csr(rng, 40, 1, np.ones(40, dtype=int))              # n_c = 1: P^T has one row of 40 entries (lane group 64)
    C, ref = check_rap(A, P)
    assert C.shape == (1, 1)


def test_rap_identity_block_empty_rows_nonsymmetric():
    """P = [I 0; 0 R] with some rows of R empty (THB truncation produces them), A non-symmetric, more values than one pass."""
    rng = np.random.default_rng(2)
    nk, nr, ncr = 150, 60, 20
    lengths = rng.integers(0, 4, nr)
    lengths[:5] = 0
    R = rand_csr(rng, nr, ncr, lengths)
    P = scipy.sparse.bmat(((scipy.sparse.identity(nk), None), (None, R)), format='csr')
    A = rand_csr(rng, nk + nr, nk + nr, rng.integers(3, 12, nk + nr))
    assert abs(A - A.T).max() > 0.1
    C, ref = check_rap(A, P)
    assert C.nnz > 2 * 64 * 4                                     # (more than two blocks of 4-lane groups hold at once)
    # the identity block copies the values of A bit for bit
    sub = A[:nk][:, :nk]
    assert abs(C[:nk][:, :nk] - sub).max() == 0.0


def test_rap_long_output_rows_and_wide_columns():
    """Output rows of 70 and 300 entries (longer than a lane group, longer than a block), a P^T row with one entry and one with
    (p + 2)^d = 25 entries for p = 3, d = 2."""
    rng = np.random.default_rng(3)
    nf, nc = 360, 330
    # rows 0 and 1 of A hold the columns 0 .. 299 and 0 .. 69, which P keeps one to one: C has rows of exactly 300 and 70 entries
    top = scipy.sparse.csr_matrix((rng.uniform(0.1, 1.0, 370), np.concatenate((np.arange(300), np.arange(70))), [0, 300, 370]), shape=(2, nf))
    A = scipy.sparse.vstack((top, rand_csr(rng, nf - 2, nf, rng.integers(2, 7, nf - 2))), format='csr')
    # P: coarse dof j < nc - 1 keeps fine dof j (one entry per column); the last coarse dof has 25 children among the rest
    rows = np.concatenate((np.arange(nc - 1), nc - 1 + np.arange(25)))
    cols = np.concatenate((np.arange(nc - 1), np.full(25, nc - 1)))
    P = scipy.sparse.csr_matrix((rng.uniform(0.1, 1.0, rows.size), (rows, cols)), shape=(nf, nc))
    PT = mm.csr(P.T)
    assert np.diff(PT.indptr).min() == 1 and np.diff(PT.indptr).max() == 25
    C, ref = check_rap(A, P)
    assert np.diff(C.indptr)[0] == 300 and np.diff(C.indptr)[1] == 70


def test_rap_position_without_terms_is_zero():
    """A position of the pattern that no term reaches is written as exactly 0.0 (the buffer is not cleared beforehand)."""
    rng = np.random.default_rng(4)
    A = rand_csr(rng, 30, 30, np.full(30, 3))
    P = rand_csr(rng, 30, 12, np.ones(30, dtype=int))
    S = mm.structural_pattern(A, P)
    full = scipy.sparse.csr_matrix(np.ones((12, 12)))
    assert full.nnz > S.nnz
    C, ref = check_rap(A, P, pattern=full)
    extra = (full - S).toarray() > 0
    assert extra.any() and np.all(C.toarray()[extra] == 0.0) and not np.any(np.signbit(C.toarray()[extra]))
    assert C.nnz == 144


def test_rap_index_outside_yields_nan():
    """An index outside its array makes the entries it belongs to NaN; nothing is read there and the other entries are right."""
    rng = np.random.default_rng(5)
    A = rand_csr(rng, 30, 30, np.full(30, 3))
    P = rand_csr(rng, 30, 12, np.ones(30, dtype=int))
    pat = mm.structural_pattern(A, P)
    PT = mm.csr(P.T)
    ref = mm.rap_longdouble(A, P, pat).toarray()
    bad = PT.copy()
    k = bad.indptr[4]                                             # the first entry of row 4 of P^T points one past the fine dofs
    assert bad.indptr[5] > k
    bad.indices[k] = 30
    got = scipy.sparse.csr_matrix((rap_device(A, bad, pat), pat.indices, pat.indptr), shape=pat.shape).toarray()
    touched = np.zeros((12, 12), dtype=bool)
    touched[4, :] = touched[:, 4] = True
    touched &= pat.toarray() > 0
    assert np.isnan(got[touched]).all() and not np.isnan(got[~touched]).any()
    assert abs(got[~touched] - ref[~touched]).max() <= RTOL * abs(ref).max()
    # a column of the pattern of C outside the matrix
    badpat = pat.copy()
    badpat.indices[0] = 12
    vals = rap_device(A, PT, badpat)
    assert np.isnan(vals[0]) and not np.isnan(vals[1:]).any()


@pytest.mark.parametrize('row_max', [3, 30, 60, 100, 300])
def test_rect_spmv(row_max):
    """y = M x and y += M x at every group width of the row kernel (longest row 3 .. 300), with empty rows, rows of one entry,
    more rows than a grid of two blocks covers in one pass."""
    rng = np.random.default_rng(10 + row_max)
    nrows, ncols = 700, 320
    lengths = rng.integers(0, min(row_max, 6) + 1, nrows)
    lengths[[0, 5, 699]] = row_max
    lengths[[1, 2]] = 0
    lengths[3] = 1
    if row_max >= 100:
        lengths[7] = 70
    M = rand_csr(rng, nrows, ncols, lengths)
    x, y0 = rng.uniform(-1, 1, ncols), rng.uniform(-1, 1, nrows)
    ref, ref_acc = mm.spmv_longdouble(M, x), mm.spmv_longdouble(M, x, y0)
    got, got_acc = solvers.csr_rect_spmv(M, x), solvers.csr_rect_spmv(M, x, y=y0)
    err, err_acc = abs(got - ref).max() / abs(ref).max(), abs(got_acc - ref_acc).max() / abs(ref_acc).max()
    print('rect spmv, longest row %d: %.2e, accumulating %.2e' % (row_max, err, err_acc))
    assert err <= RTOL and err_acc <= RTOL
    assert np.all(got[[1, 2]] == 0.0) and np.array_equal(got_acc[[1, 2]], y0[[1, 2]])
    assert np.array_equal(got, solvers.csr_rect_spmv(M, x)) and np.array_equal(got, solvers.csr_rect_spmv(M, x, max_blocks=2))
    assert np.array_equal(got_acc, solvers.csr_rect_spmv(M, x, y=y0, max_blocks=2))


def test_rect_spmv_column_outside_yields_nan():
    rng = np.random.default_rng(20)
    M = rand_csr(rng, 50, 20, np.full(50, 4))
    x = rng.uniform(-1, 1, 20)
    bad = M.copy()
    bad.indices[bad.indptr[9]] = 20
    got = solvers.csr_rect_spmv(bad, x)
    ref = mm.spmv_longdouble(M, x)
    keep = np.arange(50) != 9
    assert np.isnan(got[9]) and abs(got[keep] - ref[keep]).max() <= RTOL * abs(ref).max()


def test_transposed_products_of_a_prolongator():
    """P x_c and P^T r of a THB prolongator (tests/_hier_cases.py 'thb2inf') through the rectangular product."""
    from _hmg_fixtures import problem
    _, f, Ps, _ = problem('thb2inf')
    P = mm.csr(Ps[-1])
    xc = np.random.default_rng(30).uniform(-1, 1, P.shape[1])
    assert hc.rel_maxdiff(solvers.csr_rect_spmv(P, xc), mm.spmv_longdouble(P, xc)) <= RTOL
    assert hc.rel_maxdiff(solvers.csr_rect_spmv(mm.csr(P.T), f), mm.spmv_longdouble(mm.csr(P.T), f)) <= RTOL

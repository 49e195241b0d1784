"""Every instantiation and launch edge of the entry-wise and pattern kernels (csrc/kern_entries.hip: k_entries_list,
k_entries_wave, k_entries_csr, k_pattern, k_box_pairs) against a long-double sum: the cases of tests/_entries_cases.py, which
tests/test_entries_coverage_cpu.py ties to the source.

Reference (tests/_entries_model.py): one entry summed in long double from the patch's own quadrature fields
(``DevicePatch.fields``) and the per-axis basis tables at the patch's Gauss nodes (``bspline.active_deriv`` -- the kernel that
fills the resident tables -- and ``bspline.findspans``), so that only the entry kernels are under test.  Acceptance, entry by
entry:  |dev - ref| <= (npts + C_KIND) 2**-53 mag,  mag the same sum over absolute values, npts the Gauss points of the support
intersection, C_KIND the roundings of one point's term counted from entry_value (see the model).  No measured factor: the bound
holds for every summation order.  Pairs with disjoint supports or an index at or past prod(N) give exactly 0.0; pairs whose
intersection leaves the resident slab or box give NaN, and no other pair does.  Every test prints which kernel ran (from the
restated dispatch rule) and the largest |dev - ref| / bound.
"""
import numpy as np
import pytest
import scipy.sparse

from pyiga_amd import _lib, assemblers, bspline, geometry

import _entries_cases as ec
import _entries_model as em

pytestmark = pytest.mark.gpu

LD = np.longdouble


@pytest.fixture(autouse=True)
def _wide_long_double():
    assert np.finfo(np.longdouble).eps < 2e-19


def _geo(case):
    if case.geo == 'annulus':
        return geometry.quarter_annulus()
    if case.geo == 'twisted':
        return geometry.twisted_box()
    return geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.quarter_annulus())


def _patch(case, monkeypatch=None, thread=False, whole=False):
    """The patch of a case; thread: created under IGX_ENTRIES=thread (the choice is read when a patch is created); whole: without
    the row slab."""
    if thread:
        monkeypatch.setenv('IGX_ENTRIES', 'thread')
    try:
        return assemblers.DevicePatch(case.kvs(), _geo(case), row0=None if whole else case.row0, bbox=case.bbox, nqp=case.nqp)
    finally:
        if thread:
            monkeypatch.delenv('IGX_ENTRIES')


def _all_nodes(patch, k):
    """The Gauss nodes of the whole axis k (DevicePatch.gauss cuts them to the box of a boxed patch)."""
    nodes = np.empty(patch.info.ngauss[k])
    _lib.check(_lib.load().igx_patch_gauss(patch.handle, k, _lib.dptr(nodes), None), 'igx_patch_gauss')
    return nodes


def _tables(case, patch):
    kvs, q = case.kvs(), case.q()
    assert patch.nqp == q
    derivs = []
    for k, kv in enumerate(kvs):
        nodes = _all_nodes(patch, k)
        assert np.array_equal(nodes, em.gauss_nodes(kv, q))
        derivs.append(bspline.active_deriv(kv, nodes, 1))
    ax = em.tables_from_active_deriv(kvs, q, derivs)
    for k, (kv, a) in enumerate(zip(kvs, ax)):           # first active function of every Gauss node = that of its span
        first = bspline.findspans(kv, _all_nodes(patch, k)) - kv.p
        assert np.array_equal(first, np.repeat(a.fa, q))
    return ax


def _set_kind(case, patch, kind):
    """Give the patch what `kind` needs; returns the kind name of the library."""
    nodes = [patch.gauss(k)[0] for k in range(case.dim)]          # the resident grid (the box of a boxed patch)
    if kind == 'convdiff':
        patch.set_coeff(2.0 + ec.coef_array(0, 0, nodes))
    elif kind == 'form_phys':
        patch.set_form(ec.phys_table(case.dim, nodes))
    elif kind == 'form_par':
        patch.set_pform(ec.par_terms(case.dim, nodes))
    return ec.model_kind(kind)


def _fields(case, patch, mk, w):
    F = patch.fields(mk)
    assert patch.gauss_slab() == (w.g0, w.G0)
    assert F.shape[1:] == ((w.G0, w.L1, w.L2) if case.dim == 3 else (w.G0, w.L1)), (F.shape, w)
    return F


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check_values(tag, dev, model, ck):
    """Classes and bounds, pair by pair; returns the largest ratio."""
    worst = 0.0
    for k, (d, e) in enumerate(zip(dev, model)):
        if e.cls == 'zero':
            assert d == 0.0 and not np.signbit(d), (tag, k, d)
        elif e.cls == 'nan':
            assert np.isnan(d), (tag, k, d)
        else:
            assert not np.isnan(d), (tag, k)
            err, b = abs(LD(d) - e.value), em.bound(e, ck)
            assert err <= b, (tag, k, float(d), float(e.value), float(err / b) if b else np.inf, e.npts, e.nbox)
            if b:
                worst = max(worst, float(err / b))
    return worst


@pytest.mark.parametrize('cid', [c.id for c in ec.CASES])
def test_entries_against_long_double(cid, monkeypatch):
    """entries(kind, idx) on a default patch and on an IGX_ENTRIES=thread patch: values, exact zeros and NaNs pair by pair; the
    tails M - 3, M - 2, 1 of the request; upload_pairs + entries_resident give the same bits."""
    case = ec.BY_ID[cid]
    idx = ec.picks(case)
    M = len(idx)
    patch, patch_t = _patch(case), _patch(case, monkeypatch, thread=True)
    try:
        ax, w = _tables(case, patch), case.window()
        for kind in case.kinds:
            mk = _set_kind(case, patch, kind)
            _set_kind(case, patch_t, kind)
            F = _fields(case, patch, mk, w)
            assert np.array_equal(_bits(F), _bits(_fields(case, patch_t, mk, w)))
            form = ec.form_of(case, kind)
            ck = em.c_kind(case.dim, mk, form)
            model = em.entries(ax, w, F, em.terms_of(case.dim, mk, form), idx)
            assert [e.cls for e in model] == [em.classify(case.tables(), w, I, J)[0] for I, J in idx]
            devs = []
            for thread, p in ((False, patch), (True, patch_t)):
                fam, inst = ec.entries_kernel(case, kind, thread, M)
                assert fam == ('list' if thread else fam)
                dev = p.entries(mk, idx)
                worst = _check_values((cid, kind, fam), dev, model, ck)
                print('%s %s %s: %s, M = %d, max |dev - ref| / bound = %.3f' % (cid, kind, 'thread patch' if thread else 'default patch',
                                                                               ec.kernel_name(fam, inst), M, worst))
                for m in ec.request_lengths(M)[1:]:
                    assert ec.entries_kernel(case, kind, thread, m) == (fam, inst)
                    assert np.array_equal(_bits(p.entries(mk, idx[:m])), _bits(dev[:m])), (cid, kind, fam, m)
                p.upload_pairs(idx)
                assert p.entries_resident(mk) is None
                assert np.array_equal(_bits(p.entries_resident(mk, to_host=True)), _bits(dev)), (cid, kind, fam)
                devs.append(dev)
            # the two copies of the slab / box / empty-support checks agree
            assert np.array_equal(np.isnan(devs[0]), np.isnan(devs[1])) and np.array_equal(devs[0] == 0.0, devs[1] == 0.0)
    finally:
        patch.close()
        patch_t.close()


def _lookup(indptr, indices, data, r, J):
    row = indices[indptr[r]:indptr[r + 1]]
    k = int(np.searchsorted(row, J))
    assert k < len(row) and row[k] == J, (r, J)
    return data[indptr[r] + k]


@pytest.mark.parametrize('cid', [c.id for c in ec.CASES if c.assemble])
def test_assemble_entrywise_against_long_double(cid, monkeypatch):
    """k_entries_csr through assemble(kind, algo='entrywise') with the values NaN-filled first: every value is written, the
    picked pattern entries of the owned rows lie within the bound, and for mass and stiffness A[i, j] and A[j, i] have equal
    bits (the mirror stores the value it computed); for a row slab the partner comes from the whole patch."""
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')
    case = ec.BY_ID[cid]
    patch = _patch(case)
    whole = _patch(case, whole=True) if case.row0 else None
    try:
        ax, w = _tables(case, patch), case.window()
        Ntot = patch.shape[0]
        lo, hi = patch.row_range
        indptr, indices = patch.pattern()
        idx = [(I, J) for I, J in ec.picks(case) if lo <= I < hi and J < Ntot and em.overlap(ax, I, J) is not None][:80]
        assert len(idx) >= 10, cid
        for kind in case.kinds:
            mk = _set_kind(case, patch, kind)
            data = patch.assemble(mk, algo='entrywise')
            assert data.shape == (patch.nnz,) and not np.isnan(data).any(), (cid, kind)
            F = _fields(case, patch, mk, w)
            form = ec.form_of(case, kind)
            model = em.entries(ax, w, F, em.terms_of(case.dim, mk, form), idx)
            assert all(e.cls == 'value' for e in model)
            dev = [_lookup(indptr, indices, data, I - lo, J) for I, J in idx]
            worst = _check_values((cid, kind, 'csr'), dev, model, em.c_kind(case.dim, mk, form))
            print('%s %s: k_entries_csr<%d, IGX_%s>, %d of %d values compared, max |dev - ref| / bound = %.3f'
                  % (cid, kind, case.dim, ec.KIND_ENUM[kind], len(idx), len(data), worst))
            if kind in ec.SYMMETRIC:
                A = scipy.sparse.csr_matrix((data, indices, indptr), shape=(hi - lo, Ntot))
                if whole is None:
                    full = A
                else:
                    _set_kind(case, whole, kind)
                    full = whole.csr(mk, algo='entrywise')
                    assert not np.isnan(full.data).any()
                T = full.T.tocsr()[lo:hi]
                T.sort_indices()
                assert np.array_equal(T.indptr, A.indptr) and np.array_equal(T.indices, A.indices)
                assert np.array_equal(_bits(T.data), _bits(A.data)), (cid, kind)
    finally:
        patch.close()
        if whole is not None:
            whole.close()


@pytest.mark.parametrize('cid', [c.id for c in ec.CASES if c.assemble])
def test_pattern_against_column_ranges(cid, oracle):
    """k_pattern: indptr and indices are those built on the host from the per-axis column ranges (and the oracle's pattern), with
    the closing indptr entry; rows far shorter than the longest (boundary rows, repeated knots, mixed degrees), row slabs."""
    case = ec.BY_ID[cid]
    patch = _patch(case)
    try:
        indptr, indices = patch.pattern()
        assert indptr.dtype == np.int32 and indices.dtype == np.int32
        ip, ind = em.pattern(case.tables(), case.row0)
        assert np.array_equal(indptr, ip) and np.array_equal(indices, ind), cid
        assert indptr[0] == 0 and indptr[-1] == patch.nnz == len(indices)
        if case.row0 is None:
            I, J = oracle.full_pattern([oracle.KnotVector(kv.kv, kv.p) for kv in case.kvs()])
            order = np.lexsort((J, I))
            assert np.array_equal(indices, J[order]) and np.array_equal(np.diff(indptr), np.bincount(I, minlength=patch.shape[0]))
    finally:
        patch.close()


@pytest.mark.parametrize('cid', ec.BOX_PAIR_CASES)
def test_box_pairs_feed_the_entries_kernel(cid):
    """k_box_pairs: fast_assemble with batch >= S0 * S1 fetches the whole 2D matrix as one box of the reordered tensor, the index
    pairs built on the device; the values are, bit for bit, entries() of the pattern pairs on the same patch.  Only single-box
    requests are reachable through the API today (PairBoxes.n == 1 in every caller): the walk over several boxes in
    k_box_pairs has no test."""
    case = ec.BY_ID[cid]
    patch = _patch(case)
    try:
        S = [int((a.jhi - a.jlo).sum()) for a in case.tables()]
        indptr, indices = patch.pattern()
        rows = np.repeat(np.arange(patch.shape[0]), np.diff(indptr))
        pairs = np.stack([rows, indices], axis=1)
        for kind in ('mass', 'stiffness'):
            A = patch.fast_assemble(kind, batch=S[0] * S[1])
            assert patch.aca_stats['requests'] == 1 and patch.aca_stats['entries'] == S[0] * S[1] == patch.nnz
            assert np.array_equal(A.indptr, indptr) and np.array_equal(A.indices, indices)
            assert np.array_equal(_bits(A.data), _bits(patch.entries(kind, pairs))), (cid, kind)
    finally:
        patch.close()


@pytest.mark.parametrize('axis', ec.HIGH_DEGREE_AXES)
def test_basis_tables_of_high_degree(axis, oracle):
    """k_basis_tables at p = 8 .. 15 (the NDU[16][16] recursion up to its last row): active_deriv with two derivatives at the
    p + 1 Gauss nodes per span against the long-double run of the same recursion (the oracle's active_deriv_single, restated
    with np.longdouble in the model).  Tolerance per derivative order: 4 times the deviation of the oracle's own double
    run from the long-double one at the same nodes, relative to the largest magnitude of that order (the device runs the same
    recursion in the same precision and may differ by contraction and ordering only).  Measured on the host, in units of
    2**-53, orders 0 / 1 / 2:
        (8, 3, 1): 8.2 / 8.6 / 8.9     (15, 2, 1): 3.5 / 3.4 / 3.4     (15, 1, 1): 3.4 / 3.4 / 2.3
        (11, 2, 2): 7.2 / 6.8 / 5.8    (13, 3, 1): 8.7 / 10.0 / 8.6
    (tests/_entries_cases.py ORACLE_TABLE_DEVIATION; test_entries_coverage_cpu.py measures them again).  Exact: findspans equals
    the oracle's; the values of each point sum to 1 within (p + 1) 2**-53."""
    p, n, m = axis
    kv = bspline.make_knots(p, 0.0, 1.0, n, mult=m)
    u = em.gauss_nodes(kv, p + 1)
    dev = bspline.active_deriv(kv, u, 2)
    ref = em.active_deriv_ld(kv, u, 2)
    got = em.table_deviation(dev, ref)
    print('basis tables %s: deviation %s x 2**-53, allowed %s' % (axis, ['%.2f' % g for g in got],
                                                                 [ec.TABLE_FACTOR * r for r in ec.ORACLE_TABLE_DEVIATION[axis]]))
    for g, rec in zip(got, ec.ORACLE_TABLE_DEVIATION[axis]):
        assert g <= ec.TABLE_FACTOR * rec, (axis, got)
    okv = oracle.KnotVector(kv.kv, p)
    assert np.array_equal(bspline.findspans(kv, u), [oracle.findspan(okv.kv, p, float(x)) for x in u])
    assert abs(dev[0].astype(LD).sum(axis=0) - 1).max() <= (p + 1) * em.U

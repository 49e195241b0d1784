"""The kernels of pyiga_amd/csrc/multipatch.hip and the cases that run them cannot drift apart (no GPU needed).

tests/_multipatch_cases.py restates the constants that decide a kernel's path (the wave, the LDS sort tile, the scan tile) and
builds the case table; tests/_multipatch_model.py is the host model; tests/test_multipatch_kernels_gpu.py runs the table on the
device.  Here: the constants against the source, the model against scipy's X S X^T, the list of situations the table must
reach (asserted from the model, case by case: a deleted case line fails), and deliberately wrong variants of the model's
stages, each of which must disagree with the model on some case -- so that a kernel with that defect would fail on the device.
"""
import numpy as np
import pytest

import _multipatch_cases as mc
import _multipatch_model as mm
import _solver_cases as sc


@pytest.fixture(scope='module')
def src():
    return mc.read_source()


def test_constants(src):
    assert mc.parse_constants(src) == mc.CONSTS
    assert mc.parse_scan_tile(src) == 'SCAN_BLOCK * SCAN_ITEMS'
    assert mc.SCAN_TILE == 1024 and mc.SCAN_CHUNK == 262144
    # the ladder stands at 2^k - 1, 2^k, 2^k + 1 from the wave up to the sort tile, and past twice the tile
    assert mc.WAVE == 2 ** 6 and mc.SORT_TILE == 2 ** 10
    for k in range(6, 11):
        assert {2 ** k - 1, 2 ** k, 2 ** k + 1} <= set(mc.LADDER_LENGTHS)
    assert 4 in mc.LADDER_LENGTHS and max(mc.LADDER_LENGTHS) > 2 * mc.SORT_TILE


def test_the_twelve_kernels(src):
    assert sorted(mc.parse_kernels(src)) == sorted(mc.KERNELS)
    assert 'k_sort_long<<<nlong, ' in src and 'if (L > SORT_TILE)' in src
    assert 'for (long long c0 = 0; c0 < nt; c0 += SCAN_BLOCK)' in src


def test_case_table():
    assert mc.CASE_IDS == (
        'ladder', 'all_dup', 'dup_free_multi', 'permuted_2d_p4', 'permuted_2d_p1', 'p5_3d_identity', 'p5_3d_permuted',
        'p5_3d_two_cubes', 'many_patches_middle', 'many_patches_last', 'scan_nglobal_1023', 'scan_nglobal_1024',
        'scan_nglobal_1025', 'scan_big', 'non_injective_mix')
    for cid in mc.CASE_IDS:
        c = mc.case(cid)
        for p, m in enumerate(c.l2g):
            assert m.dtype == np.int32 and m.size == c.ndofs(p) and 0 <= m.min() and m.max() < c.nglobal
        again = mc.BUILDERS[cid]()                               # deterministic
        assert all(np.array_equal(a, b) for a, b in zip(c.l2g, again.l2g)) and again.nglobal == c.nglobal


# ---------------------------------------------------------------------------------------------
# the model against scipy
SMALL = [cid for cid in mc.CASE_IDS if cid not in ('scan_big',) and not cid.startswith('p5_3d')]


@pytest.mark.parametrize('cid', SMALL)
def test_model_against_scipy(cid):
    """X S X^T with all-ones S is positive exactly on the pattern; with integer values every sum is exact, so the dense
    X A X^T equals the model's sums entry for entry."""
    M = mc.model(cid)
    ones = [np.ones(ix.size) for ix in M.lindices]
    D = M.dense(ones)
    r, c = np.nonzero(D)
    assert np.array_equal(np.bincount(r, minlength=M.G), np.diff(M.indptr))
    assert np.array_equal(c, M.indices)
    rows = np.repeat(np.arange(M.G), np.diff(M.indptr))
    # the raw length is the row sum of X S X^T (duplicates counted), the number of terms per position its entries
    assert np.array_equal(D.sum(axis=1), M.L)
    _, m, _ = M.sum_values_ld(ones)
    assert np.array_equal(D[rows, M.indices], m)
    vals = mc.values(cid, 'mat', integer=True)
    assert np.array_equal(M.dense(vals)[rows, M.indices], M.sum_values(vals))
    ld, _, sabs = M.sum_values_ld(vals)
    assert np.array_equal(ld.astype(np.float64), M.sum_values(vals)) and (sabs >= np.abs(ld)).all()
    # vectors: X b
    bs = mc.values(cid, 'vec', integer=True)
    ref = np.zeros(M.G)
    for m_, b in zip(M.l2g, bs):
        ref += np.bincount(m_, weights=b, minlength=M.G)
    assert np.array_equal(M.sum_vector(bs), ref)
    # contrib, injective
    assert np.array_equal(M.contrib, sum(np.bincount(m_, minlength=M.G) for m_ in M.l2g))
    assert M.injective == all(len(set(m_.tolist())) == m_.size for m_ in M.l2g)


def test_model_against_the_geometric_pattern():
    MP = sc.two_cubes(5, 6)
    S = sc.multipatch_pattern(MP)
    M = mc.model('p5_3d_two_cubes')
    assert np.array_equal(M.indptr, S.indptr) and np.array_equal(M.indices, S.indices)


def test_model_positions_and_classes():
    """The position of every local entry holds its (row, column); DIRECT rows are the rows whose positions are k + delta."""
    for cid in mc.CASE_IDS:
        M = mc.model(cid)
        grows = np.repeat(np.arange(M.G), np.diff(M.indptr))
        for p in range(M.np):
            assert np.array_equal(grows[M.pos[p]], M.grow[p]) and np.array_equal(M.indices[M.pos[p]], M.gcol[p])
            k = np.arange(M.lindices[p].size)
            contiguous = M.pos[p] == k + M.delta[p][M.lrows[p]]
            whole = np.bincount(M.lrows[p][~contiguous], minlength=M.l2g[p].size) == 0
            if M.injective:
                assert np.array_equal(M.cls[p] == mm.DIRECT, whole & (M.contrib[M.l2g[p]] == 1))
        assert sum(M.entries) == sum(ix.size for ix in M.lindices)


# ---------------------------------------------------------------------------------------------
# what the table reaches
def _sorted_rows(M):
    """Global rows that go through a sort: reached, and not left as they are."""
    return (M.L > 0) & ~M.as_is


def test_ladder_reaches_every_sort_size():
    M = mc.model('ladder')
    through_sort = set(M.L[_sorted_rows(M) & (M.contrib >= 1)].tolist())
    assert set(mc.LADDER_LENGTHS) <= through_sort
    short = [L for L in mc.LADDER_LENGTHS if L <= mc.SORT_TILE]
    # every padded size of the LDS sort from 4 to the tile
    assert {1 << int(L - 1).bit_length() for L in short} == {4} | {2 ** k for k in range(6, 11)}
    long_rows = _sorted_rows(M) & (M.L > mc.SORT_TILE)
    assert long_rows.sum() >= 2 and (M.L[long_rows] > 2 * mc.SORT_TILE).any() and (M.L[long_rows] == mc.SORT_TILE + 1).any()
    # rows with duplicates and rows of contrib == 1 among the sorted ones
    assert (M.ucnt[_sorted_rows(M)] < M.L[_sorted_rows(M)]).any()
    assert (_sorted_rows(M) & (M.contrib == 1)).any()
    # unreached rows: first, last and in the middle
    empty = np.flatnonzero(M.L == 0)
    assert empty[0] == 0 and empty[-1] == M.G - 1 and empty.size >= 3 and (M.contrib[empty] == 0).all()
    assert not M.injective and M.entries[mm.ATOMIC] == sum(M.entries) and M.zero_from == 0


def test_duplicate_extremes():
    M = mc.model('all_dup')
    assert M.G == 1 and M.L.tolist() == [16] and M.ucnt.tolist() == [1] and M.contrib.tolist() == [4] and M.nnz == 1
    # contrib > 1: every local row brings its diagonal, so contrib - 1 duplicates are the fewest a summed row can have
    M = mc.model('dup_free_multi')
    assert M.contrib[0] == 2 and M.L[0] == 18 and M.ucnt[0] == 17
    # duplicate-free rows through the sort: reached once, columns out of order
    for cid in ('permuted_2d_p4', 'permuted_2d_p1', 'p5_3d_permuted'):
        M = mc.model(cid)
        s = _sorted_rows(M)
        assert s.any() and (M.contrib[s] == 1).all() and np.array_equal(M.ucnt[s], M.L[s])


def test_permuted_2d():
    for cid, longest in (('permuted_2d_p4', 81), ('permuted_2d_p1', 9)):
        M = mc.model(cid)
        assert M.injective and M.np == 1 and M.G > M.l2g[0].size
        assert M.entries[mm.DIRECT] > 0 and M.entries[mm.STORE] > 0 and M.entries[mm.RMW] == 0 and M.entries[mm.ATOMIC] == 0
        assert (M.delta[0][M.cls[0] == mm.DIRECT] != 0).all()
        assert np.diff(M.lindptr[0]).max() == longest
        # unreached rows between reached ones: no tail of rows to clear, everything is cleared
        empty = np.flatnonzero(M.contrib == 0)
        assert empty.size and empty[0] < M.l2g[0].max() and M.zero_from == 0
    M = mc.model('permuted_2d_p4')
    lens = np.diff(M.lindptr[0])
    assert (lens[M.cls[0] == mm.DIRECT] > mc.WAVE).any() and (lens[M.cls[0] == mm.STORE] > mc.WAVE).any()


def test_long_rows():
    consts = mc.CONSTS
    M = mc.model('p5_3d_identity')
    assert M.l2g[0].size == 1331 and M.lindices[0].size == 753571
    assert ((M.L > mc.SORT_TILE) & M.as_is).sum() == 25 and M.as_is.all()
    assert mm.staged_pattern(M, consts)[3] == 0                                   # n_long stays 0
    assert np.array_equal(M.indptr, M.lindptr[0]) and np.array_equal(M.indices, M.lindices[0])
    assert M.entries == [753571, 0, 0, 0] and M.zero_from == M.nnz
    M = mc.model('p5_3d_permuted')
    long_rows = (M.L > mc.SORT_TILE) & ~M.as_is
    assert long_rows.sum() == 25 and (M.contrib[long_rows] == 1).all()
    assert mm.staged_pattern(M, consts)[3] == 25
    assert M.entries[mm.STORE] > 0.99 * 753571 and M.entries[mm.RMW] == 0
    M = mc.model('p5_3d_two_cubes')
    assert M.injective and M.G == 2 * 1331 - 121
    assert ((M.contrib == 2) & (M.L == 2 * 726) & (M.ucnt == 1331)).sum() == 1   # the middle of the interface
    assert ((M.contrib == 2) & (M.L > mc.SORT_TILE) & (M.ucnt < M.L)).sum() >= 2
    lens = [np.diff(ip) for ip in M.lindptr]
    for k in (mm.DIRECT, mm.STORE):                                               # long direct rows inside, long store rows
        assert any((ln[c == k] > mc.SORT_TILE).any() for ln, c in zip(lens, M.cls))        # next to the interface
    assert any((ln[c == mm.RMW] > mc.WAVE).any() for ln, c in zip(lens, M.cls))
    assert any((M.delta[p][M.cls[p] == mm.DIRECT] != 0).any() for p in range(2))
    assert 0 < M.zero_from < M.nnz
    assert mm.staged_pattern(M, consts)[3] >= 2


def test_many_patches():
    mid, last = mc.model('many_patches_middle'), mc.model('many_patches_last')
    for M in (mid, last):
        assert M.injective and M.np >= 8
        assert {2, 3} <= set(M.contrib.tolist()) and M.contrib.max() >= 8 and M.contrib.min() == 1
        assert all(k > 0 for k in (M.entries[mm.STORE], M.entries[mm.RMW])) and M.entries[mm.ATOMIC] == 0
        _, m, _ = M.sum_values_ld([np.ones(ix.size) for ix in M.lindices])
        assert m.max() >= 8 and {2, 3} <= set(m.tolist())                        # sums of two, three and eight or more terms
    summed = np.flatnonzero(mid.contrib > 1)
    assert summed[0] > 0 and summed[-1] < mid.G - 1 and mid.zero_from == 0 and mid.r0 is None
    assert last.r0 == last.G - 3 and 0 < last.zero_from < last.nnz


def test_scan_sizes():
    assert mc.model('all_dup').G == 1
    for G in (mc.SCAN_TILE - 1, mc.SCAN_TILE, mc.SCAN_TILE + 1):
        M = mc.model('scan_nglobal_%d' % G)
        assert M.G == G and M.contrib[0] == 1 and M.contrib[G - 1] == 1 and M.injective
        assert np.flatnonzero(M.contrib).size == 35
    M = mc.model('scan_big')
    n = M.l2g[0].size
    assert M.injective and n > mc.SCAN_CHUNK and M.G > n
    assert n == min(k * k for k in range(1, 1000) if k * k > mc.SCAN_CHUNK)       # the first square patch past one trip
    ndlen = np.where(M.cls[0] == mm.DIRECT, 0, np.diff(M.lindptr[0]))
    for x in (M.L, M.ucnt, ndlen):                                                # the three scans: every tile has input
        pad = np.zeros(-x.size % mc.SCAN_TILE, dtype=x.dtype)
        tiles = np.concatenate((x, pad)).reshape(-1, mc.SCAN_TILE).sum(axis=1)
        assert tiles.size > mc.SCAN_BLOCK and (tiles > 0).all()
    assert 2.3e6 < M.lindices[0].size < 2.5e6


def test_every_class_and_the_atomic_rows():
    total = np.zeros(4, dtype=np.int64)
    for cid in mc.CASE_IDS:
        total += mc.model(cid).entries
    assert (total > 0).all()
    M = mc.model('non_injective_mix')
    assert not M.injective and M.entries[mm.ATOMIC] == sum(M.entries) and M.zero_from == 0
    assert np.unique(M.l2g[0]).size == M.l2g[0].size and np.unique(M.l2g[1]).size == M.l2g[1].size - 2
    assert np.diff(M.lindptr[1]).max() > mc.WAVE                                  # an atomic row past one trip of the lane loop
    # two columns of one local row on one global column: within a row, a position met twice
    twice = False
    for i in range(M.l2g[1].size):
        q = M.pos[1][M.lindptr[1][i]:M.lindptr[1][i + 1]]
        twice |= np.unique(q).size < q.size
    assert twice
    # a row reached once whose columns do not decrease and are not all distinct
    i = 6 * 9 + 6
    g = M.gcol[1][M.lindptr[1][i]:M.lindptr[1][i + 1]]
    assert M.contrib[M.l2g[1][i]] == 1 and (np.diff(g) >= 0).all() and (np.diff(g) == 0).sum() == 1


# ---------------------------------------------------------------------------------------------
# wrong kernels, on the host: every mutant of a stage must disagree with the model on some case
def _scan_without_carry(x, chunk):
    e = np.concatenate(([0], np.cumsum(x, dtype=np.int64)))
    start = (np.arange(x.size + 1) // chunk) * chunk
    start[-1] = ((x.size - 1) // chunk) * chunk                  # the total is the carry of the last trip alone
    return e - e[start]


def _dedup_blind_at_chunk_start(s, wave):
    keep = np.ones(s.size, dtype=bool)
    keep[1:] = s[1:] != s[:-1]
    keep[::wave] = True
    return s[keep]


def _rank_sort_colliding(raw):
    dst = np.full(raw.size, -1, dtype=raw.dtype)                 # equal keys get one rank: the other slots keep what they held
    dst[np.searchsorted(np.sort(raw), raw)] = raw
    return dst


def _bitonic_padded_with_zero(raw):
    n = 1 << int(raw.size - 1).bit_length() if raw.size > 1 else 1
    return np.sort(np.concatenate((raw, np.zeros(n - raw.size, dtype=raw.dtype))))[:raw.size]


def _shortcut_accepting_equal(raw):
    return bool((raw[1:] >= raw[:-1]).all())


def _zero_row_without_tail_check(contrib):
    other = np.flatnonzero(contrib != 1)
    return int(other[0]) if other.size else int(contrib.size)


PATTERN_MUTANTS = {
    'scan_carry_dropped': dict(scan=_scan_without_carry),
    'dedup_blind_at_chunk_start': dict(dedup=_dedup_blind_at_chunk_start),
    'rank_sort_ties_collide': dict(sort_long=_rank_sort_colliding),
    'bitonic_pad_below_keys': dict(sort_short=_bitonic_padded_with_zero),
    'shortcut_accepts_equal_neighbours': dict(shortcut=_shortcut_accepting_equal),
    'zero_from_without_tail_check': dict(zero_row=_zero_row_without_tail_check),
}


def _agrees(M, built):
    gptr, indices, zero_from, _ = built
    return np.array_equal(gptr, M.indptr) and np.array_equal(indices, M.indices) and zero_from == M.zero_from


def test_staged_build_equals_the_model():
    for cid in mc.CASE_IDS:
        assert _agrees(mc.model(cid), mm.staged_pattern(mc.model(cid), mc.CONSTS, rows=mc.case(cid).rows)), cid


@pytest.mark.parametrize('name', sorted(PATTERN_MUTANTS))
def test_pattern_mutant_is_noticed(name):
    caught = [cid for cid in mc.CASE_IDS
              if not _agrees(mc.model(cid), mm.staged_pattern(mc.model(cid), mc.CONSTS, rows=mc.case(cid).rows, **PATTERN_MUTANTS[name]))]
    assert caught, name
    expected = {'scan_carry_dropped': 'scan_big', 'dedup_blind_at_chunk_start': 'ladder', 'rank_sort_ties_collide': 'p5_3d_two_cubes',
                'bitonic_pad_below_keys': 'ladder', 'shortcut_accepts_equal_neighbours': 'non_injective_mix',
                'zero_from_without_tail_check': 'many_patches_middle'}[name]
    assert expected in caught, (name, caught)


def test_value_mutants_are_noticed():
    """RMW written as a store loses every term but the last; a sum taken in another patch order differs in its last bits."""
    for cid in ('many_patches_middle', 'many_patches_last', 'p5_3d_two_cubes'):
        M = mc.model(cid)
        vals = mc.values(cid, 'mat')
        assert np.array_equal(mm.staged_values(M, vals), M.sum_values(vals))
        assert not np.array_equal(mm.staged_values(M, vals, rmw_adds=False), M.sum_values(vals))
    M = mc.model('many_patches_middle')
    vals = mc.values('many_patches_middle', 'mat')
    out = np.zeros(M.nnz)
    for p in reversed(range(M.np)):
        out[M.pos[p]] += vals[p]
    assert not np.array_equal(out, M.sum_values(vals))
    # residue of an earlier sum: without the zeroing of the summed rows the second sum differs
    first = M.sum_values(mc.values('many_patches_middle', 'mat', scale=1e6))
    stale = first.copy()
    for p in range(M.np):
        st = (M.cls[p] <= mm.STORE)[M.lrows[p]]
        stale[M.pos[p][st]] = vals[p][st]
        stale[M.pos[p][~st]] += vals[p][~st]
    assert not np.array_equal(stale, M.sum_values(vals))


def test_sum_bound_is_the_textbook_one():
    u = 2.0 ** -53
    b = mm.sum_bound(np.array([1, 2, 9]), np.array([1.0, 1.0, 1.0], dtype=np.longdouble))
    assert b[0] == 0
    assert abs(float(b[1]) - (u / (1 - u) + 2.0 ** -64)) < 1e-30 and abs(float(b[2]) - (8 * u / (1 - 8 * u) + 8 * 2.0 ** -64)) < 1e-30

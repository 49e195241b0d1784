"""The instantiations of k_bf2, k_mirror and k_mirror2 and the cases that run them cannot drift apart (no GPU needed).

The dispatch of pyiga_amd/csrc/fused.hip -- the `case` lines of launch_bf, the four `if` lines of launch_bf2_p, the two switches
of launch_mirror -- must describe the set of kernels the cases of tests/_bf2_cases.py reach (plus the named UNREACHABLE ones),
every case must restate to the key written in its table, and -- with the library's own launch arithmetic,
igx_fused_rows_per_tile and igx_fused_chunk_plan -- must have the tile, chunk and mirror-chunk counts it is there for.
tests/test_bf2_kernels_gpu.py assembles the cases on the device.  A new instantiation in fused.hip without a case or an
UNREACHABLE entry fails here."""
import collections
import os

import pytest

import _bf2_cases as b2
import _bf3_cases as bc
from conftest import ROOT


@pytest.fixture(scope='module')
def cdll():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(ROOT, 'pyiga_amd', 'libigx.so')):
        ge.build()
    import pyiga_amd
    return pyiga_amd._lib.load()


def test_dispatch_as_parsed():
    d = b2.parse_dispatch()
    assert d['P'] == {2, 3, 4, 5, 6}
    assert d['sets'] == {(1, 'MASS', 1), (4, 'STIFF3', 1), (4, 'STIFF3', 2), (4, 'STIFF2', 1)}
    assert d['masks'] == {'MASS': 0x0001, 'STIFF3': 0x135F, 'STIFF2': 0x1248}
    assert len(b2.compiled_bf2_keys(d)) == 20 and len(b2.compiled_mirror_keys(d)) == 8
    assert d['rcm1'] == b2.RCM1 and d['rcm2'] == b2.RCM2 and d['IB'] == 3
    # the masks are the slot sets of the forms (sumfact_plan: add_slot over form_terms)
    assert b2.bf_signature(b2.form_slots(3, 'mass')) == (1, 0x0001, 1) and b2.bf_signature(b2.form_slots(2, 'mass')) == (1, 0x0001, 1)
    assert b2.bf_signature(b2.form_slots(3, 'stiffness')) == (4, 0x135F, 1)
    assert b2.bf_signature(b2.form_slots(2, 'stiffness')) == (4, 0x1248, 1)
    assert b2.bf_signature(b2.form_slots(3, 'convdiff')) == (4, 0x135F, 2)           # (before the merge: three slots with two terms)
    assert b2.bf_signature(b2.form_slots(2, 'convdiff'))[1] == 0x125A                # no kernel: the 2D form takes the stage kernels
    pt = [(b2.JET_MASK[r], b2.JET_MASK[s]) for r, s, _ in b2.na2_pterms()]
    assert len(pt) == 12 and b2.bf_signature(b2.form_slots(2, 'pform', pt)) == (4, 0x135F, 2)


def test_a_new_instantiation_without_a_case_is_noticed():
    """The parser sees an added line of each dispatch (so the coverage test below fails for it)."""
    src = b2.read_source()
    more = src.replace('    case 6: return launch_bf2_p<6>(', '    case 6: return launch_bf2_p<6>(st, A, nb, ny, mask, na, pt->ctx->ncu);\n    case 7: return launch_bf2_p<7>(', 1)
    assert b2.parse_dispatch(more)['P'] == {2, 3, 4, 5, 6, 7}
    more = src.replace('    case 7: return launch_mirror2_k<7, 0>(', '    case 11: return launch_mirror2_k<11, 0>(st, M, AL.N);\n    case 7: return launch_mirror2_k<7, 0>(', 1)
    assert b2.parse_dispatch(more)['mirror2'] == {5: 0, 7: 0, 9: b2.parse_dispatch()['VAR'], 11: 0}
    more = src.replace('    case 11: return launch_mirror_k<11>(', '    case 11: return launch_mirror_k<11>(st, M, AL.N);\n    case 13: return launch_mirror_k<13>(', 1)
    assert 13 in b2.parse_dispatch(more)['mirror1']
    more = src.replace('    if (ny == 4 && mask == BF_MASK_STIFF2 && na == 1)',
                       '    if (ny == 4 && mask == BF_MASK_STIFF2 && na == 2) return launch_bf2_c<P, 4, BF_MASK_STIFF2, 2>(st, A, nblocks, ncu);\n'
                       '    if (ny == 4 && mask == BF_MASK_STIFF2 && na == 1)', 1)
    assert (4, 'STIFF2', 2) in b2.parse_dispatch(more)['sets']


def test_every_compiled_instantiation_has_a_case_or_a_reason():
    reached = {c.key for c in b2.BF2_CASES}
    compiled = b2.compiled_bf2_keys()
    assert all(isinstance(why, str) and len(why) > 20 for why in b2.UNREACHABLE.values())
    unreachable = {k for k in b2.UNREACHABLE if isinstance(k, b2.Key)}
    assert not (reached & unreachable)
    assert compiled == reached | unreachable, ('without a case', sorted(compiled - reached - unreachable), 'not compiled', sorted((reached | unreachable) - compiled))
    mreached = {c.mirror for c in b2.BF2_CASES if c.mirror}
    mcompiled = b2.compiled_mirror_keys()
    munreachable = {k for k in b2.UNREACHABLE if isinstance(k, b2.Mirror)}
    assert not (mreached & munreachable)
    assert mcompiled == mreached | munreachable, ('without a case', sorted(mcompiled - mreached - munreachable), 'not compiled', sorted((mreached | munreachable) - mcompiled))
    # the 2D patches are the only ones that run k_mirror<5>, <7>, <9> and the 2D stiffness mask; k_mirror<3>, <11> run in 2D and 3D
    by_dim = collections.defaultdict(set)
    for c in b2.BF2_CASES:
        by_dim[len(c.axes)].add(c.mirror)
        by_dim[len(c.axes), 'key'].add(c.key)
    assert {b2.Mirror('k_mirror', WW, None) for WW in (3, 5, 7, 9, 11)} <= by_dim[2]
    assert {b2.Mirror('k_mirror', 3, None), b2.Mirror('k_mirror', 11, None)} <= by_dim[3]
    assert {b2.Key(P, 'MASS', 1) for P in range(2, 7)} <= by_dim[2, 'key'] & by_dim[3, 'key']
    assert len({c.id for c in b2.BF2_CASES}) == len(b2.BF2_CASES)


@pytest.mark.parametrize('case', b2.BF2_CASES, ids=[c.id for c in b2.BF2_CASES])
def test_the_restated_route_is_the_key_in_the_table(case):
    route = b2.bf2_route(case.axes, case.kind, case.knobs, [(b2.JET_MASK[r], b2.JET_MASK[s]) for r, s, _ in case.pterms] if case.pterms else None)
    assert route is not None, case.id
    assert route.key == case.key and route.mirror == case.mirror, (case.id, route)
    assert route.geoA == (len(case.axes) == 3 and (case.kind != 'convdiff' or case.axes[0][0] >= 2))
    assert (case.mirror is not None) == (case.kind in ('mass', 'stiffness'))
    # unequal sizes per axis
    N = [bc.numdofs(a) for a in case.axes]
    assert len(set(N)) == len(N), (case.id, N)


def test_route_rules():
    """bf2_route on hand-picked patches: without the knobs k_bf3 (or the default 2D chain) takes the symmetric forms."""
    a3 = ((1, 2, 1), (2, 5, 1), (2, 6, 1))
    a2 = ((2, 5, 1), (2, 6, 1))
    assert b2.bf2_route(a3, 'mass', {}) is None and b2.bf2_route(a3, 'stiffness', {'IGX_PATH': 'fused'}) is None
    assert b2.bf2_route(a3, 'mass', {'IGX_BF': '2', 'IGX_PATH': 'unfused'}) is None
    assert b2.bf2_route(a3, 'mass', {'IGX_BF': '2'}) == b2.Route(b2.Key(3, 'MASS', 1), b2.Mirror('k_mirror2', 5, 0), True)
    assert b2.bf2_route(a2, 'stiffness', {'IGX_BF': '2'}) is None                      # 2D: on request only
    assert b2.bf2_route(a2, 'stiffness', {'IGX_PATH': 'fused'}) is None                # k_bf3
    assert b2.bf2_route(a2, 'stiffness', b2.KNOBS_2D) == b2.Route(b2.Key(3, 'STIFF2', 1), b2.Mirror('k_mirror', 5, None), False)
    assert b2.bf2_route(((2, 5, 1), (3, 6, 1)), 'mass', b2.KNOBS_2D) is None            # unequal degrees
    assert b2.bf2_route(((2, 5, 2), (2, 6, 1)), 'mass', b2.KNOBS_2D) is None            # repeated knots
    assert b2.bf2_route(((6, 5, 1), (6, 6, 1)), 'mass', b2.KNOBS_2D) is None            # P = 7
    assert b2.bf2_route(a3, 'convdiff', {}) is None                                     # k_bf3
    assert b2.bf2_route(a3, 'convdiff', {'IGX_BF': '2'}) == b2.Route(b2.Key(3, 'STIFF3', 1), None, False)
    assert b2.bf2_route(((2, 2, 1),) + a3[1:], 'convdiff', {'IGX_BF': '2'}) == b2.Route(b2.Key(3, 'STIFF3', 1), None, True)
    assert b2.bf2_route(a2, 'convdiff', b2.KNOBS_2D) is None
    nine = [(b2.JET_MASK[r], b2.JET_MASK[s]) for r in range(3) for s in range(3)]
    assert b2.bf2_route(a2, 'pform', {'IGX_PATH': 'fused'}, nine).key == b2.Key(3, 'STIFF3', 1)
    assert b2.bf2_route(a2, 'pform', {'IGX_PATH': 'fused'}, nine + nine[:1]).key == b2.Key(3, 'STIFF3', 2)
    assert b2.bf2_route(a2, 'pform', {'IGX_PATH': 'fused'}, nine + nine[:1] * 2) is None    # three arrays in a slot
    assert b2.bf2_route(a2, 'pform', {'IGX_PATH': 'fused'}, nine[:8]) is None               # not the full first-order set
    assert b2.bf2_route(a2, 'pform', {}, nine) is None


def test_tile_heights_come_from_the_library(cdll):
    d = b2.parse_dispatch()
    for (mk, na), rows in b2.RMAX.items():
        assert tuple(cdll.igx_fused_rows_per_tile(P, d['masks'][mk], na) for P in range(2, 7)) == rows, (mk, na)
    assert {(mk, na) for _, mk, na in d['sets']} == set(b2.RMAX)
    # no kernel: -1
    for P, mask, na in ((1, 1, 1), (7, 1, 1), (3, 0x1248, 2), (3, 1, 2), (3, 0x135F, 3), (3, 0x135E, 1), (3, 0, 1), (3, 0x1135F, 1), (3, 1, 0)):
        assert cdll.igx_fused_rows_per_tile(P, mask, na) == -1, (P, mask, na)
    import ctypes
    out = (ctypes.c_int * 5)()
    for args in ((0, 1, 8, 256, 2), (1, 0, 8, 256, 2), (1, 1, 0, 256, 2), (1, 1, 8, 0, 2), (1, 1, 8, 256, 1), (1, 1, 8, 256, 7), (1 << 20, 1 << 10, 8, 256, 2)):
        assert cdll.igx_fused_chunk_plan(*args, out) == 1, args             # IGX_ERR_ARG
    assert cdll.igx_fused_chunk_plan(1, 1, 8, 256, 2, None) == 1


@pytest.mark.parametrize('case', b2.BF2_CASES, ids=[c.id for c in b2.BF2_CASES])
def test_every_case_has_the_counts_it_is_there_for(cdll, case):
    d = b2.parse_dispatch()
    dim = len(case.axes)
    p = case.axes[-1][0]
    N = [bc.numdofs(a) for a in case.axes]
    want = dict(case.want)
    for slots in (b2.TAIL_SLOTS if want.get('tail') else b2.SLOTS):
        s = b2.launch_shape(cdll, case, slots)
        tag = (case.id, slots, s)
        if 'tiles' in want:
            assert s['ntiles'] == want['tiles'], tag
            if want['tiles'] > 1:                     # the height is rebalanced: below RMAX, the last tile not empty
                assert s['R2'] < s['rmax'] and (s['ntiles'] - 1) * s['R2'] < N[-1] <= s['ntiles'] * s['R2'], tag
        if want.get('full_tile'):
            assert N[-1] == s['rmax'] and s['R2'] == s['rmax'], tag
        if want.get('edge_rows'):
            assert N[-1] <= 2 * p, tag
        if want.get('chunked'):
            assert s['nmchunks'] > 1 and s['mid_rows'] >= 4 * (p + 1), tag
        if want.get('one_chunk'):
            assert case.axes[dim - 2][1] == 1 and s['nmchunks'] == 1 and s['tail_k'] == 0, tag
        if want.get('tail'):
            assert s['tail_k'] > 0 and s['nmchunks'] == 1 and 0 < s['main_blocks'] < s['npairs'] * s['ntiles'], tag
        if 'mchunks' in want:
            assert s['mchunks'] == want['mchunks'], tag
            if want['mchunks'] > 1:
                assert s['RC'] < s['RCM'], tag
        if want.get('full_mchunk'):
            assert N[-1] == s['RCM'] == s['RC'], tag
        if want.get('ni1'):
            assert s['mid_rows'] >= 16 and s['ni1'] >= 2, tag
        if case.mirror and case.mirror.kernel == 'k_mirror2':
            if want.get('ragged'):
                assert s['i1_rows'] % d['IB'] != 0, tag
            if want.get('exact'):
                assert s['i1_rows'] % d['IB'] == 0 and s['mid_rows'] % s['i1_rows'] == 0, tag
    if case.want.get('tail'):
        assert p == 1 and dim == 3 and set(b2.SLOTS) <= set(b2.TAIL_SLOTS)
        nnz = 1
        for n, a in zip(N, case.axes):
            nnz *= b2._pairs(n, a[0])
        assert nnz <= 10e6, nnz
    if case.slabs:
        N0 = N[0]
        assert case.slabs == (sorted({0, 1, N0 // 2, N0}) if dim == 3 else sorted({0, 1, p, N0 // 2, N0 - 1, N0})), case.id
        assert want.get('chunked')


def test_every_instantiation_meets_every_edge():
    """Per k_bf2 key: one, two and three tiles, a full tile, a patch of edge rows only, a chunked and a one-span swept axis;
    per mirror key: one full chunk and two chunks, a split of the rows; k_mirror2: whole and ragged groups of IB rows; one
    tail split; slabs for every degree in 2D and 3D; all five geometries."""
    by_key, by_mirror = collections.defaultdict(list), collections.defaultdict(list)
    for c in b2.BF2_CASES:
        by_key[c.key].append(c.want)
        if c.mirror:
            by_mirror[c.mirror].append(c.want)
    for key, wants in by_key.items():
        assert {w.get('tiles') for w in wants} >= {1, 2, 3}, key
        for flag in ('full_tile', 'edge_rows', 'chunked', 'one_chunk'):
            assert any(w.get(flag) for w in wants), (key, flag)
    for mirror, wants in by_mirror.items():
        assert {w.get('mchunks') for w in wants} >= {1, 2}, mirror
        assert any(w.get('full_mchunk') for w in wants) and any(w.get('ni1') for w in wants), mirror
        if mirror.kernel == 'k_mirror2':
            assert any(w.get('ragged') for w in wants) and any(w.get('exact') for w in wants), mirror
    assert sum(bool(c.want.get('tail')) for c in b2.BF2_CASES) == 1
    assert {(len(c.axes), c.axes[-1][0]) for c in b2.SLAB_CASES} == {(dim, p) for dim in (2, 3) for p in range(1, 6)}
    assert {c.geo for c in b2.BF2_CASES} == {'cylinder', 'twisted_box', 'quarter_annulus', 'bspline_quarter_annulus', 'unit_square'}
    # 3D: axis 0 of lower degree and axis 0 of one span occur for every degree that has a lower one
    for p in range(2, 6):
        c3 = [c for c in b2.EDGE_CASES if len(c.axes) == 3 and c.axes[-1][0] == p]
        assert any(c.axes[0][0] < p for c in c3) and any(c.axes[0][1] == 1 for c in c3), p


def _decode(bid, grid, plan, ntiles, mid_rows):
    """k_bf2 / k_bf3: block id -> (outer pair, tile, rows [rlo, rhi) of the mid axis), as the kernels decode it."""
    mrows, nmch, main, tk, tmr = plan
    tail = tk > 0 and bid >= main
    per = (main if tk > 0 else grid) // 8
    if bid < per * 8:
        bid = (bid % 8) * per + bid // 8
    if tail:
        t = bid - main
        mch, rows, bid = t % tk, tmr, main + t // tk
    else:
        mch, rows = (bid // ntiles) % nmch, mrows
    tile = bid % ntiles
    r0 = bid // (ntiles * (1 if tail else nmch))
    rlo = mch * rows
    return r0, tile, rlo, min(rlo + rows, mid_rows)


def test_chunk_plan_is_sound(cdll):
    """igx_fused_chunk_plan over a sweep of (npairs, ntiles, mid_rows, slots, P): whole blocks cover the rows of the mid axis
    once; with a tail split the first main_blocks blocks (whole rounds of the chip) walk the whole axis and the others tail_k
    chunks of tail_mrows rows, the last one clipped and not empty -- every (pair, tile, row) belongs to exactly one block of
    the launch, decoded as the kernel decodes it.  Includes mid_rows < 2 P (no chunks at all), per_chunk == slots and
    per_chunk == slots + 1."""
    ntail = nchunked = 0
    sweep = []
    for P in (2, 3, 5, 6):
        for slots in (1, 3, 8, 16, 24):
            for npairs, ntiles in ((1, 1), (1, 3), (slots, 1), (slots + 1, 1), (2 * slots + 1, 1), (slots // 2 + 1, 2), (slots, 3),
                                   (3 * slots + 2, 1), (5 * slots - 1, 1), (slots + 3, 2)):
                for mid_rows in (1, P, 2 * P - 1, 2 * P, 4 * P - 1, 4 * P, 4 * P + 1, 6 * P + 1, 11 * P + 2, 16 * 2 * P + 3, 70):
                    sweep.append((npairs, ntiles, mid_rows, slots, P))
    sweep += [(519, 2, 13, s, 2) for s in b2.SLOTS] + [(1537, 2, 8, s, 2) for s in b2.TAIL_SLOTS] + [(2600, 1, 136, 256, 5), (360, 1, 136, 256, 5), (256, 1, 40, 256, 4), (257, 1, 40, 256, 4)]
    for npairs, ntiles, mid_rows, slots, P in sweep:
        plan = b2.chunk_plan(cdll, npairs, ntiles, mid_rows, slots, P)
        mrows, nmch, main, tk, tmr = plan
        tag = (npairs, ntiles, mid_rows, slots, P, plan)
        per_chunk = npairs * ntiles
        mmax = max(1, min(16, mid_rows // (2 * P)))
        assert 1 <= nmch <= mmax and mrows >= 1, tag
        assert (nmch - 1) * mrows < mid_rows <= nmch * mrows, tag
        if mid_rows < 4 * P:
            assert nmch == 1 and tk == 0, tag
        if tk == 0:
            assert main == 0 and tmr == 0, tag
            grid = per_chunk * nmch
        else:
            assert nmch == 1 and mrows == mid_rows and per_chunk > slots, tag
            assert 2 <= tk <= mmax and 0 < main < per_chunk and main % slots == 0, tag
            assert (tk - 1) * tmr < mid_rows <= tk * tmr, tag
            grid = main + (per_chunk - main) * tk
            ntail += 1
        nchunked += nmch > 1
        seen = collections.Counter()
        for bid in range(grid):
            r0, tile, rlo, rhi = _decode(bid, grid, plan, ntiles, mid_rows)
            assert 0 <= r0 < npairs and 0 <= tile < ntiles and 0 <= rlo < rhi <= mid_rows, (tag, bid)
            for row in range(rlo, rhi):
                seen[r0, tile, row] += 1
        assert len(seen) == per_chunk * mid_rows and set(seen.values()) == {1}, tag
    assert ntail >= 20 and nchunked >= 20, (ntail, nchunked)

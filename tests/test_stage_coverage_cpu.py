"""The ledger of tests/_stage_cases.py against the sources of the stage chain (no GPU): the instantiations the launchers of
sumfact.hip / sumfact_stages.h / sumfact_hi.hip name are exactly the ones the cases and edge sweeps reach plus the ones shown
unreachable, the constants of the restatement are the sources', and the sweeps visit the sizes they claim."""
import collections

import pytest

import _stage_cases as st


@pytest.fixture(scope='module')
def dispatch():
    return st.parse_dispatch()


@pytest.fixture(scope='module')
def case_keys():
    return {c.id: st.stage_keys(c.axes, c.kind, c.knobs, c.table, c.geo) for c in st.STAGE_CASES}


@pytest.fixture(scope='module')
def sweep_keys():
    return [(tag, axes, st.stage_keys(axes, kind, knobs, table)) for tag, axes, kind, knobs, table in st.sweep_patches()]


def _instantiations(keys):
    return {k for k in (keys.stageA, keys.stageB, keys.final) if k is not None and k != 'geoA'}


def test_parsed_instantiations_are_the_reached_and_the_unreachable_ones(dispatch, case_keys, sweep_keys):
    parsed = dispatch['stageA'] | dispatch['stageB'] | dispatch['final']
    # 6 per P = 2 .. 6 and 3 per P = 7, 8; (P, P) and (P, 0), (P, 0) alone from P = 7; 8 per P and 2 per high P, 10, 12
    assert (len(dispatch['stageA']), len(dispatch['stageB']), len(dispatch['final'])) == (36, 12, 44 + 10 + 12)
    reached = set()
    for keys in list(case_keys.values()) + [k for _, _, k in sweep_keys]:
        assert keys is not None
        reached |= _instantiations(keys)
    assert not reached & st.UNREACHABLE_KEYS
    assert parsed - reached - st.UNREACHABLE_KEYS == set(), 'compiled, neither reached by a case nor shown unreachable'
    assert (reached | st.UNREACHABLE_KEYS) - parsed == set(), 'the ledger names an instantiation no launcher has'
    # the ledger alone reaches them all: the sweeps add sizes, not instantiations
    assert set().union(*(_instantiations(k) for k in case_keys.values())) == reached


def test_every_stage_b_body_is_reached(dispatch, case_keys):
    """NTERM = 1 .. 9 under a kernel with a compile-time q and under one with a run-time q, the 256-thread block included."""
    body = dispatch['stageB_body']
    assert [(label, n) for label, n, _ in body] == [(n, n) for n in range(1, 10)]          # `case n` runs body n; default: 9
    assert [ct for _, _, ct in body] == [n < st.BODY_RT_Q for n in range(1, 10)]
    bodies = set().union(*(st.body_keys(k) for k in case_keys.values()))
    assert bodies == {(n, ct) for n in range(1, 10) for ct in (True, False)}
    hi = {n for k in case_keys.values() if k.stageB is not None and k.stageB.P >= st.HI_P for _, n in k.nterm}
    assert hi >= {1, 4, 5, 7, 8, 9}
    assert any(k.combine for k in case_keys.values())
    # what gives which NTERM of the last-axis type 0
    for table, n in (('react', 1), ('conv', 2), ('react_conv', 3), ('diff', 4), ('diff_react', 5), ('diff_conv', 6),
                     ('diff_react_conv', 7), ('diff_conv2', 8), ('full', 9), ('full_sym', 9)):
        types = collections.Counter(t[2] for _, t in st.form_terms(3, 'form', table))
        assert types[0] == n, table
    assert sorted(collections.Counter(t[2] for _, t in st.form_terms(3, 'stiffness')).values()) == [1, 2, 2, 4]
    assert sorted(collections.Counter(t[2] for _, t in st.form_terms(3, 'convdiff')).values()) == [1, 2, 3, 6]
    assert sorted(collections.Counter(t[2] for _, t in st.form_terms(3, 'form', 'full')).values()) == [1, 3, 3, 9]


def test_constants_are_the_sources(dispatch):
    assert dispatch['const'] == st.MODULE_CONSTANTS
    assert dispatch['DISPATCH_P'] == list(range(st.DISPATCH_P[0], st.DISPATCH_P[1] + 1))
    assert dispatch['hi_threshold'] == {st.HI_P}
    assert all(v == list(range(st.HI_P, st.MAX_P + 1)) for v in dispatch['hi_P'].values())
    assert dispatch['kpy_split'] == [4]
    assert dispatch['LAUNCH_Q'] == [('case %d' % P, P) for P in range(2, st.FINALQ_MAX_P)] + [('default', st.FINALQ_MAX_P)]
    assert dispatch['LAUNCH_Q_NY'] == [1, 4]
    lo, hi = st.MFMA_NCH
    assert dispatch['LAUNCH_M'] == [('case %d' % n if n < hi else 'default', ny, n) for ny in (1, 4) for n in range(lo, hi + 1)]


def test_declared_keys(case_keys):
    ids = [c.id for c in st.STAGE_CASES]
    assert len(set(ids)) == len(ids) and len(ids) < 130
    for c in st.STAGE_CASES:
        k = case_keys[c.id]
        assert c.final is not None or c.stageA is not None or c.stageB is not None, c.id
        for want, got in ((c.stageA, k.stageA), (c.stageB, k.stageB), (c.final, k.final)):
            assert want is None or want == got, (c.id, want, got)
        assert c.geo in (st.GEOS_3D if len(c.axes) == 3 else st.GEOS_2D), c.id       # never the identity map
    # knot multiplicities: the mid axis, axis 0, two axes at once, an irregular pattern
    rep = [tuple(not st.axis_tables(a).simple for a in c.axes) for c in st.STAGE_CASES if len(c.axes) == 3]
    assert any(r == (False, True, False) for r in rep) and any(r[0] for r in rep) and any(sum(r) >= 2 for r in rep)
    assert any(isinstance(a[2], tuple) and len(set(a[2])) > 1 for c in st.STAGE_CASES for a in c.axes)
    # row slabs: every final-kernel family, every stage-A variant
    fam = {(k.final.kernel, k.final.args[-1] if k.final.kernel == 'k_final' else None) for k in case_keys.values()}
    slab = {(case_keys[c.id].final.kernel, case_keys[c.id].final.args[-1] if case_keys[c.id].final.kernel == 'k_final' else None)
            for c in st.STAGE_CASES if c.slabs}
    assert slab == fam == {('k_final', True), ('k_final', False), ('k_final_q', None), ('k_final_mfma', None)}
    var = lambda a: a if a == 'geoA' else a[1:] if a.Q == 0 else (1,) + a[2:]
    assert {var(case_keys[c.id].stageA) for c in st.STAGE_CASES if c.slabs} == {var(k.stageA) for k in case_keys.values()}


@pytest.mark.parametrize('entry', st.UNREACHABLE, ids=[str(u[0]) for u in st.UNREACHABLE])
def test_unreachable_derivations_hold(entry, dispatch):
    key, why, check = entry
    assert key in dispatch['stageA'] | dispatch['final'] and why
    assert check(), (key, why)


def test_mfma_cases_cover_every_nch(case_keys):
    got = {k.final.args for k in case_keys.values() if k.final.kernel == 'k_final_mfma'}
    assert got == {(ny, n) for ny in (1, 4) for n in range(1, 7)}
    # NCH = 7: the restatement says another kernel takes the patch
    over = [(c, case_keys[c.id]) for c in st.STAGE_CASES if c.knobs.get('IGX_FINAL') == 'mfma' and case_keys[c.id].final.kernel != 'k_final_mfma']
    assert over and all(k.shape['mfma_nch'] == 7 for _, k in over)


def test_edge_sweeps_visit_what_they_claim(sweep_keys):
    by = collections.defaultdict(list)
    for tag, axes, k in sweep_keys:
        by[tag[:2] if tag[0] != 'tiles' else ('tiles',)].append((tag, axes, k))
    # k_final rows per wave task: last-axis dofs crmax - 1 .. 2 crmax + 2, one kernel, one / two / three chunks, every edge position
    for name, fn, crmax in st.FINAL_ROW_SWEEPS:
        rows = by[('rows', name)]
        assert [st.axis_tables(axes[-1]).N for _, axes, _ in rows] == list(range(crmax - 1, 2 * crmax + 3))
        assert st.final_row_sizes(crmax, 0) + st.final_row_sizes(crmax, 1) == st.final_row_sizes(crmax)
        assert len({k.final for _, _, k in rows}) == 1 and all(k.shape['crmax'] == crmax and k.shape['ntiles'] == 1 for _, _, k in rows)
        assert {k.shape['chunks_per_tile'] for _, _, k in rows} == {1, 2, 3}
        two = [k.shape for _, _, k in rows if k.shape['chunks_per_tile'] == 2]
        assert {s['CR'] for s in two} == set(range(crmax // 2 + 1, crmax + 1))
    kinds = {name: by[('rows', name)][0][2].final.args for name, _, _ in st.FINAL_ROW_SWEEPS}
    assert kinds['fast-p2-2d'][2:] == (3, 4, True) and kinds['generic-p2-3d'][2:] == (0, 4, False)
    # k_final tiles
    tiles = [(st.axis_tables(axes[-1]).n, k.shape['ntiles']) for _, axes, k in by[('tiles',)]]
    assert [t for _, t in tiles] == [1, 1, 2, 2, 2, 3, 3]
    assert tiles[2][0] == tiles[1][0] + 1 and tiles[5][0] == tiles[4][0] + 1
    # k_final_q rows per wave
    for name, P, fn in st.FINALQ_SWEEPS:
        rows = by[('finalq', name)]
        R = 64 // P
        assert [st.axis_tables(axes[-1]).N for _, axes, _ in rows] == list(range(R - 1, 2 * R + 2))
        assert all(k.final.kernel == 'k_final_q' and k.final.args[0] == P for _, _, k in rows)
        assert {k.shape['q_nchunks'] for _, _, k in rows} == {1, 2, 3}
        assert {k.shape['q_last_rows'] for _, _, k in rows} == set(range(1, R + 1))
    assert sorted(P for _, P, _ in st.FINALQ_SWEEPS) == [2, 3, 6]
    for name, axes, kind, knobs, per_super in st.FINALQ_LPW_CASES:
        k = st.stage_keys(axes, kind, knobs)
        assert k.final.kernel == 'k_final_q' and k.shape['q_per_super'] == per_super and len(axes) == (2 if per_super else 3)
        assert k.shape['q_lpw'] >= st.FINALQ_MIN_LPW[1 if per_super else 0]
    # chunked sweeps: 1, 2, 2, 2, 3 chunks; never k_geoA on the swept axis 0
    variants = set()
    for name, which, fn, P, factor in st.CHUNK_SWEEPS:
        rows = by[('chunks', name)]
        assert [k.shape[which][0] for _, _, k in rows] == [1, 2, 2, 2, 3], name
        swept = 0 if which == 'chunksA' else 1
        assert all(st.axis_tables(axes[swept]).P == P for _, axes, _ in rows)
        assert [st.axis_tables(axes[swept]).n for _, axes, _ in rows] == st.chunk_sweep_sizes(P, factor)
        k = rows[0][2]
        assert which == 'chunksB' or k.stageA != 'geoA'
        assert (factor == 1) == (len(rows[0][1]) == 2 and which == 'chunksA')
        variants.add((which, len(rows[0][1]), k.stageA.SYM if which == 'chunksA' else len(k.nterm) > 1 and dict(k.nterm)[0] != 4,
                      not st.axis_tables(rows[0][1][swept]).simple))
    assert {v[:2] for v in variants} == {('chunksA', 3), ('chunksB', 3), ('chunksA', 2)}
    for which in ('chunksA', 'chunksB'):
        assert {v[2:] for v in variants if v[:2] == (which, 3)} == {(a, b) for a in (True, False) for b in (True, False)}, which
    assert any(k.stageA != 'geoA' and k.stageA.PF for tag, _, k in sweep_keys if tag[0] == 'chunks')


def test_sizes_stay_within_the_budget(case_keys):
    sizes = [st.patch_size(c.axes) for c in st.STAGE_CASES] + [st.patch_size(axes) for _, axes, _, _, _ in st.sweep_patches()]
    assert max(r for r, _ in sizes) <= st.MAX_ROWS and max(z for _, z in sizes) <= st.MAX_NNZ


def test_the_chain_refuses_what_its_limits_say():
    """The guards of run_mid and run_final, restated: a stage-B block of 128 threads stages at most 1024 coefficients per span."""
    with pytest.raises(st.Unsupported, match='stage B'):
        st.stage_keys(((7, 1, 1), (5, 2, 1), (1, 2, 1)), 'mass', st.UNF)
    assert st.stage_keys(((6, 1, 1), (5, 2, 1), (1, 2, 1)), 'mass', st.UNF).stageB == st.StageB(6, 0)
    assert st.stage_keys(((2, 3, 1),) * 3, 'stiffness') is None                       # the fused stage
    assert st.stage_keys(((2, 3, 1), (2, 3, 1), (2, 3, 2)), 'stiffness') is None      # the twin
    assert st.stage_keys(((2, 3, 1), (2, 3, 1), (2, 3, 2)), 'stiffness', st.UNF).final == st.Final('k_final', (3, 4, 0, 4, False))

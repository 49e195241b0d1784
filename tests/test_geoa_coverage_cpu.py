"""The instantiations of k_geoA and the cases that run them cannot drift apart (no GPU needed).

The dispatch of launch_geoA (pyiga_amd/csrc/geoa.hip: the GEOA_P / GEOA_T / GEOA_N / GEOA_2D case lists, the degree guards of
geoA_supported / geoA_form_supported, the p0g and nc branches, the matrix-core branch, GA_MASS8) must equal what
tests/_geoa_cases.py restates, and every (instantiation, form) a patch can reach must be the key of a case in GEOA_CASES, which
tests/test_gpu_parity.py::test_every_geoa_instantiation_vs_oracle assembles on the device.  A new case line, a deleted one or a
flipped GA_MASS8 fails here."""
import pytest

import _geoa_cases as gc


@pytest.fixture(scope='module')
def dispatch():
    return gc.parse_dispatch()


def test_dispatch_lists_equal_the_degree_guards(dispatch):
    """Every case line of the dispatch is a degree the guards admit, and every admitted degree has its case line."""
    d = dispatch
    rng = lambda lo_hi: list(range(lo_hi[0], lo_hi[1] + 1))
    assert d['guard_3d_P'] == gc.P_3D and d['GEOA_P'] == rng(gc.P_3D)
    assert d['guard_convdiff_min'] == gc.P_CONVDIFF_MIN and d['GEOA_N'] == list(range(gc.P_CONVDIFF_MIN, gc.P_3D[1] + 1))
    assert d['guard_form'] == gc.P_FORM + gc.P0G_RANGE
    assert d['GEOA_T_sym'] == [(P, 3) for P in rng(gc.P_FORM)] and d['GEOA_T_nonsym'] == [(P, 2) for P in rng(gc.P_FORM)]
    assert d['guard_2d'] == gc.P_2D + gc.P0G_RANGE and d['GEOA_2D'] == rng(gc.P_2D)
    assert d['guard_3d_p0g'] == gc.P0G_RANGE
    for k in ('p0g_g', 'p0g_GEOA_T', 'p0g_GEOA_N'):
        assert d[k] == rng(gc.P0G_RANGE), k
    assert d['ns_p0g_2d'] == [(ns, g) for ns in (1, 4) for g in rng(gc.P0G_RANGE)] and d['ns_2d_mass'] == [1]
    assert d['guard_2d_nslots'] == ('1', '4') and d['guard_3d_nslots'] == ('1', '8')
    assert d['nc_3d'] == list(gc.NC_3D) and d['nc_2d'] == list(gc.NC_2D)
    assert d['gspans_rule'] == [True, True, True]


def test_matrix_core_branch_and_mass8(dispatch):
    d = dispatch
    assert d['mf_P'] == list(gc.MF_P) and d['mf_p0g'] == [gc.MF_P0G] and d['mf_q_eq_P']
    assert d['mf_launch'] == [(P, 8, gc.MF_P0G) for P in gc.MF_P]
    assert d['GA_MASS8'] == gc.GA_MASS8 and d['mass8_maxp'] == gc.GA_MASS8_MAXP
    assert (d['ns_mass_one'], d['ns_default']) == (1, 8)
    assert d['GA_NFT'] == gc.NFT_NONSYM


def test_restated_constants_of_sumfact():
    """sweep_chunks (want = 2048 blocks, chunks of at least 4 P spans, none below 2 min_len), geoa2d_min_chunk (2 P) and the
    field / source / array limits of form_table_plan."""
    s = gc.parse_sumfact()
    assert s['want'] == gc.CHUNK_WANT == 2048
    assert s['min_len'] == gc.CHUNK_MIN_3D == 4 and s['too_short'] == 2
    assert s['min_2d'] == gc.CHUNK_MIN_2D == 2
    assert s['nft'] == (gc.NFT_SYM, gc.NFT_NONSYM) and s['max_src'] == 4 and s['max_arr'] == 8


def test_every_reachable_key_has_a_case():
    keys = gc.reachable_keys()
    covered = {(c.key, c.kind) for c in gc.GEOA_CASES if c.key is not None}
    assert keys - covered == set(), sorted(keys - covered)
    assert covered - keys == set(), sorted(covered - keys)
    # 3D FORM 0: 5 P x 2 P0G x 2 NC for stiffness and mass (NS = 1 at P = 6), the matrix-core sweep at P = 4, 5; 4 P x 4 for each
    # of FORM 1, 2, 3; 2D: 4 P x 2 NS x 2 P0G x 2 NC
    assert len(keys) == 20 + 20 + 4 + 3 * 16 + 32 == 124
    assert len({k for k, _ in keys}) == 108


def test_every_case_is_reachable_or_a_decision_edge():
    """A case outside the reachable table is a decision edge whose restated key is None: the geometry has one span more than
    2 * gspans <= G allows, degree 3 along axis 0, a non-symmetric table with more than 13 fields."""
    keys = gc.reachable_keys()
    for c in gc.GEOA_CASES:
        if c.key is None:
            assert c.edge, c.id
        else:
            assert (c.key, c.kind) in keys, c.id
    assert len(gc.EDGE_NONE) == 4
    edges = {c.id: c for c in gc.GEOA_CASES if c.edge}
    kept = [c for c in edges.values() if c.key is not None]
    assert len(kept) == 1 and 2 * gc.geo_gspans(kept[0].geo) == kept[0].axes[0][1] * (max(a[0] for a in kept[0].axes) + 1)
    assert any(c.geo.deg0 == 3 for c in edges.values() if c.key is None)
    assert any(c.table == 'nonsym_wide' for c in edges.values() if c.key is None)
    assert gc.form_table_fields(gc.TABLES['nonsym_wide'])[:2] == (False, False)
    assert gc.form_table_fields(gc.TABLES['nonsym_13'])[:3] == (True, False, 13)


def test_the_cases_hit_the_edges():
    """Short axes, axis 0 below nqp - 1, repeated knots on axis 0 up to a C^0 knot, the twin for every form with a NURBS map of
    degree 2 along axis 0, both convection-diffusion coefficients kinds, tables with constant / function / absent entries,
    stage-B / final patches (no k_bf3), slabs for every (P, P0G, NC, FORM, D2)."""
    cs = gc.GEOA_CASES
    p = lambda c: [a[0] for a in c.axes]
    assert any(any(gc.bc.numdofs(a) < 2 * a[0] + 1 for a in c.axes) for c in cs)
    assert any(p(c)[0] < max(p(c)) for c in cs)
    assert any(isinstance(c.axes[0][2], tuple) and max(c.axes[0][2]) == c.axes[0][0] >= 2 for c in cs)
    for kind in gc.FORM_OF:
        assert any(c.twin and c.kind == kind and c.geo.nurbs and c.geo.deg0 == 2 for c in cs), kind
    assert {c.coeff for c in cs if c.kind == 'convdiff'} == {'affine', 'expr', 'sampled'}
    assert any(c.key is not None and len(c.axes) == 3 and not c.bf3 for c in cs)
    slabs = {(c.key.P, c.key.P0G, c.key.NC, c.key.FORM, c.key.D2) for c in cs if c.slabs}
    assert slabs == {(c.key.P, c.key.P0G, c.key.NC, c.key.FORM, c.key.D2) for c in cs if c.key is not None}
    for c in cs:
        if len(c.axes) == 2:
            assert gc.single2d_excluded(c.axes), c.id


def test_chunk_sweeps_cover_the_chunk_counts_and_remainders():
    """The sizes of test_geoa_axis0_chunks give 1 .. 4 chunks and every remainder of the last chunk; the C^0 knot and the
    geometry knot sit within the P - 1 warm-up spans before a chunk start."""
    assert gc.sweep_chunks(2048, 100, 4) == (100, 1) and gc.sweep_chunks(1, 31, 4) == (31, 1)
    assert gc.sweep_chunks(1, 33, 4) == (17, 2) and gc.sweep_chunks(1000, 70, 4) == (24, 3)
    assert gc.sweep_chunks(1, 20, 3, 6) == (7, 3)
    for name, ml, p0, g, kind, extra in gc.CHUNK_SWEEPS:
        counts, rems = set(), set()
        for n0 in gc.chunk_sweep_sizes(ml, p0):
            a0, gk, length, nch = gc.chunk_axis0(ml, p0, n0)
            key = gc.geoa_key((a0,) + tuple(ml), gc.Geo(g[0], gk, g[1], 0), kind, gc.TABLES.get(extra))
            assert key is not None, (name, n0)
            counts.add(nch)
            rems.add((nch, n0 % nch))
            if nch > 1:
                first, last = length, (nch - 1) * length
                c0 = [k + 1 for k, m in enumerate(a0[2]) if m == p0]
                assert len(c0) == 1 and first - (p0 + 1) + 1 <= c0[0] < first, (name, n0)
                assert last - p0 <= gk[0] * n0 < last, (name, n0)
        assert counts == {1, 2, 3, 4}, name
        assert {r for n, r in rems if n == 4} == {0, 1, 2, 3} and {r for n, r in rems if n == 3} == {0, 1, 2}, name


def test_geoa_key_rules():
    """geoa_key on hand-picked patches."""
    K = gc.Key
    g1, g2n = gc.Geo(1, (0.41,), False, 0), gc.Geo(2, (0.41,), True, 0)
    assert gc.geoa_key(((5, 3, 1), (5, 2, 1), (5, 3, 1)), g1, 'mass') == K(6, 1, 2, 3, False, 0, False)
    assert gc.geoa_key(((4, 3, 1), (4, 2, 1), (4, 3, 1)), g1, 'mass') == K(5, 8, 2, 3, False, 0, False)
    assert gc.geoa_key(((3, 3, 1), (3, 2, 1), (3, 3, 1)), g1, 'stiffness', mfma=True) == K(4, 8, 2, 3, True, 0, False)
    assert gc.geoa_key(((3, 3, 1), (3, 2, 1), (3, 3, 1)), g2n, 'stiffness', mfma=True) == K(4, 8, 3, 4, False, 0, False)
    assert gc.geoa_key(((2, 3, 1), (3, 2, 1), (3, 3, 1)), g1, 'stiffness', mfma=True).MF is False       # q != P
    assert gc.geoa_key(((1, 3, 1), (1, 2, 1), (1, 3, 1)), g1, 'convdiff') is None                       # P < 3
    assert gc.geoa_key(((2, 3, 1), (2, 2, 1), (1, 3, 1)), g1, 'convdiff') is None                       # unequal mid / last
    assert gc.geoa_route(((2, 3, 1), (2, 2, 1), (2, 3, 2)), g2n, 'convdiff') == (K(3, 8, 3, 4, False, 1, False), True)
    assert gc.geoa_route(((2, 3, 1), (2, 2, 2), (2, 3, 2)), g1, 'stiffness') == (K(3, 8, 2, 3, False, 0, False), False)
    assert gc.geoa_key(((2, 3, 1), (2, 2, 2), (2, 3, 2)), g1, 'convdiff') is None                       # no fused stage
    assert gc.geoa_key(((2, 1, 1), (2, 2, 1), (2, 3, 1)), gc.Geo(1, (0.2, 0.5), False, 0), 'mass') is None   # 2 * 3 > 3
    assert gc.geoa_key(((1, 3, 1), (2, 2, 1), (2, 3, 1)), g1, 'form_nonsym', gc.TABLES['nonsym_conv']) is None   # P < 3
    assert gc.geoa_key(((3, 3, 1), (3, 2, 1), (2, 3, 1)), g1, 'form_nonsym', gc.TABLES['nonsym_conv']) is None   # unequal
    assert gc.geoa_key(((3, 3, 1), (3, 2, 1), (2, 3, 1)), g1, 'form_sym', gc.TABLES['sym_react']) == K(4, 8, 2, 3, False, 3, False)
    assert gc.geoa_key(((2, 12, 1), (2, 1200, 1)), g1, 'stiffness') == K(3, 4, 2, 2, False, 0, True)
    assert gc.geoa_key(((2, 12, 1), (2, 100, 1)), g1, 'stiffness') is None                              # the single launch

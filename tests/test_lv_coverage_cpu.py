"""The paths of the load-vector kernels and the cases that run them cannot drift apart (no GPU needed).

pyiga_amd/csrc/kern_vector.hip decides with lv12_shape whether k_lv12<WEIGHT, P, 5, NPASS> serves a 3D patch (and with which
chunks of the mid axis), else with last_axis_fast between k_contract_last (128 or 256 threads) and the generic k_contract_axis;
pyiga_amd/csrc/rtc.hip holds a second copy of k_lv12's text with the function inside.  tests/_lv_cases.py restates all of it and
lists the cases, tests/test_lv_kernels_gpu.py runs them.  A changed constant, condition, switch label or chunk rule, a dropped
case line, or a copy of the kernel whose window differs from the other fails here: the table must then be extended so that every
instantiation and every fall-back still runs under a test.  tests/_lv_model.py models the sliding window of k_lv12 on the host."""
import itertools

import numpy as np
import pytest

import _lv_cases as lc
import _lv_model as lm


@pytest.fixture(scope='module')
def vec_src():
    return lc.read(lc.KERN_VECTOR_HIP)


@pytest.fixture(scope='module')
def spl_src():
    return lc.read(lc.KERN_SPLINE_HIP)


@pytest.fixture(scope='module')
def rtc_src():
    return lc.read(lc.RTC_HIP)


def _gauss_nodes(kv, q):
    x, _ = np.polynomial.legendre.leggauss(q)
    m = np.asarray(kv.mesh, dtype=np.float64)
    return (0.5 * (m[1:] + m[:-1])[:, None] + 0.5 * (m[1:] - m[:-1])[:, None] * x[None, :]).ravel()


# ---------------------------------------------------------------------------------------------
# the source against the restatement
def test_constants(vec_src, spl_src):
    assert lc.parse_constants(vec_src, spl_src) == {'VEC_MAXSUP': lc.VEC_MAXSUP, 'LV_MAXPASS': lc.LV_MAXPASS, 'LV_WAVES': lc.LV_WAVES,
                                                    'SP_MAXWAVES': lc.SP_MAXWAVES}
    assert lc.VEC_MAXSUP == 36 and lc.LV_MAX_G2 == 128 * lc.LV_MAXPC and 64 * lc.LV_MAXPASS == 256


def test_lv12_shape_is_the_restated_condition(vec_src):
    """Every conjunct of the refusal, the LDS size and every statement of the chunk rule, as text: the literals 640, 64 KB, 8192
    and 8 are part of it."""
    assert sorted(lc.parse_lv12_conjuncts(vec_src)) == sorted(lc.LV12_CONJUNCTS)
    assert set(lc.LV12_CONJUNCTS.values()) - {'P'} == set(lc.REASONS) - {'2d'}
    body = lc.parse_lv12_statements(vec_src)
    assert 'if (pd.dim != 3) return false;' in body
    assert lc.LV12_LDS_EXPR in body
    at = -1
    for stmt in lc.LV12_CHUNK_RULE:                      # all there, in this order
        nxt = body.find(stmt, at + 1)
        assert nxt > at, stmt
        at = nxt
    # the numbers of the text are the numbers of the restatement
    assert '(8192 + G0 - 1)' in lc.LV12_CHUNK_RULE[1] and lc.LV_UNITS == 8192
    assert 'std::max(a1.P, 8)' in lc.LV12_CHUNK_RULE[1] and lc.LV_MIN_CHUNK == 8
    assert 'G0_loc' not in body            # the chunks of a row slab are those of the whole patch
    assert lc.LV_MAX_G2 == 640 and lc.LV_LDS_LIMIT == 64 * 1024


def test_last_axis_dispatch_is_the_restated_one(vec_src):
    assert lc.parse_last_axis_fast(vec_src) == lc.LAST_AXIS_FAST_EXPR
    assert lc.LAST_LDS_LIMIT == 48 * 1024
    assert lc.parse_tb_lpb(vec_src) == [(lc.LAST_TB_SPLIT, lc.LPB[3]), (lc.LAST_TB_SPLIT, lc.LPB[2])]


def test_lv12_switch(vec_src):
    labels, npasses, maxpc, npass_expr = lc.parse_lv12_switch(vec_src)
    assert tuple(labels) == lc.LV12_PS
    assert npasses == lc.LV12_NPASSES
    assert maxpc == (lc.LV_MAXPC, lc.LV_MAXPC)
    assert npass_expr == '(a2.N + 63) / 64'
    assert lc.parse_lv12_kernel_npc(vec_src) == ['(G2 / 2 + 63) >> 6']
    assert 'template <bool WEIGHT, int P, int MAXPC, int NPASS>' in vec_src
    # what the restatement makes of them
    assert [lc.npass_of(n) for n in (1, 64, 65, 128, 129, 192, 193, 256)] == [1, 1, 2, 2, 3, 3, 4, 4]
    assert [lc.npc_of(g) for g in (2, 128, 130, 256, 258, 384, 386, 512, 514, 640)] == [1, 1, 2, 2, 3, 3, 4, 4, 5, 5]


def test_generated_copy_is_selected_like_the_switch(vec_src, rtc_src):
    consts, npass_expr, ranges, body = lc.parse_rtc(rtc_src)
    assert consts == ('IGX_P', str(lc.LV_MAXPC), 'IGX_NPASS', str(lc.LV_WAVES))
    assert npass_expr == 'std::max(2, (a2.N + 63) / 64)'
    assert ranges == (lc.LV12_PS[0], lc.LV12_PS[-1], lc.LV12_NPASSES[0], lc.LV12_NPASSES[-1])
    assert lc.parse_lv12_kernel_npc(body) == ['(G2 / 2 + 63) >> 6']
    assert '"#define IGX_P " + std::to_string(P)' in rtc_src and '"\\n#define IGX_NPASS " + std::to_string(npass)' in rtc_src
    # the leaving-dof step (nleave, whole, store or add, the shift of the window) is the same text in both copies
    a = lc.kernel_window_text(vec_src, 'const int base = fa1[sp];', 'l = 0; ++sp;')
    b = lc.kernel_window_text(body, 'const int base = a1.fa[sp];', 'l = 0; ++sp;')
    assert a == b
    # and so are the chunk bounds and the table of the last axis
    for text in ('const int s_a = ch * chunk_spans, s_b = ch == nchunks - 1 ? a1.n : s_a + chunk_spans;',
                 'double *buf = lds + ((PQ * N2 + 1) & ~1) + wave * ((G2 + 1) & ~1);',
                 'for (int m = 0; m < PQ; ++m) r = fma(Vt[m * N2 + i2], bl[min(m, G2 - 1 - gfirst[k])], r);'):
        assert text in vec_src and text in body, text


def test_spline_launch_shape_is_the_restated_one(spl_src):
    limit, per_wave, lpw = lc.parse_spline(spl_src)
    assert limit == '64 * 1024' and lc.SP_LDS_LIMIT == 64 * 1024
    assert per_wave == '(size_t)(grad ? dim : 1) * Nlast * sizeof(double)'
    assert lpw == '(int)std::min<long long>(8, std::max<long long>(1, nlines / 16384))'
    assert 'for (int w = SP_MAXWAVES; w >= 1; w >>= 1)' in spl_src
    assert (lc.SP_MAX_LPW, lc.SP_LINES_PER_LPW) == (8, 16384)


# ---------------------------------------------------------------------------------------------
# the tables
def test_case_ids_are_unique():
    ids = [c.id for c in lc.ALL_CASES]
    assert len(set(ids)) == len(ids)
    assert set(lc.ADJOINT_CASES) <= set(ids)


def test_every_case_takes_the_path_it_claims():
    for c in lc.ALL_CASES:
        axes = c.tables()
        assert all(a.n == spec[1] for a, spec in zip(axes, c.axes)), (c.id, [a.n for a in axes])     # (make_knots gave n spans)
        assert lc.expected_path(axes) == c.path, (c.id, lc.expected_path(axes), lc.lv12_refusals(axes))
        if c.path == 'lv12':
            a2 = axes[2]
            clen, nch, lds = lc.lv12_shape(axes)
            assert (a2.P, lc.npass_of(a2.N), lc.npc_of(a2.G), a2.N, a2.G) == (c.P, c.npass, c.npc, c.N2, c.G2), c.id
            assert (clen, nch) == c.chunks, (c.id, clen, nch)
            assert lds <= lc.LV_LDS_LIMIT and c.npc <= lc.LV_MAXPC and c.npass <= lc.LV_MAXPASS
            # the second row slab of the GPU test starts past the first Gauss plane
            assert 0 < c.slab_cut() < axes[0].N and axes[0].mslo[c.slab_cut()] > 0
        else:
            assert c.reason in lc.lv12_refusals(axes), c.id
        assert int(np.prod([a.G for a in axes])) <= 400000, c.id          # a few hundred thousand Gauss points at the most


def test_instance_cases_reach_every_instantiation():
    """Every k_lv12<WEIGHT, P, 5, NPASS> the switch can launch has a case line with exactly that P and npass: the GPU test runs
    load_vector (WEIGHT = true), the jet functional (WEIGHT = false) and the generated copy on every line."""
    want = set(itertools.product(lc.LV12_PS, lc.LV12_NPASSES))
    got = {(c.P, max(2, c.npass)) for c in lc.INSTANCE_CASES}
    assert got == want, sorted(want - got)
    launched = set(itertools.product((True, False), lc.LV12_PS, lc.LV12_NPASSES))
    assert {(w, c.P, max(2, c.npass)) for w in (True, False) for c in lc.INSTANCE_CASES} == launched and len(launched) == 30
    assert {c.npc for c in lc.INSTANCE_CASES} == set(range(1, lc.LV_MAXPC + 1))
    assert any(c.npc > 1 and (c.G2 // 2) % 64 for c in lc.INSTANCE_CASES)         # a ragged last piece
    assert any(c.G2 == lc.LV_MAX_G2 for c in lc.INSTANCE_CASES)
    # the issue's smallest last axes
    small = {(2, 3): (129, 256), (2, 4): (193, 384), (3, 3): (130, 384), (3, 4): (194, 576), (4, 3): (129, 504), (4, 4): (193, 256),
             (5, 3): (130, 630), (5, 4): (193, 240), (6, 3): (131, 156), (6, 4): (196, 234)}
    for c in lc.INSTANCE_CASES:
        if c.id != 'c4_line' and c.npass > 2:
            assert small[(c.P, c.npass)] == (c.N2, c.G2), c.id
        assert c.axes[0][1] == 2 and c.P <= c.axes[1][1] <= 16
    assert {(c.P, c.npass) for c in lc.INSTANCE_CASES if c.npass > 2 and small[(c.P, c.npass)] == (c.N2, c.G2)} == set(small)
    c4 = lc.BY_ID['c4_line']
    assert (c4.axes[2][:3], c4.N2, c4.G2, c4.npass, c4.npc) == ((4, 128, 1), 132, 640, 3, 5)


def test_chunk_cases():
    by = lc.BY_ID
    for c in lc.CHUNK_CASES:
        assert c.chunks[1] >= 2, c.id
    assert {c.P for c in lc.CHUNK_CASES} == set(lc.LV12_PS)
    assert by['ch_P6_n65'].chunks == (9, 7) and lc.chunk_rule(65, 6, 12, merge=False) == (9, 8)      # the merge is what makes it 7
    # (P, n1) = (3, 67): eight chunks of 9 spans, the last of 4; at P = 4 the last chunk is exactly P spans long
    c = by['ch_P3_n67']
    assert (c.P, c.tables()[1].P, c.tables()[1].n, c.chunks) == (3, 3, 67, (9, 8))
    c = by['ch_P4_n67']
    assert (c.P, c.tables()[1].n, c.chunks) == (4, 67, (9, 8)) and 67 - 7 * 9 == c.P
    c = by['ch_P6_n65']
    assert (c.P, c.tables()[1].P, c.tables()[1].n) == (6, 6, 65)
    # one case with single knots per P
    assert {c.P for c in lc.CHUNK_CASES if all(a[2] == 1 and len(a) == 3 for a in c.axes) and c.npass == 1 and c.axes[0][1] == 2} == set(lc.LV12_PS)
    for cid, mult in (('ch_mult2', 2), ('ch_c0_p3', 3), ('ch_c0_p2', 2)):
        c = by[cid]
        assert c.axes[1][2] == mult and c.chunks[1] >= 4 and (mult == c.axes[1][0] or cid == 'ch_mult2')
    # the mixed case: only some interior knots are repeated, one on a chunk boundary, one a span away from one
    c = by['ch_mixed']
    rep = dict(c.axes[1][3])
    clen, nch = c.chunks
    bounds = {k * clen for k in range(1, nch)}
    assert len(rep) < c.axes[1][1] - 1 and bounds & set(rep) and any(m + 1 in bounds or m - 1 in bounds for m in rep)
    a1 = c.tables()[1]
    assert a1.N == 3 + 1 + 31 + sum(rep.values()) and a1.n == 32
    assert by['ch_np3'].npass == 3 and by['ch_np3'].chunks[1] >= 2
    # many planes: the 8192-wave branch of the rule decides.  With the planes of the slab in place of the whole axis' the second
    # slab of the GPU test (62 planes) would get 75 chunks: the case that failed before lv12_shape took the whole axis
    c = by['ch_g0cap']
    a0, a1, _ = c.tables()
    assert (lc.LV_UNITS + a0.G - 1) // a0.G < a1.n // max(a1.P, lc.LV_MIN_CHUNK)
    planes = a0.G - int(a0.mslo[c.slab_cut()]) * a0.q
    assert planes == 62 and lc.chunk_rule(a1.n, a1.P, planes) == (8, 75) != c.chunks


def test_fallback_cases_reach_every_reason_and_kernel():
    for reason in lc.REASONS:
        assert any(lc.lv12_refusals(c.tables()) == {reason} and c.reason == reason for c in lc.FALLBACK_CASES), reason
    seen = set()
    for c in lc.FALLBACK_CASES:
        axes = c.tables()
        ragged = lc.last_lines(axes) % lc.LPB[c.dim] != 0
        seen.add((c.dim, c.path, ragged))
    for dim in (2, 3):
        for path in ('last128', 'last256'):
            assert (dim, path, True) in seen, (dim, path)          # a last block shorter than LPB
        assert any(s[0] == dim and s[1] == 'generic' for s in seen)
    generic3 = {c.reason for c in lc.FALLBACK_CASES if c.dim == 3 and c.path == 'generic'}
    assert generic3 == {'N2>256', 'PQ>36'}
    assert any(c.nqp for c in lc.FALLBACK_CASES) and any(c.axes[0][0] == 6 and c.axes[2][0] == 5 for c in lc.FALLBACK_CASES)
    assert any(c.axes[-1][2] > 1 for c in lc.FALLBACK_CASES)                     # repeated knots on the last axis
    # the thresholds of the restated dispatch
    A = lc.Axis
    e = np.zeros(0, dtype=np.int64)
    assert lc.last_axis_fast(A(1, 2, 256, 255, 2, 510, e, e, e)) and not lc.last_axis_fast(A(1, 2, 257, 256, 2, 512, e, e, e))
    assert lc.last_axis_fast(A(5, 6, 9, 4, 6, 24, e, e, e)) and not lc.last_axis_fast(A(5, 6, 9, 4, 7, 28, e, e, e))
    assert lc.last_axis_fast(A(1, 2, 200, 199, 15, 3072, e, e, e)) and not lc.last_axis_fast(A(1, 2, 200, 199, 15, 3073, e, e, e))


def test_spline_cases():
    by = lc.SPLINE_BY_ID
    for c in lc.SPLINE_CASES:
        assert lc.spline12_waves(c.dim, c.grad, c.nlast()) == c.waves, c.id
        assert lc.spline_lpw(c.nlines()) == c.lpw, c.id
    assert by['3d_lines364'].nlines() == 364 * 364 and by['3d_lines364'].lpw == lc.SP_MAX_LPW
    assert lc.spline_lpw(182 * 182) == 2                      # the '3d_manylines' shape of test_spline_eval_gpu.py
    # 16562 units of 8 lines in blocks of 4 waves: the last block is ragged
    assert (by['3d_lines364'].nlines() // 8) % lc.SP_MAXWAVES != 0
    assert [by[k].nlast() for k in ('3d_last700', '3d_last1400', '3d_last2800', '2d_last1100')] == [700, 1400, 2800, 1100]
    assert {c.waves for c in lc.SPLINE_CASES} == {0, 1, 2, 4}
    assert lc.spline12_waves(3, False, 2800) == 2             # the refusal needs the gradient


# ---------------------------------------------------------------------------------------------
# the window of k_lv12 on the host
def test_collocation_ld_against_scipy():
    import scipy.interpolate
    for spec in ((3, 7, 1), (2, 5, 2), (4, 6, 4), (3, 32, 1, ((5, 2), (8, 2), (17, 1))), (1, 4, 1), (5, 6, 3)):
        kv = lc.make_kv(spec)
        x = _gauss_nodes(kv, kv.p + 1)
        C = lm.collocation_ld(kv, x)
        assert C.dtype == np.longdouble and C.shape == (2, x.size, kv.numdofs)
        B = scipy.interpolate.BSpline(np.asarray(kv.kv, dtype=float), np.eye(kv.numdofs), kv.p)
        assert abs(C[0] - B(x)).max() <= 1e-14 and abs(C[1] - B.derivative()(x)).max() <= 1e-12 * kv.numspans
        assert abs(C[0].sum(axis=1) - 1).max() <= 1e-18 and abs(C[1].sum(axis=1)).max() <= 1e-15 * kv.numspans
        t = lc.axis_tables(kv, kv.p + 1)
        nz = C[0] != 0
        for i in range(t.N):                                  # the supports are those of the axis tables
            g = np.flatnonzero(nz[:, i])
            assert g[0] == t.mslo[i] * t.q and g[-1] + 1 == t.mshi[i] * t.q


def test_contract_ld_is_the_dense_contraction():
    case = lc.BY_ID['fb_last_mult2']
    kvs, q = case.kvs(), case.q()
    Cs = [lm.collocation_ld(kv, _gauss_nodes(kv, q)) for kv in kvs]
    T = np.random.default_rng(3).uniform(-1.0, 1.0, tuple(C.shape[1] for C in Cs))
    for derivs in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        M = [C[d] for C, d in zip(Cs, derivs)]
        dense = np.einsum('ai,bj,ck,abc->ijk', *[m.astype(np.float64) for m in M], T)
        got = lm.contract_ld(Cs, q, T, derivs)
        assert got.dtype == np.longdouble and abs(got - dense).max() <= 1e-13 * abs(dense).max()
        B = lm.contract_ld(Cs, q, T, derivs, absolute=True)
        assert abs(B - np.einsum('ai,bj,ck,abc->ijk', *[abs(m).astype(np.float64) for m in M], abs(T))).max() <= 1e-13 * B.max()
        assert (abs(got) <= B).all()
    # a slab of Gauss planes of axis 0
    part = lm.contract_ld(Cs, q, T[q:], g0_lo=q) + lm.contract_ld(Cs, q, T[:q])
    assert abs(part - lm.contract_ld(Cs, q, T)).max() <= 1e-17


@pytest.mark.parametrize('cid', [c.id for c in lc.CHUNK_CASES] + ['P4_np2'])
def test_window_model_against_the_dense_contraction(cid):
    c = lc.BY_ID[cid]
    a1 = c.tables()[1]
    kv = c.kvs()[1]
    clen, nch = c.chunks
    lm.check_window(a1, clen, nch)
    C = lm.collocation_ld(kv, _gauss_nodes(kv, a1.q))
    V1 = np.zeros((a1.G, a1.P))
    for g in range(a1.G):
        V1[g] = C[0][g, a1.fa[g // a1.q]:a1.fa[g // a1.q] + a1.P].astype(np.float64)
    r = np.random.default_rng(5).uniform(-1.0, 1.0, a1.G)
    ref = (C[0].T.dot(r.astype(np.longdouble))).astype(np.float64)
    fwd = lm.apply_window(a1, clen, nch, V1, r)
    bwd = lm.apply_window(a1, clen, nch, V1, r, order=reversed(range(nch)))
    assert abs(fwd - ref).max() <= 1e-14 and abs(bwd - ref).max() <= 1e-14
    assert abs(fwd - bwd).max() <= 1e-15


def test_window_of_the_big_plane_count_case():
    c = lc.BY_ID['ch_g0cap']
    a0, a1, _ = c.tables()
    lm.check_window(a1, *c.chunks)
    for G0 in (a0.G, a0.G // 2, 2 * a0.q):
        lm.check_window(a1, *lc.chunk_rule(a1.n, a1.P, G0))


def test_window_exhaustively():
    """p = 1..5, every multiplicity, P <= n1 <= 80 spans, few and many Gauss planes: every dof of the mid axis receives its whole
    support exactly once, at most two chunks add to it, a stored dof is stored by one chunk."""
    ran = shared = 0
    for p in range(1, 6):
        for mult in range(1, p + 1):
            for n1 in range(p + 1, 81):
                a1 = lc.synthetic_axis(p, n1, mult, 2)
                for G0 in (6, 3000):
                    clen, nch = lc.chunk_rule(n1, p + 1, G0)
                    shared += lm.check_window(a1, clen, nch)
                    ran += nch > 1
    assert ran > 1000 and shared > 1000
    # the synthetic tables are those of the knot vectors
    for p, n1, mult in ((1, 9, 1), (3, 40, 3), (5, 65, 1), (4, 17, 2)):
        s, t = lc.synthetic_axis(p, n1, mult, 2), lc.axis_tables(lc.make_kv((p, n1, mult)), 2)
        assert s[:6] == t[:6] and all(np.array_equal(x, y) for x, y in zip(s[6:], t[6:]))


def test_window_model_notices_a_chunk_rule_without_the_merge():
    """The mutation the issue names: without `a short last chunk joins its neighbour` the rule leaves chunks shorter than P
    spans, which the kernel's two-addend argument excludes."""
    a1 = lc.synthetic_axis(5, 65, 1, 2)
    clen, nch = lc.chunk_rule(65, 6, 12, merge=False)
    with pytest.raises(AssertionError):
        lm.check_window(a1, clen, nch)
    # and a window that forgets the dofs still active at the end of a chunk loses them
    a1 = lc.synthetic_axis(3, 20, 1, 2)
    events = [e for e in lm.window_events(a1, 10, 2)]
    assert sum(1 for e in events if e[2] == 'add') == 2 * 3

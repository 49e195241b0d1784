"""The geometry-field kernels, k_grid_geo, k_coeff_affine and k_single2d (pyiga_amd/csrc/kern_basis.hip) and the cases that run
them cannot drift apart (no GPU needed).

What tests/_fields_cases.py restates -- geo_fields_plan, single2d_supported, single2d_plan, single2d_wanted -- must equal the
source constant by constant and line by line; the dispatch macros of launch_geo_fields must name exactly the listed
instantiations; every instantiation and every reachable tile shape of k_single2d must have a case in the tables that
tests/test_fields_kernels_gpu.py runs on the device; the restated NCOL must hold the control columns every tile touches; and
every named mutant of the long-double model (tests/_fields_model.py) must miss the tolerance the device is held to by a factor
of at least 100 on the cases it applies to -- else the case is too tame."""
import functools

import numpy as np
import pytest

import _fields_cases as fc
import _fields_model as fm

LD = np.longdouble
MUTANT_FACTOR = 100


@pytest.fixture(scope='module')
def src():
    return fc.parse_source()


def test_restated_constants_equal_the_source(src):
    d = src
    assert d['lines_cond'] and d['lines_LN'] and d['lds_formula'] and d['launch_uses_plan']
    assert d['lpb_pass'] == [fc.LINES_PASS, fc.LINES_PASS] and d['lpb_mod'] == fc.LINES_PASS
    assert d['lines_block'] == d['lines_bounds'] == fc.LINES_PASS
    assert d['lpb_search'] == fc.LINES_SEARCH and d['lds_limit'] == fc.LINES_LDS_LIMIT
    assert d['pts_block'] == fc.POINTS_BLOCK and d['grid_block'] == [fc.POINTS_BLOCK] * 3
    assert d['supported'] == fc.SUPPORTED_TEXT and 'P <= %d' % fc.SINGLE2D_MAX_P in fc.SUPPORTED_TEXT
    assert d['shapes'] == fc.SHAPES and d['nshape'] == len(fc.SHAPES) and d['smallest_wanted'] == fc.SMALLEST_WANTED
    assert d['s2d_lds_limit'] == fc.SINGLE2D_LDS_LIMIT and d['round'] == fc.SINGLE2D_ROUND and d['shrink']
    assert d['image'] and d['geo_columns'] and d['ncol_kernel'] and d['max_comp'] == fc.MAX_COMP
    assert d['sumfact_min_p'] == fc.SUMFACT_MIN_P
    assert d['max_blocks'] == fc.SINGLE2D_MAX_BLOCKS and d['max_tile'] == fc.SINGLE2D_MAX_TILE and d['wanted']
    # the queries and the launches share one function each
    assert d['query_uses_plan'] and d['launch_uses_s2d_plan']


def test_dispatch_names_exactly_the_listed_instantiations(src):
    assert src['instantiations'] == set(fc.INSTANTIATIONS)
    assert src['lines_dispatch'] == {'2d': ((2, 3), (2, 2)), '3d': ((3, 4), (3, 3))}
    assert src['pts_dispatch'] == [(2, True), (2, False), (3, True), (3, False)]
    # k_coeff_affine<2> is gone: nothing reached it (igx_patch_set_coeff_affine refuses 2D patches)
    assert ('k_coeff_affine', (2,)) not in src['instantiations']


def test_lines_per_block():
    assert [fc.lines_per_block(n) for n in (2, 255, 256, 257, 258, 259, 260)] == [128, 1, 1, 1, 1, 1, 1]
    assert [fc.lines_per_block(n) for n in (288, 320, 384, 512, 576)] == [8, 4, 2, 1, 4]


@functools.lru_cache(maxsize=None)
def _field_plans():
    return {c.id: fc.field_case_plan(c) for c in fc.FIELD_CASES}


def test_every_field_instantiation_and_edge_has_a_case():
    plans = _field_plans()
    inst = {fc.fields_instantiation(c.dim, plans[c.id][2], c.kind.startswith('form')) for c in fc.FIELD_CASES}
    want = {i for i in fc.INSTANTIATIONS if i[0].startswith('k_geo_fields')}
    assert inst == want, inst ^ want
    lines = [c for c in fc.FIELD_CASES if plans[c.id][2]['lines']]
    LN2 = {plans[c.id][1].L1 for c in lines if c.dim == 2}
    assert LN2 >= {2, 256, 257, 258, 259, 260, 288, 320, 384, 512, 576}
    assert {plans[c.id][2]['lpb'] for c in lines if c.dim == 2} >= {128, 8, 4, 2, 1}
    nl = lambda c: plans[c.id][1].G0 * (plans[c.id][1].L1 if c.dim == 3 else 1)
    # a ragged last block, in 2D and in 3D; 3D blocks that start inside a plane (G1 does not divide the lines of a block)
    for dim in (2, 3):
        assert any(nl(c) > plans[c.id][2]['lpb'] > 1 and nl(c) % plans[c.id][2]['lpb'] for c in lines if c.dim == dim), dim
    assert any(nl(c) > plans[c.id][2]['lpb'] and plans[c.id][2]['lpb'] % plans[c.id][1].L1 for c in lines if c.dim == 3)
    for dim in (2, 3):
        assert any(c.win[0] == 'slab' and plans[c.id][1].g0 > 0 for c in lines if c.dim == dim), dim
        # the silent fall-back: a spline geometry on a whole patch or slab whose line coefficients exceed the limit
        fb = [c for c in fc.FIELD_CASES if c.dim == dim and c.geo != 'jac' and c.win[0] != 'box' and not plans[c.id][2]['lines']]
        assert {c.kind.startswith('form') for c in fb} == {False, True}, dim
        box = [c for c in fc.FIELD_CASES if c.dim == dim and c.win[0] == 'box']
        assert any(plans[c.id][1].b1 > 0 and (dim == 2 or plans[c.id][1].b2 > 0) for c in box), dim
        jac = [c for c in fc.FIELD_CASES if c.dim == dim and c.geo == 'jac']
        assert {c.win[0] for c in jac} == {'whole', 'slab'} and any(plans[c.id][1].g0 > 0 for c in jac), dim
    # the limit itself: the same patch with two components stays line-wise
    a, b = (next(c for c in fc.FIELD_CASES if c.id == i) for i in ('2d-fallback-stiff-nurbs', '2d-nofallback-stiff-bsp'))
    assert fc.fields_plan(2, 2, a.geo, False)['lines'] is False and plans[b.id][2] == {'lines': True, 'lpb': 128, 'lds': 49152, 'nc': 2}
    pts = [c for c in fc.FIELD_CASES if not plans[c.id][2]['lines']]
    assert any((plans[c.id][1].G0 * plans[c.id][1].L1 * plans[c.id][1].L2) % fc.POINTS_BLOCK for c in pts)
    assert any(plans[c.id][1].G0 * plans[c.id][1].L1 * plans[c.id][1].L2 > fc.POINTS_BLOCK for c in pts)
    kinds = {(c.dim, c.kind, c.extra) for c in fc.FIELD_CASES}
    assert {(3, 'convdiff', 'sampled'), (3, 'convdiff', 'affine')} <= kinds
    for dim in (2, 3):
        assert (dim, 'form_par', None) in kinds
    assert {e for d, k, e in kinds if k == 'form_phys'} == {'value_only', 'deriv_nonsym', 'mixed_sym', 'mixed_nonsym'}
    # k_coeff_affine<3>: whole-patch slab and span box (b1, b2 > 0)
    aff = [c for c in fc.FIELD_CASES if c.extra == 'affine']
    assert {c.win[0] for c in aff} == {'slab', 'box'} and any(plans[c.id][1].b1 > 0 and plans[c.id][1].b2 > 0 for c in aff)


def test_grid_cases_cover_components_and_totals():
    tot = lambda c: int(np.prod([len(g) for g in c.grid]))
    for dim in (2, 3):
        cs = [c for c in fc.GRID_CASES if len(c.grid) == dim]
        assert {tot(c) for c in cs} >= {127, 128, 129}
        assert {c.ncomp for c in cs if not c.spec.nurbs} >= {1, fc.MAX_COMP} and {c.ncomp for c in cs if c.spec.nurbs} >= {1, fc.MAX_COMP - 1}
        assert all(c.ncomp + c.spec.nurbs <= fc.MAX_COMP for c in cs)
        knots = lambda c, a: set(c.spec.axes[a][1])
        assert any(0. in c.grid[a] and 1. in c.grid[a] and knots(c, a) & set(c.grid[a]) and len(set(c.grid[a])) < len(c.grid[a])
                   for c in cs for a in range(dim)), dim
    assert {c.ncomp for c in fc.GRID_CASES if len(c.grid) == 2 and not c.spec.nurbs} >= {1, 2, 3, 4}


# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _s2d_plans():
    out = {}
    for c in fc.S2D_CASES:
        if fc.s2d_refused(c):
            continue
        sp = fc.Space(c.axes, c.nqp)
        for kind in fc.S2D_KINDS:
            out[(c.id, kind)] = (sp, fc.single2d_plan(sp, c.geo, kind, c.path))
    return out


def test_every_reachable_tile_shape_has_a_case():
    reach = fc.reachable_shapes()
    assert set(reach) == set(range(len(fc.SHAPES))), reach          # by enumeration: every shape is reachable ...
    assert reach[0][-1] == 'single'                                 # ... 8 x 8 rows on request only (64 > SINGLE2D_MAX_TILE)
    plans = _s2d_plans()
    by_shape = {}
    for (cid, kind), (sp, pl) in plans.items():
        assert pl['supported'] and pl['wanted'], (cid, kind)
        by_shape.setdefault((pl['R0'], pl['R1']), set()).add(kind)
    assert set(by_shape) == set(fc.SHAPES), set(fc.SHAPES) ^ set(by_shape)
    for shape in ((8, 8), (6, 6), (4, 4), (2, 4)):
        assert by_shape[shape] == set(fc.S2D_KINDS), shape
    # the hand count: degree 5 with nqp 8, 9, 11 lands the stiffness form on 2 x 2, 1 x 2 and 1 x 1 rows
    shape = lambda cid: (plans[(cid, 'stiffness')][1]['R0'], plans[(cid, 'stiffness')][1]['R1'])
    assert [shape(c) for c in ('p5-q8', 'p5-q9', 'p5-q11-jac', 'p54-q11-nurbs')] == [(2, 2), (1, 2), (1, 1), (1, 1)]
    assert all(plans[(c, 'stiffness')][1]['lds'] > 64 * 1024 for c in ('p5-q8', 'p5-q9', 'p5-q11-jac'))      # (the opt-in LDS size)


def test_single2d_cases_hit_the_edges():
    plans = _s2d_plans()
    cs = {c.id: c for c in fc.S2D_CASES}
    N = lambda c: [t.N for t in plans[(c.id, 'mass')][0].tables]
    run = [c for c in fc.S2D_CASES if not fc.s2d_refused(c)]
    seen = {}
    for (cid, kind), (sp, pl) in plans.items():
        c, n = cs[cid], [t.N for t in sp.tables]
        e = seen.setdefault((pl['R0'], pl['R1']), set())
        e |= {'ragged0'} if n[0] % pl['R0'] else set()
        e |= {'ragged1'} if n[1] % pl['R1'] else set()
        e.add('jac' if c.geo == 'jac' else 'nurbs' if c.geo.nurbs else 'bsp')
        for lo, hi in c.slabs:                              # (a slab plans its own tile from its own rows)
            ps = fc.single2d_plan(sp, c.geo, kind, c.path, row0=(lo, hi))
            if lo % ps['R0']:
                seen.setdefault((ps['R0'], ps['R1']), set()).add('slab')
    for shape in fc.SHAPES:
        need = ({'ragged0', 'slab'} if shape[0] > 1 else set()) | ({'ragged1'} if shape[1] > 1 else set())
        assert need <= seen[shape], (shape, seen[shape])
    assert {'jac', 'nurbs', 'bsp'} <= seen[(2, 4)] and {'jac', 'bsp'} <= seen[(8, 8)] and {'jac', 'nurbs'} <= seen[(1, 1)]
    tile = lambda c: (plans[(c.id, 'mass')][1]['R0'], plans[(c.id, 'mass')][1]['R1'])
    # a patch smaller than one tile (two dofs per axis are the least a degree >= 1 gives)
    assert any(all(n <= r for n, r in zip(N(c), tile(c))) and N(c)[1] < tile(c)[1] for c in run)
    p = lambda c: [a[0] for a in c.axes]
    # degree 0 on either axis: refused by the sum-factorised assembly, asserted on the device; unequal degrees both ways
    assert any(p(c)[0] == 0 for c in fc.S2D_CASES) and any(p(c)[1] == 0 for c in fc.S2D_CASES)
    assert any(p(c)[0] < p(c)[1] for c in run) and any(p(c)[0] > p(c)[1] for c in run)
    assert any(c.nqp and c.nqp > max(p(c)) + 1 for c in fc.S2D_CASES)
    for a in (0, 1):                                        # interior knots of multiplicity 2 and p
        assert any(isinstance(c.axes[a][2], tuple) and 2 in c.axes[a][2] and c.axes[a][0] in c.axes[a][2] for c in run), a
    assert any(c.path == 'single' for c in fc.S2D_CASES) and any(c.path == 'default' for c in fc.S2D_CASES)
    # a geometry mesh finer than the space mesh and not nested, a repeated interior geometry knot, one on a space knot
    fine = [c for c in fc.S2D_CASES if c.geo != 'jac' and len(c.geo.axes[1][1]) > c.axes[1][1]]
    assert fine
    for c in fine:
        gk = c.geo.axes[1][1]
        sk = set(np.arange(1, c.axes[1][1]) / c.axes[1][1])
        assert len(set(gk)) < len(gk) and set(gk) & sk and set(gk) - sk, c.id


def test_ncol_holds_every_tile():
    """The LDS extent NCOL the host works out from knot counts (geo_columns) is at least the ncol any tile of the kernel computes
    from the first active functions at its first and last window point -- for the tile of the patch and of each slab, and for
    every other shape too (a knob or a larger patch may choose it)."""
    tight = set()
    for c in fc.S2D_CASES:
        if c.geo == 'jac':
            continue
        sp = fc.Space(c.axes, c.nqp)
        gN = len(c.geo.axes[1][1]) + c.geo.axes[1][0] + 1
        for R0, R1 in fc.SHAPES:
            ncol, NCOL = fc.kernel_ncol(sp, c.geo, R1), fc.geo_columns(sp, c.geo, R1)
            assert ncol <= NCOL <= gN, (c.id, R1, ncol, NCOL)
            if ncol == NCOL < gN:
                tight.add(c.id)
    # the bound is met with equality below the whole net (a bound smaller by one would fail above), also under a repeated
    # geometry knot
    assert {'long-8x8', 'long-4x4'} <= tight, tight


# ---------------------------------------------------------------------------------------------
# the tolerance would catch a subtly wrong kernel
@pytest.mark.parametrize('cid', [c.id for c in fc.FIELD_CASES])
def test_field_mutants_miss_the_tolerance(cid):
    case = next(c for c in fc.FIELD_CASES if c.id == cid)
    sp, w, plan = _field_plans()[cid]
    inp = fc.field_inputs(case, sp, w)
    FLD = fc.model_fields(case, LD, sp, w, inp)
    F64 = fc.model_fields(case, np.float64, sp, w, inp)
    tol, D, mag = fm.tolerance(F64, FLD)
    assert np.isfinite(FLD.astype(np.float64)).all() and (mag > 0).all()
    assert fm.deviation(F64, FLD, tol) <= 1.0 / fm.MARGIN + 1e-12
    assert (D < 1e4 * fm.U).all(), D / fm.U                         # (a well-conditioned map: the yardstick is a few ulps)
    for m in fc.field_mutants(case, plan):
        FM = fc.model_fields(case, LD, sp, w, inp, mutate=m, lpb=max(plan['lpb'], 1))
        assert fm.deviation(FM, FLD, tol) >= MUTANT_FACTOR, (m, fm.deviation(FM, FLD, tol))


def test_every_field_mutant_applies_somewhere():
    plans = _field_plans()
    used = {m for c in fc.FIELD_CASES for m in fc.field_mutants(c, plans[c.id][2])}
    assert used == set(fm.FIELD_MUTANTS)


def s2d_model(case, kind, sp=None):
    """(val, mag, npts, bound) of the whole patch, banded (tests/_fields_model.py: assemble2d)."""
    sp = sp or fc.Space(case.axes, case.nqp, with_V=True)
    w = sp.window(('whole',))
    kw = dict(jac=fc.s2d_jac(case, sp)) if case.geo == 'jac' else dict(geo=fc.model_map(case.geo))
    FLD = fm.fields(kind, 2, w, sp.gauss, LD, **kw)
    F64 = fm.fields(kind, 2, w, sp.gauss, np.float64, **kw)
    tol = fm.tolerance(F64, FLD)[0]
    val, mag, npts = fm.assemble2d(sp.tables, FLD, kind)
    magF = fm.assemble2d(sp.tables, FLD, kind, Fmag=np.broadcast_to(tol.reshape(-1, 1, 1), FLD.shape))[1]
    return sp, FLD, val, mag, npts, fm.single2d_bound(kind, mag, npts, magF)


@pytest.mark.parametrize('cid', [c.id for c in fc.S2D_CASES if not c.id.startswith('long') and not fc.s2d_refused(c)] + ['long-4x4'])
def test_assembly_mutants_exceed_the_bound(cid):
    case = next(c for c in fc.S2D_CASES if c.id == cid)
    for kind in fc.S2D_KINDS:
        sp, FLD, val, mag, npts, bound = s2d_model(case, kind)
        idx = fm.csr_order(sp.tables)
        assert (npts[idx] > 0).all() and (bound[idx] > 0).all()
        # entry (j, i) is entry (i, j): the model is symmetric to rounding, far inside the bound
        for m in fm.ASSEMBLY_MUTANTS:
            if m == 'swap_T12' and kind == 'mass':
                continue
            vm = fm.assemble2d(sp.tables, FLD, kind, mutate=m)[0]
            r = float((abs(vm - val)[idx] / bound[idx]).max())
            assert r >= MUTANT_FACTOR, (kind, m, r)

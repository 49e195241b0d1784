"""The entry-wise and pattern kernels (pyiga_amd/csrc/kern_entries.hip) and the cases that run them cannot drift apart, and the
long-double model the GPU test judges them by can tell a wrong kernel from a right one (no GPU needed).

- the instantiations named in launch_entries_list, launch_entries_csr and launch_pattern, the dispatch condition, the block
  sizes, the 4 entries per wave block and IGX_MAX_DEGREE are read from the source and compared with tests/_entries_cases.py;
- every instantiation and every launch edge is reached by a case, computed from the knot vectors alone;
- with fields and basis tables from the oracle the model agrees with the oracle's own entry sums;
- three mutations of the model (a shifted field index, a lost Gauss point, a lost second lane trip) move the entries by more
  than four times the acceptance bound.
"""
import numpy as np
import pytest

import _entries_cases as ec
import _entries_model as em

LD = np.longdouble


@pytest.fixture(autouse=True)
def _wide_long_double():
    assert np.finfo(np.longdouble).eps < 2e-19


@pytest.fixture(scope='module')
def src():
    return ec.read_source()


# ---------------------------------------------------------------------------------------------
# source against table
def test_instantiations(src):
    inst = ec.parse_instances(src)
    assert inst == {'list': ec.LIST_INSTANCES, 'wave': ec.WAVE_INSTANCES, 'csr': ec.CSR_INSTANCES, 'pattern': ec.PATTERN_INSTANCES}
    assert (len(inst['list']), len(inst['wave']), len(inst['csr']), len(inst['pattern'])) == (7, 5, 7, 2)


def test_no_instance_outside_the_launch_functions():
    assert ec.instances_outside_launchers() == []


def test_dispatch_rule_and_constants(src):
    assert ec.parse_dispatch_rule(src) == ec.DISPATCH_RULE
    assert ec.parse_constants(src) == ec.EXPECTED_CONSTANTS
    assert ec.WAVE_BLOCK == ec.WAVE_ENTRIES_PER_BLOCK * ec.WAVE_LANES
    # the restatement around its thresholds
    assert ec.wave_runs('mass', (2, 1, 1), False, 1) and not ec.wave_runs('mass', (1, 1, 1), False, 1)
    assert not ec.wave_runs('mass', (3, 3), True, 1) and not ec.wave_runs('form_phys', (3, 3), False, 1)
    assert ec.wave_runs('convdiff', (2, 2, 2), False, (1 << 25) - 1) and not ec.wave_runs('convdiff', (2, 2, 2), False, 1 << 25)


def test_a_changed_rule_or_instance_is_noticed(src):
    """The parsers see an edit of the source: a scratch copy with the rule changed, one with an instantiation added."""
    changed = src.replace('pmax >= 2 &&', 'pmax >= 3 &&')
    assert changed != src and ec.parse_dispatch_rule(changed) != ec.DISPATCH_RULE
    line = '        if (kind == IGX_MASS) k_entries_wave<2, IGX_MASS><<<gridw, blockw, 0, st>>>(pd, pt->d_fields, d_ij, M, d_out);'
    assert line in src
    added = src.replace(line, line.replace('IGX_MASS>', 'IGX_FORM>') + '\n' + line)
    assert ec.parse_instances(added)['wave'] != ec.WAVE_INSTANCES


# ---------------------------------------------------------------------------------------------
# reach
@pytest.fixture(scope='module')
def reach():
    """Per case: tables, window, picks and their classes / overlaps, from the knot vectors alone."""
    out = {}
    for c in ec.CASES:
        ax, w, idx = c.tables(), c.window(), ec.picks(c)
        out[c.id] = (ax, w, idx, [em.classify(ax, w, I, J) for I, J in idx])
    return out


def test_every_instantiation_is_reached(reach):
    got = {'list': set(), 'wave': set(), 'csr': set(), 'pattern': set()}
    how_list = {}
    for c in ec.CASES:
        M = len(reach[c.id][2])
        degrees = [a[0] for a in c.axes]
        for kind in c.kinds:
            for thread in (False, True):
                for m in ec.request_lengths(M):
                    fam, inst = ec.entries_kernel(c, kind, thread, m)
                    got[fam].add(inst)
                    if fam == 'list' and ec.KIND_ENUM[kind] != 'FORM':
                        how_list.setdefault(inst, set()).add('thread' if max(degrees) >= 2 else 'p1')
            if c.assemble:
                got['csr'].add((c.dim, ec.KIND_ENUM[kind]))
        if c.assemble:
            got['pattern'].add(c.dim)
    assert got == {'list': ec.LIST_INSTANCES, 'wave': ec.WAVE_INSTANCES, 'csr': ec.CSR_INSTANCES, 'pattern': ec.PATTERN_INSTANCES}
    # the fixed forms reach k_entries_list both ways: IGX_ENTRIES=thread at p >= 2, and an all-p=1 patch
    assert all(how == {'thread', 'p1'} for how in how_list.values()) and len(how_list) == 5, how_list
    # both kinds of IGX_FORM in 2D and 3D
    for dim in (2, 3):
        assert {k for c in ec.CASES if c.dim == dim for k in c.kinds} >= {'form_phys', 'form_par'}


def test_tails(reach):
    for c in ec.CASES:
        M = len(reach[c.id][2])
        lens = ec.request_lengths(M)
        assert {m % 4 for m in lens} >= {1, 2, 3} and 1 in lens and min(lens) >= 1, (c.id, M)
        assert all(m % ec.LIST_BLOCK != 0 for m in lens)
    assert any(len(reach[c.id][2]) > ec.LIST_BLOCK for c in ec.CASES)          # more than one block of the thread kernel


def test_wave_boxes(reach):
    """Lane loop of k_entries_wave: boxes under, at and over 64 points, and over 128 (a third trip), among the value picks of the
    cases the wave kernel serves; in 2D and in 3D."""
    sizes = {2: set(), 3: set()}
    for c in ec.CASES:
        if not any(ec.wave_runs(k, [a[0] for a in c.axes], False, 1) for k in c.kinds):
            continue
        sizes[c.dim] |= {em.box_points(ov) for cls, ov in reach[c.id][3] if cls == 'value'}
    both = sizes[2] | sizes[3]
    assert min(both) < 64 and 64 in both and any(64 < s <= 128 for s in both) and max(both) > 128
    assert max(sizes[2]) > 64 and max(sizes[3]) > 128 and 64 in sizes[3]
    # per-axis: a two-function axis and a 16-function axis under the wave kernel
    assert any(1 in [a[0] for a in c.axes] and max(a[0] for a in c.axes) >= 2 for c in ec.CASES)


def test_degrees_and_knots():
    # (one line per case of the table: a line that is dropped, renamed or added shows here)
    assert [c.id for c in ec.CASES] == ['p1_2d', 'p1_3d', 'p3_2d_nqp17', 'p3_3d', 'p4_3d', 'p15_2d', 'p8_3_2d', 'p15_2_1_3d', 'mixed_3d',
                                        'rep_ax0_2d', 'rep_last_3d', 'c0_2d', 'slab_2d', 'slab_3d', 'slab1_2d', 'box_2d', 'box_3d', 'p0_2d']
    deg ={a[0] for c in ec.CASES for a in c.axes}
    assert {0, 1, 2, 3, 4, 8, 15} <= deg and max(deg) == ec.IGX_MAX_DEGREE
    by = ec.BY_ID
    assert by['p15_2d'].axes == ((15, 2, 1), (15, 2, 1)) and by['p8_3_2d'].axes[0][0] == 8 and by['p8_3_2d'].axes[1][0] == 3
    assert [a[0] for a in by['p15_2_1_3d'].axes] == [15, 2, 1] and [a[1] for a in by['p15_2_1_3d'].axes] == [1, 3, 4]
    assert all(a[0] == 4 and a[0] + a[1] >= 2 * a[0] + 2 for a in by['p4_3d'].axes)
    assert any(c.axes[0][2] > 1 for c in ec.CASES) and any(c.axes[-1][2] > 1 for c in ec.CASES)
    assert any(a[2] == a[0] and a[0] >= 2 for c in ec.CASES for a in c.axes)             # C^0
    assert any(c.nqp and c.nqp > max(a[0] for a in c.axes) + 1 for c in ec.CASES)
    assert {a[0] for a in ec.HIGH_DEGREE_AXES} >= {8, 15} and all(8 <= a[0] <= 15 for a in ec.HIGH_DEGREE_AXES)
    # rows far shorter than maxrow (boundary rows, repeated knots, mixed degrees): k_pattern / k_entries_csr spread maxrow threads per row
    for c in ec.CASES:
        if c.assemble:
            lens = [np.asarray(a.jhi - a.jlo) for a in c.tables()]
            assert any(L.min() < L.max() for L in lens), c.id
    # interior rows exist: a dof whose row has the full length on every axis
    for cid in ('p3_3d', 'p4_3d'):
        assert all((a.jhi - a.jlo).max() == 2 * a.p + 1 for a in by[cid].tables())


def test_slabs_and_boxes(reach):
    slabs = [c for c in ec.CASES if c.row0]
    assert {c.dim for c in slabs} == {2, 3} and any(c.row0[1] - c.row0[0] == 1 for c in slabs)
    for c in slabs:
        ax, w, idx, cl = reach[c.id]
        assert 0 < c.row0[0] < c.row0[1] < ax[0].N and w.g0 > 0 and w.g0 + w.G0 < ax[0].n * ax[0].q
        inside = sum(cls == 'value' for cls, _ in cl)
        lower = sum(cls == 'nan' and ov[0][0] < w.g0 < ov[0][0] + ov[0][1] for cls, ov in cl)
        upper = sum(cls == 'nan' and ov[0][0] < w.g0 + w.G0 < ov[0][0] + ov[0][1] for cls, ov in cl)
        assert inside >= 10 and lower >= 3 and upper >= 3, (c.id, inside, lower, upper)
    boxes = [c for c in ec.CASES if c.bbox]
    assert {c.dim for c in boxes} == {2, 3}
    for c in boxes:
        ax, w, idx, cl = reach[c.id]
        lo = (w.g0, w.b1, w.b2)
        hi = (w.g0 + w.G0, w.b1 + w.L1, w.b2 + w.L2)
        assert sum(cls == 'value' for cls, _ in cl) >= 10
        for k in range(c.dim):
            assert any(cls == 'nan' and ov[k][0] < lo[k] < ov[k][0] + ov[k][1] for cls, ov in cl), (c.id, k, 'lower face')
            assert any(cls == 'nan' and ov[k][0] < hi[k] < ov[k][0] + ov[k][1] for cls, ov in cl), (c.id, k, 'upper face')
        assert any(cls == 'nan' and any(ov[k][0] + ov[k][1] <= lo[k] or ov[k][0] >= hi[k] for k in range(c.dim)) for cls, ov in cl), (c.id, 'outside')


def test_picks_have_every_class(reach):
    for c in ec.CASES:
        ax, w, idx, cl = reach[c.id]
        Ntot = int(np.prod([a.N for a in ax]))
        classes = [cls for cls, _ in cl]
        assert classes.count('value') >= 20 and classes.count('zero') >= ec.N_OUTSIDE + 4, c.id
        assert (idx >= Ntot).any(axis=1).sum() >= 4 and (idx == Ntot).any()
        assert np.array_equal(idx, ec.picks(c))                                           # seeded
    assert ec.BY_ID['p15_2d'].top1


def test_box_pair_cases():
    for cid in ec.BOX_PAIR_CASES:
        c = ec.BY_ID[cid]
        assert c.dim == 2 and c.assemble and (len({a[0] for a in c.axes}) > 1 or any(a[2] > 1 for a in c.axes))


def test_pattern_against_oracle(oracle):
    """The model's pattern (per-axis column ranges) is the oracle's full_pattern, row by row."""
    for c in ec.CASES:
        ax = c.tables()
        okvs = [oracle.KnotVector(kv.kv, kv.p) for kv in c.kvs()]
        I, J = oracle.full_pattern(okvs)
        order = np.lexsort((J, I))
        indptr, indices = em.pattern(ax)
        assert np.array_equal(indices, J[order]) and np.array_equal(np.diff(indptr), np.bincount(I, minlength=len(indptr) - 1)), c.id
        if c.row0:
            plane = int(np.prod([a.N for a in ax[1:]]))
            ip, ind = em.pattern(ax, c.row0)
            lo, hi = indptr[c.row0[0] * plane], indptr[c.row0[1] * plane]
            assert np.array_equal(ind, indices[lo:hi]) and ip[-1] == hi - lo


# ---------------------------------------------------------------------------------------------
# model against oracle, and its sensitivity
def _oracle_geo(oracle, case):
    return {'annulus': oracle.geo_quarter_annulus, 'cylinder': oracle.geo_cylinder, 'twisted': oracle.geo_twisted_box}[case.geo]()


def _oracle_assembler(oracle, kind, okvs, geo, nqp, coeff=None, table=None):
    """oracle.Assembler with `nqp` Gauss points per span (its constructor takes max p + 1; everything else is its own code)."""
    asm = oracle.Assembler.__new__(oracle.Assembler)
    asm.kind, asm.kvs, asm.dim, asm.nqp = kind, tuple(okvs), len(okvs), nqp
    asm.grid, asm.gw = oracle.make_tensor_quadrature([kv.mesh for kv in okvs], nqp)
    asm.nder = 1 if kind == 'mass' else 2
    asm.meshsupp = [np.ascontiguousarray(nqp * kv.mesh_support_idx_all(), dtype=np.int64) for kv in okvs]
    asm.C = [oracle.compute_values_derivs(kv, g, asm.nder - 1) for kv, g in zip(okvs, asm.grid)]
    asm.jac = np.ascontiguousarray(oracle.grid_jacobian(geo, asm.grid))
    if kind == 'convdiff':
        xphys = oracle.grid_eval(geo, asm.grid)
        c = coeff(xphys[..., 0], xphys[..., 1], xphys[..., 2]) * np.ones(xphys.shape[:-1])
        asm.fields = np.ascontiguousarray(oracle.precompute_fields_convdiff(asm.jac, xphys, c, asm.gw))
    elif kind == 'form':
        asm.fields = np.ascontiguousarray(oracle.precompute_fields_form(asm.jac, table, asm.gw))
    else:
        asm.fields = np.ascontiguousarray(oracle.precompute_fields(kind, asm.jac, asm.gw))
    asm.ndofs = np.array([kv.numdofs for kv in okvs], dtype=np.uintp)
    asm.ngauss = np.array([g.shape[0] for g in asm.grid], dtype=np.uintp)
    return asm


# roundings on one monomial of the ORACLE's term where it composes the fields inside its loop (oracle_kernels.c); the model gets the
# composed fields in long double, so these stand in for C_KIND in the comparison with the oracle (and the magnitude is taken
# from fields composed of absolute values: the oracle's intermediate sums are bounded by those, not by |composed field|):
#   convdiff: gu (du 2, product 1, adds 2) 5, gv 5, f0*gu*gv 2, adds 2, + convection 1, * W 1 = 16  (convection: 5 + 2 + 2 + 1 + 1)
#   form 2D: Gu (du 1, product 1, add 1) 3, Gv 3, two products, up to 9 adds, * W = 18;  3D: 5 + 5 + 2 + 16 + 1 = 29
C_ORACLE = {('convdiff', 3): 16, ('form', 2): 18, ('form', 3): 29}


def _composed_fields(kind, dim, raw, ab, absolute):
    """The device's field layout from the oracle's raw per-point data, in long double: convdiff [c, x, y, z, W, JacInv(9)] ->
    c W JI JI^T (upper triangle), W JI b with b = (y, -x, 1); form [P(16), W, JacInv] -> W T P T^t at the (a, b) of form_ab."""
    f = np.moveaxis(np.asarray(raw), -1, 0).astype(LD)
    fix = abs if absolute else (lambda x: x)
    if kind == 'convdiff':
        c, x, y, W = fix(f[0]), f[1], f[2], f[4]
        JI = fix(f[5:14]).reshape((3, 3) + f.shape[1:])
        b = [fix(y), fix(-x), np.ones_like(y)]
        out = [c * W * sum(JI[a][r] * JI[bb][r] for r in range(3)) for a in range(3) for bb in range(a, 3)]
        out += [W * sum(JI[a][r] * b[r] for r in range(3)) for a in range(3)]
        return np.stack(out)
    P, W = fix(f[:16]).reshape((4, 4) + f.shape[1:]), f[16]
    T = np.zeros((4, 4) + f.shape[1:], dtype=LD)
    T[0, 0] = 1
    T[1:dim + 1, 1:dim + 1] = fix(f[17:17 + dim * dim]).reshape((dim, dim) + f.shape[1:])
    return np.stack([W * sum(T[t >> 2][r] * P[r][s] * T[t & 3][s] for r in range(dim + 1) for s in range(dim + 1)) for t in ab])


@pytest.fixture(scope='module')
def host_inputs(oracle):
    """case id -> (axis tables with the oracle's basis values, window, picks, {kind: (fields, fields for the magnitude or None,
    oracle assembler or None)}), fields in the device's layout over the window."""
    cache = {}

    def get(cid):
        if cid in cache:
            return cache[cid]
        c = ec.BY_ID[cid]
        q, dim = c.q(), c.dim
        kvs = c.kvs()
        okvs = [oracle.KnotVector(kv.kv, kv.p) for kv in kvs]
        grid, gw = oracle.make_tensor_quadrature([kv.mesh for kv in okvs], q)
        for g, kv in zip(grid, kvs):
            assert np.array_equal(g, em.gauss_nodes(kv, q))
        ax = em.tables_from_active_deriv(kvs, q, [oracle.active_deriv(kv, g, 1) for kv, g in zip(okvs, grid)])
        w = c.window()
        sl = (slice(None), slice(w.g0, w.g0 + w.G0), slice(w.b1, w.b1 + w.L1)) + ((slice(w.b2, w.b2 + w.L2),) if dim == 3 else ())
        geo = _oracle_geo(oracle, c)
        per_kind = {}
        for kind in c.kinds:
            form = ec.form_of(c, kind)
            if kind == 'form_par':
                GW = gw[0].astype(LD)
                for x in gw[1:]:
                    GW = GW[..., None] * x.astype(LD)
                F = np.stack([GW * coef.astype(LD) for _, _, coef in ec.par_terms(dim, grid)])
                per_kind[kind] = (F[sl], None, None)
                continue
            asm = _oracle_assembler(oracle, ec.model_kind(kind), okvs, geo, q, coeff=lambda x, y, z: 1.0 + x,
                                    table=ec.phys_table(dim, grid) if kind == 'form_phys' else None)
            if kind in ('mass', 'stiffness'):
                per_kind[kind] = (np.moveaxis(asm.fields, -1, 0)[sl], None, asm)
            else:
                ab = form[1] if form else None
                per_kind[kind] = (_composed_fields(ec.model_kind(kind), dim, asm.fields, ab, False)[sl],
                                  _composed_fields(ec.model_kind(kind), dim, asm.fields, ab, True)[sl], asm)
        cache[cid] = (ax, w, ec.picks(c), per_kind)
        return cache[cid]
    return get


@pytest.mark.parametrize('cid', [c.id for c in ec.CASES])
def test_model_against_oracle(cid, host_inputs):
    """Mass and stiffness: the oracle sums the same term in double, so the bound of the GPU test applies as it stands.  Convdiff
    and the physical form: the oracle composes the fields inside its loop, see C_ORACLE.  Parametric forms have no oracle."""
    c = ec.BY_ID[cid]
    ax, w, idx, per_kind = host_inputs(cid)
    whole = em.whole_window(ax)
    Ntot = int(np.prod([a.N for a in ax]))
    for kind in c.kinds:
        F, Fmag, asm = per_kind[kind]
        if asm is None:
            continue
        form = ec.form_of(c, kind)
        terms = em.terms_of(c.dim, ec.model_kind(kind), form)
        ck = C_ORACLE.get((ec.model_kind(kind), c.dim), em.c_kind(c.dim, ec.model_kind(kind), form))
        ref = asm.multi_entries(np.where(idx >= Ntot, Ntot, idx))           # (the oracle takes any index past the end)
        worst = 0.0
        for (I, J), r in zip(idx, ref):
            e = em.entry(ax, w, F, terms, I, J, fields_mag=Fmag)
            if e.cls == 'zero':
                assert r == 0.0 and em.classify(ax, whole, I, J)[0] == 'zero'
            elif e.cls == 'value':
                b = em.bound(e, ck)
                assert abs(LD(r) - e.value) <= b, (cid, kind, int(I), int(J), float(abs(LD(r) - e.value) / b))
                worst = max(worst, float(abs(LD(r) - e.value) / b))
            else:
                assert em.classify(ax, whole, I, J)[0] == 'value' and (c.row0 or c.bbox)
        print('%s %s: max |oracle - model| / bound = %.3f' % (cid, kind, worst))


MUTATIONS = ('shift', 'drop1', 'drop64')


@pytest.mark.parametrize('cid', [c.id for c in ec.CASES])
def test_model_sensitivity(cid, host_inputs):
    """Each mutation moves at least a quarter of the value picks it applies to by more than 4 times the bound ('drop64' applies
    to picks whose box has more than 64 points)."""
    c = ec.BY_ID[cid]
    ax, w, idx, per_kind = host_inputs(cid)
    for kind in c.kinds:
        F = per_kind[kind][0]
        form = ec.form_of(c, kind)
        terms = em.terms_of(c.dim, ec.model_kind(kind), form)
        ck = em.c_kind(c.dim, ec.model_kind(kind), form)
        base = em.entries(ax, w, F, terms, idx)
        for mut in MUTATIONS:
            applies = [k for k, e in enumerate(base) if e.cls == 'value' and (mut != 'drop64' or e.nbox > 64)]
            if mut == 'drop64' and not applies:
                continue
            assert len(applies) >= 4, (cid, kind, mut)
            moved = 0
            for k in applies:
                m = em.entry(ax, w, F, terms, idx[k][0], idx[k][1], mutate=mut)
                moved += abs(m.value - base[k].value) > 4 * em.bound(base[k], ck)
            assert 4 * moved >= len(applies), (cid, kind, mut, moved, len(applies))


def test_recorded_basis_table_deviations(oracle):
    """ORACLE_TABLE_DEVIATION is what the oracle's double-precision recursion does at these axes today (recorded rounded up,
    so: not above the record, and not far below it)."""
    from pyiga_amd import bspline
    assert set(ec.ORACLE_TABLE_DEVIATION) == set(ec.HIGH_DEGREE_AXES)
    for p, n, m in ec.HIGH_DEGREE_AXES:
        kv = bspline.make_knots(p, 0.0, 1.0, n, mult=m)
        u = em.gauss_nodes(kv, p + 1)
        ref = em.active_deriv_ld(kv, u, 2)
        got = em.table_deviation(oracle.active_deriv(oracle.KnotVector(kv.kv, p), u, 2), ref)
        for g, rec in zip(got, ec.ORACLE_TABLE_DEVIATION[(p, n, m)]):
            assert rec - 0.11 <= g <= rec, ((p, n, m), got)


def test_long_double_recursion_against_oracle(oracle):
    """The model's long-double Piegl-Tiller recursion restates the oracle's statement by statement: at a low degree the oracle's
    double values lie within a few roundings of it (values, first and second derivatives), the spans are equal, and its values
    sum to 1."""
    from pyiga_amd import bspline
    kv = bspline.make_knots(3, 0.0, 1.0, 4, mult=2)
    okv = oracle.KnotVector(kv.kv, kv.p)
    u = em.gauss_nodes(kv, 4)
    ref = em.active_deriv_ld(kv, u, 2)
    got = oracle.active_deriv(okv, u, 2)
    for k in range(3):
        assert float(abs(got[k] - ref[k]).max() / abs(ref[k]).max()) < 32 * 2.0 ** -53
    assert np.array_equal([em.findspan(kv.kv, 3, x) for x in u], [oracle.findspan(okv.kv, 3, float(x)) for x in u])
    assert abs(ref[0].sum(axis=0) - 1).max() < 2.0 ** -60

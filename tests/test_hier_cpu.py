"""Hierarchical spline spaces without a GPU: the space against the reference's (tests/golden/golden_hier.npz), the coupling
formula as a numpy model fed with the oracle's tensor-product matrices against the reference's matrices, the host planning
of the device contraction, and the refusals."""
import numpy as np
import pytest
import scipy.sparse

import _hier_cases as hc
import _hier_model as hm
from conftest import golden_csr

from pyiga_amd import assemble, bspline, geometry, hierarchical
from pyiga_amd.hierarchical import HSpace

CASE_IDS = list(hc.CASES)
_SPACES = {}


def space(name):
    if name not in _SPACES:
        _SPACES[name] = hc.build(bspline, HSpace, name)
    return _SPACES[name]


def gold_matrix(g, name):
    if name + 'u_data' in g.files:
        U = golden_csr(g, name + 'u')
        return (U + scipy.sparse.triu(U, k=1).T).tocsr()
    return golden_csr(g, name)


def as_array(tuples, dim):
    return np.array(sorted(tuples), dtype=np.int32).reshape(-1, dim)


@pytest.mark.parametrize('name', CASE_IDS)
def test_space_matches_reference(golden, name):
    g = golden('hier')
    hs, refined = space(name)
    dim = hs.dim
    assert hs.numlevels == int(g[name + '_nlev'])
    assert hs.numactive == tuple(g[name + '_numactive']) == hc.CASES[name][6]
    assert hs.numdofs == sum(hs.numactive)
    knots = np.split(g[name + '_kv'], np.cumsum(g[name + '_kvlen'])[:-1])
    mine = [kv.kv for lv in range(hs.numlevels) for kv in hs.knotvectors(lv)]
    assert len(knots) == len(mine) and all(a.shape == b.shape and np.allclose(a, b, rtol=0, atol=1e-15) for a, b in zip(mine, knots))

    def level_rows(key, lv):
        rows = g[name + key]
        return rows[rows[:, 0] == lv, 1:]
    for lv in range(hs.numlevels):
        assert np.array_equal(as_array(hs.active_cells(lv), dim), level_rows('_ac', lv))
        assert np.array_equal(as_array(hs.deactivated_cells(lv), dim), level_rows('_dc', lv))
        assert np.array_equal(as_array(hs.active_functions(lv), dim), level_rows('_af', lv))
        assert np.array_equal(as_array(hs.deactivated_functions(lv), dim), level_rows('_df', lv))
        # canonical order: ascending ravelled index
        af = level_rows('_af', lv)
        want = np.ravel_multi_index(af.T, hs.mesh(lv).numdofs) if af.size else np.arange(0)
        assert np.array_equal(hs.active_indices()[lv], want)
    assert sum(len(c) for c in hs.active_cells()) == hs.total_active_cells
    flat = hs.active_functions(flat=True)
    assert len(flat) == hs.numdofs and flat == sorted(flat)
    assert np.array_equal(hs.dirichlet_dofs(), g[name + '_dirichlet'])
    nd = hs.non_dirichlet_dofs()
    assert sorted(set(nd) | set(hs.dirichlet_dofs().tolist())) == list(range(hs.numdofs)) and not set(nd) & set(hs.dirichlet_dofs().tolist())
    # what refine() reported: with a finite disparity a superset of the marked cells
    ref = g[name + '_ref']
    assert len(refined) == hc.CASES[name][3] and set(ref[:, 0].tolist()) <= set(range(len(refined)))
    for r, marked in enumerate(refined):
        rows = ref[ref[:, 0] == r]
        assert sorted(lv for lv, c in marked.items() if len(c)) == sorted(set(rows[:, 1].tolist()))
        for lv in set(rows[:, 1].tolist()):
            assert np.array_equal(as_array(marked[lv], dim), rows[rows[:, 1] == lv, 2:])


@pytest.mark.parametrize('name', CASE_IDS)
def test_representation_matches_reference(golden, name):
    g = golden('hier')
    hs, _ = space(name)
    rows1 = hs.active_indices()[1]
    for key, kw in (('_rf1hb', dict(lv=1, truncate=False)), ('_rf1thb', dict(lv=1, truncate=True)),
                    ('_rf1rows', dict(lv=1, truncate=False, rows=rows1)), ('_rf1restr', dict(lv=1, truncate=False, rows=rows1, restrict=True))):
        assert (name + key + '_data' in g.files) == (name in hc.RF_LV1_CASES)
        if name in hc.RF_LV1_CASES:
            R, G = hs.represent_fine(**kw), golden_csr(g, name + key)
            assert R.shape == G.shape, key
            assert abs(R - G).max() < 1e-14, key
    # both bases on the finest level, for every case: entry by entry to 1e-14 where the golden file holds the entries;
    # otherwise the pattern (entries above 1e-14) and the transposed products with two seeded vectors of entries in [-1, 1].
    # Entries within 1e-14 of the reference's move the product of a column by at most 1e-14 times the number of its entries.
    for key, truncate in (('_rfhb', False), ('_rfthb', True)):
        R = hs.represent_fine(truncate=truncate)
        assert R.shape == tuple(g[name + key + '_shape']), key
        if name + key + '_data' in g.files:
            assert abs(R - golden_csr(g, name + key)).max() < 1e-14, key
        else:
            dense = R.toarray()
            pat = np.unpackbits(g[name + key + '_pat'])[:dense.size].reshape(dense.shape).astype(bool)
            assert np.array_equal(abs(dense) > 1e-14, pat), key
            diff = abs(R.T @ hc.probe_vectors(R.shape[0]) - g[name + key + '_probe'])
            assert (diff <= 1e-14 * pat.sum(axis=0)[:, None]).all(), key
    T, Ti = hs.thb_to_hb(), hs.hb_to_thb()
    assert abs(T - golden_csr(g, name + '_t2h')).max() < 1e-14
    assert abs(Ti @ T - scipy.sparse.identity(hs.numdofs)).max() < 1e-13
    # the THB basis is a partition of unity
    assert abs(hs.represent_fine(truncate=True) @ np.ones(hs.numdofs) - 1.0).max() < 1e-13
    x = np.arange(hs.numdofs, dtype=float)
    parts = hs.split_coeffs(x)
    assert [len(p) for p in parts] == list(hs.numactive) and np.array_equal(np.concatenate(parts), x)
    # tp_prolongation: one matrix per axis, whose Kronecker product represents level 0 on level 1
    P = hs.tp_prolongation(0, kron=True)
    assert P.shape == (hs.mesh(1).numbf, hs.mesh(0).numbf) and len(hs.tp_prolongation(0)) == hs.dim
    R1 = hs.represent_fine(lv=1, truncate=False)
    act0 = hs.active_indices()[0]
    assert abs(P[:, act0] - R1[:, :act0.size]).max() < 1e-14 if act0.size else True


def test_copy_and_accessors():
    hs, _ = space('hb2')
    cp = hs.copy()
    cp.refine_region(0, lambda *X: True)
    assert cp.numactive != hs.numactive and hs.numactive == hc.CASES['hb2'][6]
    m = hs.mesh(1)
    assert m.numbf == int(np.prod(m.numdofs)) and len(m.cells()) == int(np.prod(m.numspans))
    f = (1, 2)
    supp = m.support([f])
    assert f in m.supported_in(supp)
    ext = hs.function_support(1, f)
    cells = [hs.cell_extents(1, c) for c in supp]
    assert ext[0][0] == min(c[0][0] for c in cells) and ext[1][1] == max(c[1][1] for c in cells)
    assert m.cell_extents((0, 0)) == hs.cell_extents(1, (0, 0))
    r = hs.ravel_indices(hs.active_functions())
    assert all(np.array_equal(a, b) for a, b in zip(r, hs.active_indices()))
    assert all(np.array_equal(a, b) for a, b in zip(hs.ravel_indices(hs.deactivated_functions()), hs.deactivated_indices()))


# ---------------------------------------------------------------------------------------------------------------------------
def _oracle_levels(oracle, hs, form, dim):
    geo = oracle.geo_bspline_quarter_annulus() if dim == 2 else oracle.geo_twisted_box()
    mats = []
    for k in range(hs.numlevels):
        if hs.numactive[k] == 0:
            mats.append(None)
            continue
        kvs = tuple(oracle.KnotVector(kv.kv, kv.p) for kv in hs.knotvectors(k))
        if form == hc.NONSYM:
            t = [[None] * 4 for _ in range(4)]
            t[1][1] = t[2][2] = 1.0
            t[0][1] = t[0][2] = 1.0
            mats.append(oracle.assemble_nonsymmetric('form', kvs, geo, table=t))
        else:
            mats.append(oracle.assemble('stiffness', kvs, geo=geo))
    return mats, geo


_LEVELS = {}


def oracle_levels(oracle, name):
    if name not in _LEVELS:
        hs, _ = space(name)
        _LEVELS[name] = _oracle_levels(oracle, hs, hc.CASES[name][5], hs.dim)
    return _LEVELS[name]


def _tol(g, name, base=1e-12):
    return base * max(1.0, float(g[name + '_thb_amp'])) if hc.CASES[name][1] else base


@pytest.mark.parametrize('name', CASE_IDS)
def test_model_reproduces_reference(golden, oracle, name):
    """The coupling formula with the oracle's tensor-product matrices gives the reference's matrix and right-hand side."""
    g = golden('hier')
    hs, _ = space(name)
    mats, geo = oracle_levels(oracle, name)
    kvs_levels = [hs.knotvectors(k) for k in range(hs.numlevels)]
    act = hs.active_indices()
    A = hm.hb_matrix(bspline, kvs_levels, act, mats, disparity=hs.disparity)
    vecs = [oracle.inner_products(tuple(oracle.KnotVector(kv.kv, kv.p) for kv in kvs), hc.f_rhs, f_physical=True, geo=geo)
            if hs.numactive[k] else None for k, kvs in enumerate(kvs_levels)]
    b = hm.hb_vector(act, vecs)
    if hs.truncate:
        T = hs.thb_to_hb()
        A = T.T @ A @ T
        b = T.T @ b
    G = gold_matrix(g, name + '_A').toarray()
    err = hc.rel_maxdiff(A, G)
    errb = abs(b - g[name + '_rhs']).max() / abs(g[name + '_rhs']).max()
    print(name, 'model vs reference: matrix %.2e rhs %.2e' % (err, errb))
    assert err < _tol(g, name)
    assert errb < _tol(g, name)


@pytest.mark.parametrize('name', CASE_IDS)
def test_plan_pattern_and_positions(oracle, name):
    """The host plan: CSR pattern = support overlap, one position per entry, and the model of the kernel fed with the oracle's
    entries writes every position (NaN-filled buffer) and reproduces the coupling formula."""
    hs, _ = space(name)
    pl = hierarchical.plan(hs)
    n = hs.numdofs
    indptr, indices = pl['indptr'], pl['indices']
    assert indptr.dtype == np.int32 and indices.dtype == np.int32 and indptr[-1] == indices.size and indptr.size == n + 1
    rows = np.repeat(np.arange(n), np.diff(indptr))
    assert (np.diff(rows * n + indices.astype(np.int64)) > 0).all()            # rows sorted, columns ascending, no duplicates
    kvs_levels = [hs.knotvectors(k) for k in range(hs.numlevels)]
    P = hm.overlap_pattern(bspline, kvs_levels, hs.active_indices(), disparity=hs.disparity)
    mine = np.zeros((n, n), dtype=bool)
    mine[rows, indices] = True
    assert np.array_equal(mine, P)
    # one output position per entry: pos and pos2 together hit every position exactly once
    hits = np.zeros(indices.size, dtype=int)
    for k, lev in enumerate(pl['levels']):
        for blk in lev['blocks']:
            np.add.at(hits, blk['pos'], 1)
            np.add.at(hits, blk['pos2'][blk['pos2'] >= 0], 1)
            assert (blk['pos2'] >= 0).all() or blk['la'] == k                    # only diagonal entries have no mirror
    assert (hits == 1).all()
    mats, _ = oracle_levels(oracle, name)
    layouts, entries = [], []
    for k, lev in enumerate(pl['levels']):
        if not lev['blocks']:
            layouts.append(None)
            entries.append(None)
            continue
        lay = hierarchical.level_layout(hs.knotvectors(k), lev['rows'])
        box = assemble.bbox_for_rows(hs.knotvectors(k), lev['rows'])
        assert all(0 <= lo < hi <= kv.numspans for (lo, hi), kv in zip(box, hs.knotvectors(k)))
        assert lay['rowptr'][-1] == lay['pairs'].shape[0] and (lay['slot'] >= 0).sum() == lev['rows'].size
        layouts.append(lay)
        entries.append(np.asarray(scipy.sparse.csr_matrix(mats[k])[lay['pairs'][:, 0], lay['pairs'][:, 1]]).ravel())
    sym = hc.CASES[name][5] != hc.NONSYM
    vals = hm.model_contract(hs, pl, layouts, entries, symmetric=sym)
    assert not np.isnan(vals).any()
    A = scipy.sparse.csr_matrix((vals, indices, indptr), shape=(n, n)).toarray()
    ref = hm.hb_matrix(bspline, kvs_levels, hs.active_indices(), mats, disparity=hs.disparity)
    assert hc.rel_maxdiff(A, ref) < 1e-14
    if sym:
        assert abs(A - A.T).max() == 0.0
        both = hm.model_contract(hs, pl, layouts, entries, symmetric=False)
        assert abs(both - vals).max() <= 1e-13 * abs(vals).max()


def test_refusals_come_before_the_device():
    """What is outside the scope raises NotImplementedError on the host (without a device, reaching it would raise something
    else)."""
    hs, _ = space('hb2')
    geo = geometry.bspline_quarter_annulus()
    with pytest.raises(NotImplementedError):
        assemble.assemble('inner(grad(u),grad(v))*dx', hs, geo=geo, bfuns=[('u', 2), ('v', 2)])
    with pytest.raises(NotImplementedError):
        assemble.assemble('u*v*ds', hs, geo=geo, boundary='left')
    with pytest.raises(NotImplementedError):
        assemble.assemble('inner(hess(u),hess(v))*dx', hs, geo=geo)
    with pytest.raises(NotImplementedError):
        assemble.assemble('inner(grad(u,parametric=True),grad(v,parametric=True))*dx', hs, geo=geo)
    w = bspline.BSplineFunc(hs.knotvectors(0), np.ones(hs.mesh(0).numbf))
    with pytest.raises(NotImplementedError):
        assemble.assemble('w*u*v*dx', hs, geo=geo, w=w)
    with pytest.raises(NotImplementedError):
        assemble.assemble('div(u)*p*dx', hs, geo=geo, bfuns=[('u', 2, 0), ('p', 1, 1)])
    with pytest.raises(NotImplementedError):
        hierarchical.HDiscretization(hs, assemble.assemblers.MassAssembler2D, {'geo': geo})

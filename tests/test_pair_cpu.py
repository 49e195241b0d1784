"""Bilinear forms over two spline spaces, host side (no GPU): the pattern and entry models of tests/_pair_model.py against the
reference's matrices (tests/golden/golden_pair.npz, made by tests/golden/make_golden_pair.py), the 1D helpers, the role rule and
the other refusals of ``form_assemblers.space_roles``, and the ABI of the ``igx_pair_*`` entry points.

The entry model is independent of the device code: collocation matrices of both spaces at the shared Gauss grid from the
oracle's ``active_deriv``, the oracle's geometry Jacobians, and the physical coefficient table ``tforms.evaluate`` derives from
the form string.  It must match every golden matrix at ``rel_maxdiff <= 1e-12`` (the project's RTOL; 5.5e-16 was measured for the
th2 mass matrix), and two deliberately wrong variants of it must miss by more than 1e-6: the trial tables used for both spaces,
and (hi2) the Gauss rule taken from the trial space alone.
"""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse

from conftest import ROOT, golden_csr

import _pair_cases as pc
import _pair_model as pm

RTOL = 1e-12


def _geo(oracle, name):
    return oracle.geo_quarter_annulus() if name == 'quarter_annulus' else oracle.geo_twisted_box()


class Ref:
    """Everything the model needs of one case, from the oracle: computed once per case and shared."""

    def __init__(self, oracle, case, q=None, dtype=np.float64):
        self.case = case
        self.ku, self.kv = case.kvs(oracle)
        self.q = case.q() if q is None else q
        geo = _geo(oracle, case.geo)
        nodes, weights = oracle.make_tensor_quadrature([k.mesh for k in self.ku], self.q)
        self.G = tuple(len(g) for g in nodes)
        self.X = oracle.grid_eval(geo, nodes)
        jac = oracle.grid_jacobian(geo, nodes)
        self.JI = np.linalg.inv(jac)
        W = abs(np.linalg.det(jac))
        for k, w in enumerate(weights):
            W = W * w.reshape((1,) * k + (-1,) + (1,) * (len(weights) - 1 - k))
        self.W = W
        self.tab_u = [(oracle.first_active(k, g), oracle.active_deriv(k, g, 1)) for k, g in zip(self.ku, nodes)]
        self.tab_v = [(oracle.first_active(k, g), oracle.active_deriv(k, g, 1)) for k, g in zip(self.kv, nodes)]
        self.Bu = [pm.dense_colloc(k, f, v, dtype) for k, (f, v) in zip(self.ku, self.tab_u)]
        self.Bv = [pm.dense_colloc(k, f, v, dtype) for k, (f, v) in zip(self.kv, self.tab_v)]
        # the wrong variant "trial tables for both spaces": the trial space's active values at the test space's first indices
        self.Bv_wrong = [pm.dense_colloc(k, fv, vu, dtype) for k, (fv, _), (_, vu) in zip(self.kv, self.tab_v, self.tab_u)]
        self.dtype = dtype

    def blocks(self, form, Bv=None):
        """[[dense block of test component a, trial component b]] from the physical table of the form string."""
        from pyiga_amd import tforms
        arity, measure, table, ncs = tforms.evaluate(form.form, self.G, self.X, self.case.args(form), form.bfuns)
        assert arity == 2 and measure == 'dx' and ncs == (form.bfuns[0][1], form.bfuns[1][1])
        n = (int(np.prod([k.numdofs for k in self.kv])), int(np.prod([k.numdofs for k in self.ku])))
        return [[np.zeros(n) if all(e is None for row in tab for e in row) else
                 pm.physical_matrix(self.Bu, self.Bv if Bv is None else Bv, self.W, self.JI, tab, self.dtype) for tab in row] for row in table]


def _layout(blocks, layout):
    if layout == 'blocked':
        return np.block(blocks)
    ncv, ncu = len(blocks), len(blocks[0])
    n1, n0 = blocks[0][0].shape
    A = np.zeros((n1 * ncv, n0 * ncu), dtype=blocks[0][0].dtype)
    for a in range(ncv):
        for b in range(ncu):
            A[a::ncv, b::ncu] = blocks[a][b]
    return A


@pytest.fixture(scope='module')
def refs(oracle):
    cache = {}

    def get(cid):
        if cid not in cache:
            cache[cid] = Ref(oracle, pc.BY_ID[cid])
        return cache[cid]
    return get


@pytest.mark.parametrize('cid', [c.id for c in pc.CASES])
def test_pattern_model_equals_reference(cid, refs, golden):
    """indptr / indices of every golden matrix are those of the product pattern: canonical, complete, no reordering."""
    g, case, ref = golden('pair'), pc.BY_ID[cid], refs(cid)
    indptr, indices, maxrow = pm.pattern(ref.ku, ref.kv)
    assert (len(indptr) - 1, int(np.prod([k.numdofs for k in ref.ku]))) == case.shape and indptr[-1] == case.nnz
    assert np.array_equal(np.diff(indptr) > 0, np.ones(case.shape[0], bool)) and maxrow == np.diff(indptr).max()
    assert cid == 'q1p0' or len(set(np.diff(indptr).tolist())) > 1, 'rows of unequal length'
    npts = pm.npts_matrix(ref.ku, ref.kv, ref.q)
    P = scipy.sparse.csr_matrix((np.ones(len(indices)), indices, indptr), shape=case.shape)
    assert np.array_equal(P.toarray() > 0, npts > 0)
    for form in case.forms:
        ncu, ncv = form.bfuns[0][1], form.bfuns[1][1]
        for layout in form.layouts:
            A = golden_csr(g, '%s_%s_%s' % (cid, form.name, layout))
            E = scipy.sparse.kron(P, np.ones((ncv, ncu)), format='csr') if layout == 'packed' else scipy.sparse.bmat([[P] * ncu] * ncv, format='csr')
            E.sort_indices()
            assert A.shape == E.shape
            assert np.array_equal(A.indptr, E.indptr) and np.array_equal(A.indices, E.indices), (cid, form.name, layout)


@pytest.mark.parametrize('cid', [c.id for c in pc.CASES])
def test_entry_model_matches_reference(cid, refs, golden):
    g, case, ref = golden('pair'), pc.BY_ID[cid], refs(cid)
    for form in case.forms:
        B = ref.blocks(form)
        for layout in form.layouts:
            A = golden_csr(g, '%s_%s_%s' % (cid, form.name, layout)).toarray()
            err = pm.rel_maxdiff(_layout(B, layout), A)
            print('%s %s %s: model vs reference %.2e' % (cid, form.name, layout, err))
            assert err <= RTOL, (cid, form.name, layout, err)
        # the picked entries / blocks of the reference's assembler object are entries of its matrix
        idx = g['%s_%s_idx' % (cid, form.name)].astype(np.int64)
        if form.bfuns[0][1] == form.bfuns[1][1] == 1:
            got = B[0][0][idx[:, 0], idx[:, 1]]
            want = g['%s_%s_entries' % (cid, form.name)]
        else:
            ncu, ncv = form.bfuns[0][1], form.bfuns[1][1]
            assert tuple(g['%s_%s_numcomp' % (cid, form.name)]) == (ncu, ncv)
            got = np.array([[[B[a][b][i, j] for b in range(ncu)] for a in range(ncv)] for i, j in idx]).reshape(len(idx), ncu, ncv)
            want = g['%s_%s_blocks' % (cid, form.name)]
        assert got.shape == want.shape and abs(got - want).max() <= RTOL * abs(want).max(), (cid, form.name)


def test_transposed_block_is_the_transpose(golden):
    """'p * div(v) * dx' over (kvs_p, kvs_u) equals the transpose of 'div(u) * p * dx' over (kvs_u, kvs_p) bit for bit."""
    g = golden('pair')
    A, T = golden_csr(g, 'th2_div_blocked'), golden_csr(g, 'th2t_divt_blocked')
    assert T.shape == A.shape[::-1] and (T != A.T).nnz == 0


def test_long_double_model_agrees_with_double(oracle, refs):
    case = pc.BY_ID['q1p0']
    hi = Ref(oracle, case, dtype=pm.LD)
    B, Bl = refs('q1p0').blocks(case.forms[0]), hi.blocks(case.forms[0])
    assert Bl[0][0].dtype == pm.LD and pm.rel_maxdiff(_layout(B, 'blocked'), _layout(Bl, 'blocked').astype(float)) <= 1e-14


def test_wrong_models_miss(oracle, refs, golden):
    """Mutation check: the trial tables used for both spaces, or the Gauss rule of the trial space alone (hi2: 3 instead of 5
    points per span), miss the reference by more than 1e-6."""
    g = golden('pair')
    for cid in ('th2', 'hi2', 'lo2'):
        case, ref = pc.BY_ID[cid], refs(cid)
        form = case.forms[0]
        A = golden_csr(g, '%s_%s_blocked' % (cid, form.name)).toarray()
        err = pm.rel_maxdiff(_layout(ref.blocks(form, Bv=ref.Bv_wrong), 'blocked'), A)
        print('%s: trial tables for both spaces: %.2e' % (cid, err))
        assert err > 1e-6, (cid, err)
    case = pc.BY_ID['hi2']
    q_trial = max(p for p, _, _ in case.trial) + 1
    assert q_trial == 3 and case.q() == 5
    low = Ref(oracle, case, q=q_trial)
    err = pm.rel_maxdiff(_layout(low.blocks(case.forms[0]), 'blocked'), golden_csr(g, 'hi2_full_blocked').toarray())
    print('hi2: Gauss rule of the trial space alone: %.2e' % err)
    assert err > 1e-6, err


def test_a_value_launch_spans_blocks_with_a_ragged_end(oracle):
    """Host arithmetic of the launch of k_pair_entries_csr (one thread per row and offset below the longest row, 128 per block):
    th3, hi2 and lo2 launch more than one block and their last block is not full (th2 fills 15 blocks exactly)."""
    hit = []
    for case in pc.CASES:
        ku, kv = case.kvs(oracle)
        nblocks, last = pc.csr_blocks(case.shape[0], pm.pattern(ku, kv)[2])
        if nblocks > 1 and last != pc.CSR_BLOCK:
            hit.append(case.id)
    assert hit == ['th3', 'hi2', 'lo2'], hit


def test_asym_1d_helpers(oracle, golden, monkeypatch):
    """bsp_mixed_deriv_biform_1d_asym and its two named cases against the reference at 1e-12.  Like every 1D matrix of the package
    they evaluate the basis on the device; here the two evaluation calls are replaced by the oracle's, so that the assembly around
    them is what is checked (tests/test_pair_gpu.py runs them as they are)."""
    from pyiga_amd import assemble, bspline
    monkeypatch.setattr(bspline, 'active_deriv', lambda kv, u, nd: oracle.active_deriv(oracle.KnotVector(kv.kv, kv.p), u, nd))
    monkeypatch.setattr(bspline, 'findspans', lambda kv, u: oracle.first_active(oracle.KnotVector(kv.kv, kv.p), u) + kv.p)
    g = golden('pair')
    kv1, kv2 = bspline.make_knots(3, 0., 1., 4, mult=2), bspline.make_knots(2, 0., 1., 4)
    assert np.array_equal(kv1.kv, g['asym_kv1']) and np.array_equal(kv2.kv, g['asym_kv2'])
    for du in (0, 1):
        for dv in (0, 1):
            A = assemble.bsp_mixed_deriv_biform_1d_asym(kv1, kv2, du, dv)
            ref = g['asym_%d%d' % (du, dv)]
            assert A.shape == ref.shape == (kv2.numdofs, kv1.numdofs)
            assert abs(A.toarray() - ref).max() <= RTOL * abs(ref).max(), (du, dv)
    assert abs(assemble.bsp_mass_1d_asym(kv1, kv2).toarray() - g['asym_00']).max() <= RTOL * abs(g['asym_00']).max()
    assert abs(assemble.bsp_stiffness_1d_asym(kv1, kv2).toarray() - g['asym_11']).max() <= RTOL * abs(g['asym_11']).max()


def test_normalise_bfuns_keeps_the_space():
    from pyiga_amd import tforms
    assert tforms.normalise_bfuns('div(u) * p * dx', [('u', 2, 0), ('p', 1, 1)]) == [('u', 2, 0), ('p', 1, 1)]
    assert tforms.normalise_bfuns('u * v * dx', None) == [('u', 1, 0), ('v', 1, 0)]
    assert tforms.normalise_bfuns('x', ['w', ('z', 3)]) == [('w', 1, 0), ('z', 3, 0)]
    with pytest.raises(ValueError):
        tforms.normalise_bfuns('x', [('u', 1, 2)])


def test_refusals_need_no_device(monkeypatch):
    """The role rule, unequal meshes, boundary= and symmetric=True with two spaces are refused before any device object exists."""
    from pyiga_amd import assemble, assemblers, bspline, geometry, form_assemblers

    def no_device(*a, **k):
        raise AssertionError('a device object was created')
    monkeypatch.setattr(assemblers.DevicePatch, '__init__', no_device)
    monkeypatch.setattr(form_assemblers, 'DevicePatch', no_device)
    monkeypatch.setattr(form_assemblers, 'DevicePair', no_device)
    mk = bspline.make_knots
    ku, kp = (mk(3, 0., 1., 4, mult=2), mk(3, 0., 1., 3, mult=2)), (mk(2, 0., 1., 4), mk(2, 0., 1., 3))
    geo = geometry.quarter_annulus()
    th = [('u', 2, 0), ('p', 1, 1)]
    with pytest.raises(ValueError, match='other order'):
        assemble.assemble('div(u) * p * dx', (kp, ku), bfuns=[('u', 2, 1), ('p', 1, 0)], geo=geo)
    with pytest.raises(ValueError, match='other order'):
        assemble.instantiate_assembler('p * div(v) * dx', (ku, kp), dict(geo=geo), [('p', 1, 1), ('v', 2, 0)])
    with pytest.raises(ValueError, match='different meshes'):
        assemble.assemble('div(u) * p * dx', (ku, (mk(2, 0., 1., 4), mk(2, 0., 1., 4))), bfuns=th, geo=geo)
    with pytest.raises(ValueError, match='different dimensions'):
        assemble.assemble('div(u) * p * dx', (ku, kp + (kp[0],)), bfuns=th, geo=geo)
    with pytest.raises(NotImplementedError, match='boundary'):
        assemble.assemble('u * p * ds', (ku, kp), bfuns=[('u', 1, 0), ('p', 1, 1)], geo=geo, boundary='left')
    with pytest.raises(NotImplementedError, match='surface'):
        assemble.assemble('u * p * ds', (ku, kp), bfuns=[('u', 1, 0), ('p', 1, 1)], geo=geo)
    with pytest.raises(ValueError, match='symmetric'):
        assemble.assemble('u * p * dx', (ku, kp), bfuns=[('u', 1, 0), ('p', 1, 1)], geo=geo, symmetric=True)
    with pytest.raises(ValueError, match='only one space'):
        assemble.assemble('u * p * dx', ku, bfuns=[('u', 1, 0), ('p', 1, 1)], geo=geo)
    # what IS accepted, as roles: trial in space 0 and test in space 1; every function in one space
    assert form_assemblers.space_roles((ku, kp), 'div(u) * p * dx', th) == (ku, kp)
    assert form_assemblers.space_roles((ku, kp), 'u * v * dx', [('u', 1, 1), ('v', 1, 1)]) == (kp, None)
    assert form_assemblers.space_roles((ku, kp), 'u * v * dx', None) == (ku, None)
    assert form_assemblers.space_roles(ku, 'u * v * dx', None) == (ku, None)


def test_pair_abi():
    """Every igx_pair_* entry point is declared in the header, bound in _lib.py and exported by the built library."""
    import __graft_entry__ as ge
    from pyiga_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    want = {'igx_pair_create', 'igx_pair_destroy', 'igx_pair_get_info', 'igx_pair_pattern', 'igx_pair_assemble', 'igx_pair_entries',
            'igx_pair_d_data', 'igx_pair_last_timing'}
    hdr = open(os.path.join(ROOT, 'include', 'igx.h')).read()
    assert {n for n in re.findall(r'\b(igx_pair_[a-z_0-9]+)\s*\(', hdr)} == want
    assert {n for n, _, _ in _lib.SYMBOLS if n.startswith('igx_pair_')} == want
    nm = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in want:
        assert re.search(r'\bT %s\b' % name, nm), name
    cdll = _lib.load()
    assert cdll.igx_version() == 101
    assert cdll.igx_pair_create(None, 2, None, None, None) is None and b'null argument' in cdll.igx_last_error()
    src = ('#include <stdio.h>\n#include "igx.h"\nint main(){printf("%zu\\n", sizeof(igx_pair_info)); return 0;}')
    import ctypes
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, 's.c'), 'w').write(src)
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), os.path.join(tmp, 's.c'), '-o', os.path.join(tmp, 's')])
        assert int(subprocess.check_output([os.path.join(tmp, 's')], text=True)) == ctypes.sizeof(_lib.PairInfo)

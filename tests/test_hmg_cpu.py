"""Local multigrid on hierarchical spline spaces, host side (no device): the index sets and prolongators of ``HSpace`` against
the reference (tests/golden/golden_hmg.npz), and the host model of the cycle (tests/_hmg_model.py) against the reference's
iterates -- which is what entitles the model to judge the device in tests/test_hmg_gpu.py.
"""
import numpy as np
import pytest
import scipy.sparse

import _hier_cases as hc
import _hmg_cases as mc
import _hmg_model as mm
from _hmg_fixtures import G, TOL12, chain, golden_prolongators, model_run, problem, space


@pytest.mark.parametrize('name', mc.SPACE_CASES)
def test_index_sets_equal_reference(name):
    hs = space(name)
    for fam in mc.FAMILIES:
        got = mc.pack_family(getattr(hs, fam + '_indices')(), hs.dim)
        assert np.array_equal(got, G['%s_%s' % (name, fam)]), fam
        flat, off = mc.pack_lists(hs.indices_to_smooth(fam))
        assert np.array_equal(flat, G['%s_smooth_%s' % (name, fam)]) and np.array_equal(off, G['%s_smooth_%s_off' % (name, fam)]), fam
    assert np.array_equal(mc.pack_family(hs.global_indices(), hs.dim), G[name + '_global'])
    assert np.array_equal(mc.pack_family(hs.cell_supp_indices(remove_dirichlet=False), hs.dim), G[name + '_cell_supp_all'])
    # one virtual level alone, and the conversion of ravelled indices
    lv = hs.numlevels - 1
    assert hs.global_indices(vlvl=lv) == hs.global_indices()[lv]
    new = hs.ravel_indices(hs.new_indices()[lv])
    assert np.array_equal(hs.raveled_to_virtual_canonical_indices(lv, new), hs.indices_to_smooth('new')[lv])


@pytest.mark.parametrize('name', mc.SPACE_CASES)
def test_prolongators_equal_reference(name):
    hs = space(name)
    Ps, ref = hs.virtual_hierarchy_prolongators(), golden_prolongators(name)
    assert len(Ps) == len(ref) == hs.numlevels - 1
    for P, R in zip(Ps, ref):
        assert scipy.sparse.issparse(P) and P.shape == R.shape
        assert hc.rel_maxdiff(P, R) <= TOL12
    # the other basis: a THB prolongator is the HB one with the inverse truncation of its level applied
    other = hs.virtual_hierarchy_prolongators(truncate=not hs.truncate)
    hb, thb = (other, Ps) if hs.truncate else (Ps, other)
    for k, (Ph, Pt) in enumerate(zip(hb, thb)):
        assert hc.rel_maxdiff(hs.truncate_one_level(k, num_rows=Ph.shape[0], inverse=True) @ Ph, Pt) <= TOL12


def test_smoothing_strategy_is_checked():
    with pytest.raises(AssertionError):
        space('hb2').indices_to_smooth('everything')
    with pytest.raises(ValueError):
        hs = space('hb2')
        hs.raveled_to_virtual_canonical_indices(0, hs.ravel_indices(hs.new_indices()[1]))


def test_python_colouring_equals_library():
    """The model's first-fit colouring is the library's host colouring (no device needed) on every level of two hierarchies."""
    from pyiga_amd import solvers
    for name, strategy in (('thb2', 'cell_supp'), ('hb3', 'new')):
        A, _, Ps, _ = problem(name)
        As = chain(name)
        inds = space(name).indices_to_smooth(strategy)
        for l in range(1, len(As)):
            rows, nc = mm.colour_order(As[l], inds[l])
            got_rows, coff = solvers.colour_order(As[l].indptr, As[l].indices, inds[l])
            assert np.array_equal(rows, got_rows) and coff.size - 1 == nc and coff[-1] == len(inds[l])


def test_long_double_triple_product():
    """The long-double product agrees with scipy's double one on a level of a THB chain, keeps structural zeros explicitly, and
    is exact on small integers."""
    A, _, Ps, _ = problem('thb2inf')
    C = mm.rap_longdouble(A, Ps[-1])
    assert hc.rel_maxdiff(C, Ps[-1].T @ A @ Ps[-1]) <= TOL12
    P = scipy.sparse.csr_matrix(np.array([[1.0, 0.0], [1.0, 1.0], [0.0, -1.0]]))
    B = scipy.sparse.csr_matrix(np.array([[2.0, 1.0, 0.0], [1.0, 2.0, 1.0], [0.0, 1.0, 1.0]]))
    C = mm.rap_longdouble(B, P)
    assert np.array_equal(C.toarray(), (P.T @ B @ P).toarray()) and C.nnz == 4


@pytest.mark.parametrize('row', mc.SOLVE_ROWS, ids=mc.row_key)
def test_model_reproduces_reference(row):
    """In the reference's own order the model gives the reference's iterates 1 and 2 and its iteration count."""
    key = mc.row_key(row)
    xs, ratios = model_run(row, False)
    assert len(ratios) == int(G[key + '_its'])
    for k, ref in ((0, G[key + '_x1']), (1, G[key + '_x2'])):
        assert abs(xs[k] - ref).max() / abs(ref).max() <= TOL12, k


@pytest.mark.parametrize('row', mc.SOLVE_ROWS, ids=mc.row_key)
def test_colour_order_is_admissible(row):
    """In colour order the model converges, and its last two residual ratios keep clear of the tolerance by 1 %: rounding of the
    device (about 1e-12 relative) cannot move the iteration count tests/test_hmg_gpu.py asserts."""
    _, ratios = model_run(row, True)
    assert len(ratios) >= 2 and ratios[-1] <= 0.99 * mc.TOL, ratios[-3:]
    assert ratios[-2] >= 1.01 * mc.TOL, ratios[-3:]
    print(mc.row_key(row), 'reference', int(G[mc.row_key(row) + '_its']), 'colour order', len(ratios), 'last ratios %.3e %.3e' % (ratios[-2], ratios[-1]))

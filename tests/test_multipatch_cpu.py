"""Multipatch host API without a GPU: dof slices, Greville points, boundary conditions combined, control-net transforms and the
numbering of the L-shape of the reference's test_multipatch (pyiga test/test_assemble.py:508-560), against arrays made with
the reference (tests/golden/make_golden_multipatch.py)."""
import os

import numpy as np
import pytest
import scipy.sparse

from pyiga_amd import assemble, bspline, geometry

GOLD = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'golden_multipatch.npz'))


def _lshape():
    kvs = 2 * (bspline.make_knots(2, 0.0, 1.0, 8),)
    squ = geometry.unit_square()
    geos = (squ, squ.translate((1, 0)), squ.scale((-1, 1)).translate((2, 1)))
    MP = assemble.Multipatch([(kvs, g) for g in geos])
    MP.join_boundaries(0, 'right', 1, 'left')
    MP.join_boundaries(1, 'top', 2, 'bottom', flip=(True,))
    MP.finalize()
    return MP


SLICES = [(0, 0, (4, 5), None), (1, -1, (4, 5), (True,)), (2, 0, (3, 4, 5), (True, False)),
          (1, -1, (3, 4, 5), (False, True)), (0, -1, (3, 4, 5), (True, True))]


@pytest.mark.parametrize('k', range(len(SLICES)))
def test_slice_indices(k):
    ax, idx, shape, flip = SLICES[k]
    assert np.array_equal(assemble.slice_indices(ax, idx, shape, flip=flip), GOLD['slice%d_mi' % k])
    assert np.array_equal(assemble.slice_indices(ax, idx, shape, ravel=True, flip=flip), GOLD['slice%d_rav' % k])


def test_slice_indices_flip_order():
    # bottom row of a 3 x 4 grid traversed backwards
    assert np.array_equal(assemble.slice_indices(0, 0, (3, 4), ravel=True, flip=(True,)), [3, 2, 1, 0])
    assert np.array_equal(assemble.slice_indices(1, -1, (3, 4), ravel=True), [3, 7, 11])


def test_boundary_dofs():
    kvs3 = (bspline.make_knots(2, 0.0, 1.0, 3), bspline.make_knots(1, 0.0, 1.0, 4), bspline.make_knots(3, 0.0, 1.0, 2))
    for k, (bd, flip) in enumerate([('left', None), ('top', (True, False)), ((0, 1), (False, True)), ('back', None)]):
        assert np.array_equal(assemble.boundary_dofs(kvs3, bd, ravel=True, flip=flip), GOLD['bdofs%d' % k]), bd
    kvs = 2 * (bspline.make_knots(2, 0.0, 1.0, 8),)
    assert np.array_equal(assemble.boundary_dofs(kvs, 'right', ravel=True), np.arange(9, 100, 10))
    assert np.array_equal(assemble.boundary_dofs(kvs, (0, 0)), np.stack((np.zeros(10, int), np.arange(10)), axis=1))


def test_greville():
    kvs = [bspline.make_knots(3, 0.0, 1.0, 7), bspline.make_knots(2, -1.0, 2.0, 5, mult=2),
           bspline.make_knots(1, 0.0, 1.0, 4), bspline.KnotVector(np.array([0, 0, 0, .1, .5, .5, 1, 1, 1.]), 2)]
    for k, kv in enumerate(kvs):
        g = kv.greville()
        assert g.shape == (kv.numdofs,)
        assert np.allclose(g, GOLD['grev%d' % k], rtol=0, atol=1e-15)


def test_combine_bcs():
    idx, val = assemble.combine_bcs([(np.array([5, 1, 3]), np.array([.5, .1, .3])), (np.array([3, 7, 1]), np.array([3., 7., 1.]))])
    assert np.array_equal(idx, GOLD['comb_idx']) and np.array_equal(val, GOLD['comb_val'])
    assert np.array_equal(idx, [1, 3, 5, 7]) and np.array_equal(val, [.1, .3, .5, 7.])


def test_control_net_transforms():
    B = geometry.unit_square().translate((1, 2)).scale((-1, 3)).rotate_2d(0.3)
    assert np.allclose(B.coeffs, GOLD['tr_bspl'], rtol=0, atol=1e-15)
    N = geometry.quarter_annulus().rotate_2d(np.pi).translate((-1, 3)).scale(2.0)
    assert isinstance(N, geometry.NurbsFunc)
    # homogeneous control net (weighted points, weights) as in the reference
    assert np.allclose(N.coeffs, GOLD['tr_nurbs'], rtol=0, atol=1e-14)
    M = geometry.quarter_annulus().apply_matrix(np.array([[0.0, 1.0], [1.0, 0.0]]))
    C0, W0 = geometry.quarter_annulus().coeffs_weights()
    assert np.array_equal(M.coeffs_weights()[1], W0) and np.allclose(M.coeffs_weights()[0], C0[..., ::-1])


def test_identity_geometry():
    kv = bspline.make_knots(2, -1.0, 3.0, 4)
    G = geometry.identity([kv, (0.5, 2.0)])
    assert G.sdim == 2 and G.dim == 2
    assert G.support == ((-1.0, 3.0), (0.5, 2.0))
    assert np.allclose(G.coeffs[0, 0], [0.5, -1.0]) and np.allclose(G.coeffs[-1, -1], [2.0, 3.0])


def test_lshape_numbering():
    MP = _lshape()
    assert MP.numpatches == 3
    assert MP.numdofs == 90 + 81 + 90 + 2 * 10 - 1 == GOLD['L_numdofs']
    idx1 = MP.patch_to_global_idx(1)
    assert idx1.size == 100
    idx1 = idx1.reshape((10, 10))
    assert np.array_equal(idx1[:-1, 1:].ravel(), 90 + np.arange(9 * 9))
    assert np.array_equal(idx1[:, 0], 90 + 81 + 90 + np.arange(10))
    assert np.array_equal(idx1[-1, 1:], 90 + 81 + 90 + 10 + np.arange(9))
    for p in range(3):
        assert np.array_equal(MP.patch_to_global_idx(p), GOLD['L_p2g%d' % p])
        P = MP.patch_to_global(p)
        assert scipy.sparse.linalg.norm(MP.global_to_patch(p) @ P - scipy.sparse.eye(100)) == 0
        assert MP.patch_to_global(p, j_global=True).shape == (MP.numdofs, 300)
    u1 = np.arange(100)
    ug = MP.patch_to_global(1) @ u1
    u2 = (MP.global_to_patch(2) @ ug).reshape((10, 10))
    assert np.allclose(u2[1:, :], 0) and np.array_equal(u2[0, :], np.arange(99, 89, -1))
    assert MP.injective


def test_non_injective_join_numbering():
    kvs = 2 * (bspline.make_knots(1, 0.0, 1.0, 2),)
    MP = assemble.Multipatch([(kvs, geometry.unit_square()), (kvs, geometry.unit_square().translate((1, 0)))])
    MP.join_dofs(0, [2], 1, [0])
    MP.join_dofs(1, [0], 0, [8])
    MP.finalize()
    idx0 = MP.patch_to_global_idx(0)
    assert idx0[2] == idx0[8] == MP.M_ofs[-1]
    assert MP.numdofs == 9 + 9 - 2 and not MP.injective


def test_vector_valued_multipatch_rejected():
    MP = _lshape()
    with pytest.raises(NotImplementedError):
        MP.assemble_system('inner(grad(u),grad(v))*dx', 'v*dx', bfuns=[('u', 2), ('v', 2)])

"""igx_patch_eval_spline_d (csrc/kern_spline.hip): a spline of the patch's own space, given by a device dof vector, at the
resident Gauss points -- against numpy with dense collocation matrices at the patch's own Gauss nodes.

Tolerances are derived, not fitted: an output is a sum of at most P^dim <= 216 products V_0 V_1 V_2 c, so its rounding error is
below  250 eps max|c| prod_k S_k  with  S_k = max_g sum_l |V_k[g][l][d_k]|  (d_k: the derivative order taken on axis k), computed
here from the tables.  A physical gradient is J^-T times the parametric one: the same bound times dim * max |J^-1|."""
import numpy as np
import pytest

from pyiga_amd import _lib, assemblers, bspline, geometry

import _lv_cases as lc

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


def _double_knot(kv):
    """The same mesh with one interior knot repeated: the first active index is no longer span + const there."""
    k = kv.kv[kv.p + 2]
    return bspline.KnotVector(np.sort(np.append(kv.kv, k)), kv.p)


def _kvs(degrees, spans, double=()):
    kvs = []
    for k, (p, n) in enumerate(zip(degrees, spans)):
        kv = bspline.make_knots(p, 0.0, 1.0, n)
        kvs.append(_double_knot(kv) if k in double else kv)
    return tuple(kvs)


# name -> (degrees, spans, axes with a double interior knot)
SHAPES = {
    '3d_p1': ((1, 1, 1), (3, 2, 4), ()), '3d_p2': ((2, 2, 2), (3, 2, 4), ()), '3d_p3': ((3, 3, 3), (3, 2, 4), ()),
    '3d_p4': ((4, 4, 4), (3, 2, 4), ()), '3d_p5': ((5, 5, 5), (3, 2, 4), ()),
    '3d_mixed_double': ((2, 3, 1), (3, 5, 4), (1, 2)),
    '3d_manylines': ((1, 1, 1), (91, 91, 1), ()),               # 182 x 182 = 33124 grid lines: a wave walks two lines, reusing its LDS
    '3d_last65': ((1, 1, 1), (2, 2, 64), ()), '3d_last129': ((1, 1, 1), (2, 2, 128), ()),     # lane passes beyond 64 dofs
    '3d_onespan0': ((2, 2, 2), (1, 3, 2), ()), '3d_onespan1': ((2, 2, 2), (3, 1, 2), ()), '3d_onespan2': ((2, 2, 2), (3, 2, 1), ()),
    '2d_p3': ((3, 3), (5, 5), ()), '2d_p14': ((1, 4), (5, 5), ()),
    '2d_last129': ((1, 1), (2, 128), ()), '2d_double': ((3, 2), (4, 5), (0, 1)),
}


def _geo(name, dim):
    if name == 'identity':
        return geometry.unit_square() if dim == 2 else geometry.unit_cube()
    return geometry.quarter_annulus() if dim == 2 else geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.quarter_annulus())


def _dense_tables(kv, nodes):
    """(2, G, N): values and first derivatives of every basis function at the nodes."""
    first, vals = bspline.collocation_derivs_info(kv, nodes, derivs=1)          # (2, G, p + 1)
    M = np.zeros((2, nodes.shape[0], kv.numdofs))
    cols = first[:, None] + np.arange(kv.p + 1)[None, :]
    rows = np.broadcast_to(np.arange(nodes.shape[0])[:, None], cols.shape)
    for d in range(2):
        M[d][rows, cols] = vals[d]
    return M


def _expand(Ms, orders, c):
    out = c
    for k, (M, d) in enumerate(zip(Ms, orders)):
        out = np.moveaxis(np.tensordot(M[d], out, axes=(1, k)), 0, k)
    return out


def _reference(patch, kvs, geo, c):
    dim = len(kvs)
    grid = tuple(patch.gauss(k)[0] for k in range(dim))
    Ms = [_dense_tables(kv, g) for kv, g in zip(kvs, grid)]
    S = [[abs(M[d]).sum(axis=1).max() for d in range(2)] for M in Ms]
    cmax = abs(c).max()
    val = _expand(Ms, (0,) * dim, c)
    tol_val = 250 * EPS * cmax * np.prod([S[k][0] for k in range(dim)])
    # parametric gradient in (x, y, z) order: x belongs to the LAST grid axis
    gpar, tol_d = [], []
    for r in range(dim):
        ax = dim - 1 - r
        orders = tuple(1 if k == ax else 0 for k in range(dim))
        gpar.append(_expand(Ms, orders, c))
        tol_d.append(250 * EPS * cmax * np.prod([S[k][orders[k]] for k in range(dim)]))
    gpar = np.stack(gpar, axis=-1)
    J = geo.grid_jacobian(grid)                                                   # G + (dim, dim): d G_r / d xi_c, c in (x, y, z) order
    gphys = np.linalg.solve(np.swapaxes(J, -1, -2), gpar[..., None])[..., 0]
    tol_phys = max(tol_d) * dim * abs(np.linalg.inv(J)).max()
    return val, tol_val, gpar, tol_d, gphys, tol_phys


# A dense 3x3 matrix, all nine entries non-zero and of distinct magnitude, det A = 0.94: the Jacobian of the mapped cube has no
# zero entry, so every cofactor of the kernel's inverse matters (line x annulus has four zero entries: a swapped index in five of
# the nine cofactors cannot show there)
DENSE_A = np.array([[1.0, 0.3, -0.22], [0.15, 0.9, 0.25], [-0.1, 0.2, 1.2]])
SHEAR_A = np.array([[1.1, 0.35], [-0.2, 0.8]])


def _dense_geo(name, dim):
    """'affine': the unit cube's (square's) multilinear control net mapped by DENSE_A (SHEAR_A); 'bent': the same with a
    multiquadratic net and the interior control point moved."""
    A = DENSE_A if dim == 3 else SHEAR_A
    if name == 'affine':
        return (geometry.unit_cube() if dim == 3 else geometry.unit_square()).apply_matrix(A)
    kv = bspline.make_knots(2, 0.0, 1.0, 1)
    g = np.array([0.0, 0.5, 1.0])
    pts = np.stack(np.meshgrid(*(dim * (g,)), indexing='ij')[::-1], axis=-1)          # (x, y, z) order: x belongs to the last axis
    ctrl = pts @ A.T
    ctrl[(1,) * dim] += np.array([0.1, -0.07, 0.05])[:dim]
    return bspline.BSplineFunc(dim * (kv,), ctrl)


def _check_against_numpy(kvs, geo, tag, seed, affine=None):
    dim = len(kvs)
    patch = assemblers.DevicePatch(kvs, geo)
    try:
        rng = np.random.default_rng(seed)
        c = rng.uniform(-1.0, 1.0, size=tuple(kv.numdofs for kv in kvs))
        val, tol_val, gpar, tol_d, gphys, tol_phys = _reference(patch, kvs, geo, c)
        d_c = patch.upload_dofs(c)
        only = patch.eval_spline(d_c, want_grad=False, to_host=True)
        assert only.shape == (1,) + val.shape
        err0 = abs(only[0] - val).max()
        full = patch.eval_spline(d_c, want_grad=True, to_host=True)
        assert full.shape == (1 + dim,) + val.shape
        err1 = abs(full[0] - val).max()
        errg = abs(np.moveaxis(full[1:], 0, -1) - gphys).max()
        print('%s: value %.2e / %.2e (tol %.2e)  gradient %.2e (tol %.2e)' % (tag, err0, err1, tol_val, errg, tol_phys))
        assert err0 <= tol_val and err1 <= tol_val
        assert np.array_equal(only[0], full[0]), 'the value does not depend on whether the gradient is asked for'
        assert errg <= tol_phys
        if affine is not None:            # J = A everywhere: the gradient is A^-T times the parametric one, in numpy alone
            Ainv = np.linalg.inv(affine)
            gA = np.einsum('cr,...c->...r', Ainv, gpar)
            assert abs(np.moveaxis(full[1:], 0, -1) - gA).max() <= max(tol_d) * dim * abs(Ainv).max()
        return full, gpar, tol_d
    finally:
        patch.close()


@pytest.mark.parametrize('geo_name', ['identity', 'annulus'])
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_spline_eval_against_numpy(shape, geo_name):
    degrees, spans, double = SHAPES[shape]
    kvs = _kvs(degrees, spans, double)
    dim = len(kvs)
    full, gpar, tol_d = _check_against_numpy(kvs, _geo(geo_name, dim), '%s %s' % (shape, geo_name), 1234 + len(shape))
    if geo_name == 'identity':        # J = I: the outputs ARE the parametric derivatives, each within its own bound
        for r in range(dim):
            assert abs(full[1 + r] - gpar[..., r]).max() <= dim * tol_d[r]


@pytest.mark.parametrize('geo_name', ['affine', 'bent'])
@pytest.mark.parametrize('shape', ['3d_p2', '3d_mixed_double', '3d_last129', '2d_double'])
def test_spline_eval_with_a_dense_jacobian(shape, geo_name):
    """A geometry whose Jacobian has no zero entry: every cofactor of the inverse in k_spline12 enters the gradient."""
    degrees, spans, double = SHAPES[shape]
    kvs = _kvs(degrees, spans, double)
    dim = len(kvs)
    geo = _dense_geo(geo_name, dim)
    grid = tuple(np.array([0.3, 0.8]) for _ in range(dim))
    assert (abs(geo.grid_jacobian(grid)) > 0.05).all()
    A = (DENSE_A if dim == 3 else SHEAR_A) if geo_name == 'affine' else None
    _check_against_numpy(kvs, geo, '%s %s' % (shape, geo_name), 4321 + len(shape), affine=A)


@pytest.mark.parametrize('sid', [c.id for c in lc.SPLINE_CASES])
def test_spline_launch_shapes(sid):
    """The launch shapes of k_spline12 the other cases do not reach (tests/_lv_cases.py restates spline12_waves and lpw, and
    tests/test_lv_coverage_cpu.py ties the restatement to the source): a wave walking 8 lines, blocks of 2 and of 1 wave, and the
    refusal on the host when not even one wave's lines fit the LDS (nothing is launched; the patch serves the value afterwards)."""
    case = lc.SPLINE_BY_ID[sid]
    kvs = _kvs(case.degrees, case.spans)
    dim = case.dim
    assert kvs[-1].numdofs == case.nlast()
    geo = _geo('identity', dim)
    if case.waves > 0:
        full, gpar, tol_d = _check_against_numpy(kvs, geo, sid, 99 + len(sid))
        for r in range(dim):
            assert abs(full[1 + r] - gpar[..., r]).max() <= dim * tol_d[r]
        return
    patch = assemblers.DevicePatch(kvs, geo)
    try:
        c = np.random.default_rng(11).uniform(-1.0, 1.0, size=tuple(kv.numdofs for kv in kvs))
        d_c = patch.upload_dofs(c)
        with pytest.raises(_lib.IgxError) as e:
            patch.eval_spline(d_c, want_grad=True)
        assert e.value.code == _lib.IGX_ERR_UNSUPPORTED
        val, tol_val = _reference(patch, kvs, geo, c)[:2]
        assert abs(patch.eval_spline(d_c, want_grad=False, to_host=True)[0] - val).max() <= tol_val
    finally:
        patch.close()


def test_row_slab_is_refused():
    kvs = _kvs((2, 2, 2), (4, 2, 2))
    patch = assemblers.DevicePatch(kvs, geometry.unit_cube(), row0=(0, 3))
    try:
        lib = _lib.load()
        n = int(np.prod([kv.numdofs for kv in kvs]))
        d_c = patch._dev_buffer('_d_dofs', 8 * n)
        d_o = patch._dev_buffer('_d_spl', 8 * patch.resident_points() * 4)
        import ctypes as C
        ptrs = (C.c_void_p * 4)(d_o, None, None, None)
        assert lib.igx_patch_eval_spline_d(patch.handle, d_c, 0, ptrs) == _lib.IGX_ERR_UNSUPPORTED
    finally:
        patch.close()


def test_jacobian_geometry_serves_the_value_only():
    kvs = _kvs((2, 1), (3, 4))
    geo = geometry.quarter_annulus()
    spl = assemblers.DevicePatch(kvs, geo)
    grid = tuple(spl.gauss(k)[0] for k in range(2))
    spl.close()
    patch = assemblers.DevicePatch(kvs, geo, jacobian=geo.grid_jacobian(grid))
    try:
        rng = np.random.default_rng(7)
        c = rng.uniform(-1.0, 1.0, size=tuple(kv.numdofs for kv in kvs))
        d_c = patch.upload_dofs(c)
        val, tol_val = _reference(patch, kvs, geo, c)[:2]
        assert abs(patch.eval_spline(d_c, want_grad=False, to_host=True)[0] - val).max() <= tol_val
        with pytest.raises(_lib.IgxError) as e:
            patch.eval_spline(d_c, want_grad=True)
        assert e.value.code == _lib.IGX_ERR_UNSUPPORTED
    finally:
        patch.close()

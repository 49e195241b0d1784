"""igx_patch_eval_vspline_d (csrc/kern_spline.hip, k_vspline12): nc = 2 or 3 splines of the patch's own space, their dofs
component-major in one device vector, at the resident Gauss points in one pass.

Two yardsticks per case: numpy with dense collocation matrices within the bound derived in test_spline_eval_gpu.py
(250 eps max|c| prod_k S_k, times dim max|J^-1| for the physical gradient), and the scalar call igx_patch_eval_spline_d on every
component's dofs, which the fused kernel must reproduce bit for bit, value and gradient."""
import ctypes as C

import numpy as np
import pytest

from pyiga_amd import _lib, assemblers, geometry

import test_spline_eval_gpu as se

pytestmark = pytest.mark.gpu

# the shapes of test_spline_eval_gpu.py (degrees 1 to 5, mixed degrees with a double interior knot on the mid and on the last axis,
# 65 and 129 dofs on the last axis, one span per axis in turn, enough lines that a wave walks two) and last axes so long that
# fewer than four waves' lines fit the LDS: 3 components with the gradient hold 9 lines of N doubles per wave, so 301 dofs leave
# room for 2 waves and 501 for 1
SHAPES = dict(se.SHAPES)
SHAPES.update({'3d_last301': ((1, 1, 1), (1, 1, 300), ()), '3d_last501': ((1, 1, 1), (1, 1, 500), ()),
               '2d_last1024': ((1, 1), (1, 1023), ())})
LDS_BYTES = 64 * 1024


def _waves(dim, nc, grad, nlast):
    per_wave = nc * (dim if grad else 1) * nlast * 8
    for w in (4, 2, 1):
        if w * per_wave <= LDS_BYTES:
            return w
    return 0


def test_the_wave_counts_the_shapes_are_meant_to_reach():
    assert _waves(3, 3, True, 301) == 2 and _waves(3, 3, True, 501) == 1 and _waves(3, 2, True, 301) == 4
    assert _waves(2, 3, True, 1024) == 1 and _waves(2, 2, True, 1024) == 2 and _waves(2, 2, False, 1024) == 4
    assert _waves(3, 3, True, 1001) == 0 and _waves(3, 3, False, 1001) == 2


def _upload(patch, c):
    c = np.ascontiguousarray(c, dtype=np.float64)
    ptr = patch._dev_buffer('_d_vdofs', c.nbytes)
    _lib.check(_lib.load().igx_dev_upload(patch.ctx.handle, ptr, c.ctypes.data, c.nbytes), 'igx_dev_upload')
    return ptr


def _check(kvs, geo, nc, tag, seed):
    dim = len(kvs)
    patch = assemblers.DevicePatch(kvs, geo)
    try:
        rng = np.random.default_rng(seed)
        c = rng.uniform(-1.0, 1.0, size=(nc,) + tuple(kv.numdofs for kv in kvs))
        c[1] *= 37.0                                   # (components of different size: a swapped component shows in the bound)
        d_c = _upload(patch, c)
        only = patch.eval_vspline(d_c, nc, want_grad=False, to_host=True)
        full = patch.eval_vspline(d_c, nc, want_grad=True, to_host=True)
        assert only.shape[0] == nc and full.shape[0] == nc * (1 + dim)
        for k in range(nc):
            val, tol_val, gpar, tol_d, gphys, tol_phys = se._reference(patch, kvs, geo, c[k])
            grad = np.moveaxis(full[nc + k * dim:nc + (k + 1) * dim], 0, -1)
            err0, err1, errg = abs(only[k] - val).max(), abs(full[k] - val).max(), abs(grad - gphys).max()
            print('%s nc=%d component %d: value %.2e / %.2e (tol %.2e)  gradient %.2e (tol %.2e)' % (tag, nc, k, err0, err1, tol_val, errg, tol_phys))
            assert err0 <= tol_val and err1 <= tol_val and errg <= tol_phys
            d_k = patch.upload_dofs(c[k])
            scalar = patch.eval_spline(d_k, want_grad=True, to_host=True)
            assert np.array_equal(full[k], scalar[0]) and np.array_equal(only[k], scalar[0]), 'value bits of component %d' % k
            for r in range(dim):
                assert np.array_equal(full[nc + k * dim + r], scalar[1 + r]), 'gradient bits of component %d, partial %d' % (k, r)
            assert np.array_equal(patch.eval_spline(d_k, want_grad=False, to_host=True)[0], only[k])
    finally:
        patch.close()


@pytest.mark.parametrize('nc', [2, 3])
@pytest.mark.parametrize('geo_name', ['identity', 'annulus'])
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_vspline_against_numpy_and_the_scalar_call(shape, geo_name, nc):
    degrees, spans, double = SHAPES[shape]
    kvs = se._kvs(degrees, spans, double)
    _check(kvs, se._geo(geo_name, len(kvs)), nc, '%s %s' % (shape, geo_name), 777 + len(shape) + nc)


@pytest.mark.parametrize('nc', [2, 3])
@pytest.mark.parametrize('geo_name', ['affine', 'bent'])
@pytest.mark.parametrize('shape', ['3d_mixed_double', '2d_double'])
def test_vspline_with_a_dense_jacobian(shape, geo_name, nc):
    """Every cofactor of the inverse the kernel forms once per point enters the gradient of every component."""
    degrees, spans, double = SHAPES[shape]
    kvs = se._kvs(degrees, spans, double)
    _check(kvs, se._dense_geo(geo_name, len(kvs)), nc, '%s %s' % (shape, geo_name), 31 + nc)


def _raw_call(patch, nc, want_grad, n_out=12, d_c='dofs', whole=True):
    """The return code of the plain call; `whole` False: a patch that is refused before anything is read or written (its output
    pointers need only be non-null)."""
    lib = _lib.load()
    n = int(np.prod([kv.numdofs for kv in patch.kvs]))
    d_dofs = patch._dev_buffer('_d_vdofs', 8 * 3 * n)
    npts = patch.resident_points() if whole else 1
    base = patch._dev_buffer('_d_vspl', 8 * npts * 12)
    ptrs = (C.c_void_p * 12)()
    for k in range(n_out):
        ptrs[k] = base + 8 * npts * k
    return lib.igx_patch_eval_vspline_d(patch.handle, nc, d_dofs if d_c == 'dofs' else None, 1 if want_grad else 0, ptrs)


def test_lines_that_do_not_fit_the_lds_are_refused_and_the_value_is_served():
    kvs = se._kvs((1, 1, 1), (1, 1, 1000))
    geo = geometry.unit_cube()
    patch = assemblers.DevicePatch(kvs, geo)
    try:
        c = np.random.default_rng(5).uniform(-1.0, 1.0, size=(3,) + tuple(kv.numdofs for kv in kvs))
        d_c = _upload(patch, c)
        with pytest.raises(_lib.IgxError) as e:
            patch.eval_vspline(d_c, 3, want_grad=True)
        assert e.value.code == _lib.IGX_ERR_UNSUPPORTED
        only = patch.eval_vspline(d_c, 3, want_grad=False, to_host=True)
        for k in range(3):
            val, tol_val = se._reference(patch, kvs, geo, c[k])[:2]
            assert abs(only[k] - val).max() <= tol_val
    finally:
        patch.close()


def test_row_slab_span_box_and_bad_arguments_are_refused():
    kvs = se._kvs((2, 2, 2), (4, 2, 2))
    slab = assemblers.DevicePatch(kvs, geometry.unit_cube(), row0=(0, 3))
    try:
        assert _raw_call(slab, 2, False, whole=False) == _lib.IGX_ERR_UNSUPPORTED
    finally:
        slab.close()
    boxed = assemblers.DevicePatch(kvs, geometry.unit_cube(), bbox=((0, 2), (0, 1), (1, 2)))
    try:
        assert _raw_call(boxed, 3, True, whole=False) == _lib.IGX_ERR_UNSUPPORTED
    finally:
        boxed.close()
    patch = assemblers.DevicePatch(kvs, geometry.unit_cube())
    try:
        assert _raw_call(patch, 1, False) == _lib.IGX_ERR_ARG and _raw_call(patch, 4, False) == _lib.IGX_ERR_ARG
        assert _raw_call(patch, 2, False, d_c=None) == _lib.IGX_ERR_ARG
        assert _raw_call(patch, 2, False, n_out=1) == _lib.IGX_ERR_ARG              # a value array missing
        assert _raw_call(patch, 2, True, n_out=2 + 2 * 3 - 1) == _lib.IGX_ERR_ARG   # the last gradient array missing
        assert _raw_call(patch, 2, True, n_out=8) == _lib.IGX_OK
    finally:
        patch.close()


def test_jacobian_geometry_serves_the_values_only():
    kvs = se._kvs((2, 1), (3, 4))
    geo = geometry.quarter_annulus()
    spl = assemblers.DevicePatch(kvs, geo)
    grid = tuple(spl.gauss(k)[0] for k in range(2))
    spl.close()
    patch = assemblers.DevicePatch(kvs, geo, jacobian=geo.grid_jacobian(grid))
    try:
        c = np.random.default_rng(7).uniform(-1.0, 1.0, size=(2,) + tuple(kv.numdofs for kv in kvs))
        d_c = _upload(patch, c)
        only = patch.eval_vspline(d_c, 2, want_grad=False, to_host=True)
        for k in range(2):
            val, tol_val = se._reference(patch, kvs, geo, c[k])[:2]
            assert abs(only[k] - val).max() <= tol_val
        with pytest.raises(_lib.IgxError) as e:
            patch.eval_vspline(d_c, 2, want_grad=True)
        assert e.value.code == _lib.IGX_ERR_UNSUPPORTED
    finally:
        patch.close()

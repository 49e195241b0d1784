"""Spline functions as inputs of form strings on the device: the assembled matrices and functionals against the same forms with
the function given another way -- as a callable sampled on the host (identity map, where physical and parametric coordinates
coincide), or on other knot vectors (evaluated with grid_eval on the host and uploaded) -- and the updatable Assembler."""
import numpy as np
import pytest

from pyiga_amd import assemble, bspline, geometry

from conftest import rel_maxdiff

pytestmark = pytest.mark.gpu

RES_CUBIC = '(inner(grad(w),grad(v)) + w**3*v - f*v)*dx'
JAC_CUBIC = '(inner(grad(u),grad(v)) + 3*w**2*u*v)*dx'
RES_BURG = '(nu*inner(grad(w),grad(v)) + w*grad(w)[0]*v - f*v)*dx'
JAC_BURG = '(nu*inner(grad(u),grad(v)) + w*grad(u)[0]*v + grad(w)[0]*u*v)*dx'


def _random_spline(kvs, seed):
    rng = np.random.default_rng(seed)
    return bspline.BSplineFunc(kvs, rng.uniform(-1.0, 1.0, size=tuple(kv.numdofs for kv in kvs)))      # non-smooth on purpose


def _axes(xyz):
    """Grid axes (axis 0 first) from the coordinate arrays of the identity map: x varies along the LAST grid axis."""
    d = len(xyz)
    return tuple(np.asarray(xyz[d - 1 - k])[tuple(slice(None) if j == k else 0 for j in range(d))] for k in range(d))


@pytest.mark.parametrize('dim', [2, 3])
def test_identity_map_against_sampled_callables(dim):
    kvs = tuple(bspline.make_knots(p, 0.0, 1.0, n) for p, n in zip((3, 2, 2)[:dim], (5, 4, 3)[:dim]))
    geo = geometry.unit_square() if dim == 2 else geometry.unit_cube()
    w = _random_spline(kvs, 11)

    def wv(*xyz):
        return w.grid_eval(_axes(xyz))

    def wx(*xyz):
        return w.grid_jacobian(_axes(xyz))[..., 0]

    def gw(*xyz):
        J = w.grid_jacobian(_axes(xyz))
        return tuple(J[..., k] for k in range(dim))

    f = (lambda x, y: np.sin(x) * y) if dim == 2 else (lambda x, y, z: np.sin(x) * y + z)
    A = assemble.assemble(JAC_CUBIC, kvs, geo=geo, w=w)
    R = assemble.assemble('(inner(grad(u),grad(v)) + 3*wv**2*u*v)*dx', kvs, geo=geo, wv=wv)
    assert rel_maxdiff(A, R) <= 1e-12
    A = assemble.assemble(JAC_BURG, kvs, geo=geo, w=w, nu=0.1)
    R = assemble.assemble('(nu*inner(grad(u),grad(v)) + wv*inner((1.0,) + (0.0,) * %d, grad(u))*v + wx*u*v)*dx' % (dim - 1), kvs, geo=geo, wv=wv, wx=wx, nu=0.1)
    assert rel_maxdiff(A, R) <= 1e-12
    for res, ref, extra in ((RES_CUBIC, '(inner(gw,grad(v)) + wv**3*v - f*v)*dx', {}),
                            (RES_BURG, '(nu*inner(gw,grad(v)) + wv*wx*v - f*v)*dx', dict(nu=0.1))):
        b = assemble.assemble(res, kvs, geo=geo, w=w, f=f, **extra)
        r = assemble.assemble(ref, kvs, geo=geo, wv=wv, wx=wx, gw=gw, f=f, **extra)
        assert b.shape == r.shape and abs(b - r).max() <= 1e-12 * abs(r).max()


@pytest.mark.parametrize('dim', [2, 3])
def test_other_knot_vectors_agree_with_knot_insertion(dim):
    """A function on coarser knot vectors (host grid_eval, uploaded) and the same function after exact knot insertion onto the
    patch's space (dofs uploaded, evaluated by the spline kernel), on the quarter annulus: value and physical gradient."""
    n_c, n_f = (7, 14) if dim == 2 else (3, 6)
    coarse = tuple(bspline.make_knots(2, 0.0, 1.0, n_c) for _ in range(dim))
    kvs = tuple(bspline.make_knots(2, 0.0, 1.0, n_f) for _ in range(dim))
    geo = geometry.quarter_annulus() if dim == 2 else geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.quarter_annulus())
    wc = _random_spline(coarse, 3)
    c = wc.coeffs
    for k in range(dim):
        P = bspline.prolongation(coarse[k], kvs[k])
        c = np.moveaxis(np.tensordot(np.asarray(P.todense()), c, axes=(1, k)), 0, k)
    wf = bspline.BSplineFunc(kvs, c)
    for form, extra in ((JAC_CUBIC, {}), (JAC_BURG, dict(nu=0.1))):
        A = assemble.assemble(form, kvs, geo=geo, w=wf, **extra)
        B = assemble.assemble(form, kvs, geo=geo, w=wc, **extra)
        assert rel_maxdiff(A, B) <= 1e-12
    f = (lambda x, y: np.sin(x) * y) if dim == 2 else (lambda x, y, z: np.sin(x) * y + z)
    a = assemble.assemble(RES_BURG, kvs, geo=geo, w=wf, f=f, nu=0.1)
    b = assemble.assemble(RES_BURG, kvs, geo=geo, w=wc, f=f, nu=0.1)
    assert abs(a - b).max() <= 1e-12 * abs(b).max()


def test_updatable_spline_input_keeps_the_device_assembler():
    kvs = tuple(bspline.make_knots(3, 0.0, 1.0, 6) for _ in range(2))
    geo = geometry.quarter_annulus()
    w1, w2 = _random_spline(kvs, 1), _random_spline(kvs, 2)
    asm = assemble.Assembler(JAC_BURG, kvs, geo=geo, w=w1, nu=0.1, updatable=['w'])
    A1 = asm.assemble()
    dev, patch, handle = asm.asm, asm.asm.patch, asm.asm.patch.handle
    A2 = asm.assemble(w=w2)
    assert asm.asm is dev and asm.asm.patch is patch and patch.handle == handle
    assert asm.asm.coeff_cache_hit is True
    assert rel_maxdiff(A1, assemble.assemble(JAC_BURG, kvs, geo=geo, w=w1, nu=0.1)) == 0.0
    assert rel_maxdiff(A2, assemble.assemble(JAC_BURG, kvs, geo=geo, w=w2, nu=0.1)) == 0.0
    assert rel_maxdiff(A2, A1) > 1e-3
    with pytest.raises(RuntimeError):
        asm.update(nu=0.2)
    fun = assemble.Assembler(RES_BURG, kvs, geo=geo, w=w1, nu=0.1, f=lambda x, y: x * y, updatable=['w'])
    b1 = fun.assemble()
    b2 = fun.assemble(w=w2)
    assert np.array_equal(b2, assemble.assemble(RES_BURG, kvs, geo=geo, w=w2, nu=0.1, f=lambda x, y: x * y))
    assert abs(b2 - b1).max() > 1e-3

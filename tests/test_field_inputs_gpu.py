"""Coefficient expressions that read device arrays (igx_patch_eval_exprs_inputs_d) and the jet functional with its coefficients
and its result in device memory (igx_load_vector_jet_d)."""
import numpy as np
import pytest

from pyiga_amd import assemblers, bspline, geometry

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


@pytest.mark.parametrize('dim', [2, 3])
def test_expressions_with_inputs_and_resident_jet_functional(dim):
    kvs = tuple(bspline.make_knots(p, 0.0, 1.0, n) for p, n in zip((2, 3, 1)[:dim], (5, 3, 4)[:dim]))
    geo = geometry.quarter_annulus() if dim == 2 else geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.quarter_annulus())
    patch = assemblers.DevicePatch(kvs, geo)
    try:
        rng = np.random.default_rng(5)
        c = rng.uniform(-1.0, 1.0, size=tuple(kv.numdofs for kv in kvs))
        d_c = patch.upload_dofs(c)
        w = patch.eval_spline(d_c, want_grad=True, to_host=True)
        d_w = patch.eval_spline(d_c, want_grad=True)
        exprs = ['f0*f0*f0 + x*f1', 'sin(pi*y)*f2 - f0']
        out, _ = patch.eval_exprs_inputs(exprs, d_w, to_host=True)
        out2, hit = patch.eval_exprs_inputs(exprs, d_w, to_host=True)
        assert hit and np.array_equal(out, out2)
        grid = tuple(patch.gauss(k)[0] for k in range(dim))
        X = geo.grid_eval(grid)
        x, y = X[..., 0], X[..., 1]
        ref = [w[0] ** 3 + x * w[1], np.sin(np.pi * y) * w[2] - w[0]]
        for k in range(2):
            # a handful of roundings on operands of size <= max|ref| + 1 (sin and the coordinates of the device differ by ulps)
            assert abs(out[k] - ref[k]).max() <= 32 * EPS * (1.0 + abs(ref[k]).max())
        # another number of inputs is another kernel: f2 is not in scope with m = 2
        with pytest.raises(Exception):
            patch.eval_exprs_inputs(['f2'], d_w[:2])
        # the functional from the device arrays equals the one from the same arrays given on the host, bit for bit
        d_tab, _ = patch.eval_exprs_inputs(exprs, d_w)
        jet = [d_tab[0], d_tab[1]] + [None] * 2
        dev = patch.load_vector_jet_resident(jet, to_host=True)
        host = patch.load_vector_jet([out[0], out[1]] + [None] * (dim - 1))
        assert dev.shape == host.shape and np.array_equal(dev, host)
    finally:
        patch.close()

"""integrate() and error_norms() without a GPU: the host model against closed forms, the 1D integral, the argument errors and the
case table of the quadrature kernels against their launch logic."""
import os
import re

import numpy as np
import pytest

from pyiga_amd import approx, assemble, bspline, geometry

import _quad_cases as qc
import _quad_model as qm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grid(kvs):
    q = max(kv.p for kv in kvs) + 1
    return [qm.gauss_rule(kv, q)[0] for kv in kvs]


def _sample(f, geo, nodes):
    X = qm.geometry_ld(geo, nodes)[0].astype(np.float64)
    return f(*(X[..., k] for k in range(X.shape[-1])))


def test_model_annulus_area_and_second_moment():
    kvs = 2 * (bspline.make_knots(3, 0.0, 1.0, 10),)
    geo = geometry.quarter_annulus()
    nodes = _grid(kvs)
    f = [np.ones([len(n) for n in nodes]), _sample(lambda x, y: x * x + y * y, geo, nodes)]
    m = qm.quad_model(kvs, geo, f)
    assert abs(float(m['total'][0]) - 3 * np.pi / 4) < 1e-8            # (the reference's own check of integrate)
    assert abs(float(m['total'][1]) - 15 * np.pi / 8) < 1e-8           # int r^2 dA = (pi / 2) (r2^4 - r1^4) / 4
    assert m['elem'].shape == (2, 10, 10)
    assert abs(float(m['elem'].sum()) - float(m['total'].sum())) < 1e-14


def test_model_polynomial_on_the_cube_is_exact():
    kvs = qc.knots(bspline, (2, 1, 2), (3, 2, 4))                      # 3 points per span: exact to degree 5
    geo = geometry.unit_cube()
    nodes = _grid(kvs)
    f = _sample(lambda x, y, z: x ** 5 * y ** 2 * z ** 3 + 2.0 * y, geo, nodes)
    m = qm.quad_model(kvs, geo, [f])
    assert abs(float(m['total'][0]) - (1.0 / 6 / 3 / 4 + 1.0)) < 1e-14
    assert 0 < m['total_bound'][0] < 1e-9                                # (a rounding bound, not a discretisation error)


def test_model_error_sums_of_known_splines():
    kvs = qc.knots(bspline, (2, 2), (4, 3))
    # u_h = x (x belongs to the LAST axis): the Greville abscissae are its dofs
    c = np.broadcast_to(kvs[1].greville()[None, :], (kvs[0].numdofs, kvs[1].numdofs))
    m = qm.error_model(kvs, geometry.unit_square(), c, True)
    assert abs(float(m['total'][0]) - 1.0 / 3) < 1e-14 and abs(float(m['total'][1]) - 1.0) < 1e-14
    nodes = _grid(kvs)
    X = np.broadcast_to(nodes[1][None, :], (len(nodes[0]), len(nodes[1])))
    m = qm.error_model(kvs, geometry.unit_square(), c, True, exact=[X, np.ones_like(X), np.zeros_like(X)])
    assert abs(m['total']).max() < 1e-28 and m['total_bound'].max() < 1e-20
    # u_h = 1 on the annulus: the area, no gradient
    kvs = 2 * (bspline.make_knots(3, 0.0, 1.0, 10),)
    m = qm.error_model(kvs, geometry.quarter_annulus(), np.ones((13, 13)), True)
    assert abs(float(m['total'][0]) - 3 * np.pi / 4) < 1e-8 and abs(float(m['total'][1])) < 1e-25


def test_integrate_1d_on_the_host():
    kv = bspline.make_knots(2, 0.0, 1.0, 4)
    assert abs(assemble.integrate(kv, lambda x: x ** 2) - 1.0 / 3) < 1e-15
    v = assemble.integrate((kv,), lambda x: (x, 3.0 * x ** 2))
    assert v.shape == (2,) and np.allclose(v, [0.5, 1.0], rtol=0, atol=1e-15)


def test_argument_errors():
    kvs = 2 * (bspline.make_knots(2, 0.0, 1.0, 3),)
    with pytest.raises(AssertionError):
        assemble.integrate(kvs, lambda x, y: x, f_physical=True)
    with pytest.raises(ValueError):
        approx.error_norms(kvs, geometry.unit_square(), np.zeros(24))
    with pytest.raises(ValueError):
        approx.error_norms(kvs, geometry.unit_square(), np.zeros(25), grad_exact=lambda x, y: (x, y))


def test_case_table_reaches_the_launch_paths():
    d, s, dbl, _ = qc.CASES['3d_manylines']
    assert qc.nlines(qc.shape(d, s, dbl)[1]) == 33124 and qc.lpw(qc.shape(d, s, dbl)[1]) == 2
    for name in sorted(qc.CASES):
        d, s, dbl, _ = qc.CASES[name]
        if name != '3d_manylines':
            assert qc.lpw(qc.shape(d, s, dbl)[1]) == 1
        if name != '2d_long':
            assert qc.err12_waves(d, s, dbl, True) == qc.MAXWAVES and qc.wsum_waves(d, s, dbl, 4) == qc.MAXWAVES
    d, s, dbl, _ = qc.CASES['3d_straddle']
    assert qc.shape(d, s, dbl)[1][-1] == 69 and qc.straddling_elements(d, s) == [21]
    d, s, dbl, _ = qc.CASES['3d_straddle5']
    assert qc.shape(d, s, dbl)[1][-1] == 65 and qc.straddling_elements(d, s) == [12]
    d, s, dbl, _ = qc.CASES['2d_long']
    assert qc.err12_waves(d, s, dbl, True) == 1 and qc.err12_waves(d, s, dbl, False) == 2 and qc.wsum_waves(d, s, dbl, 4) == 1
    assert sorted(max(qc.CASES['3d_p%d' % p][0]) + 1 for p in range(1, 6)) == [2, 3, 4, 5, 6]
    for name, (d, s, dbl, _) in qc.CASES.items():                     # the dof counts of the table are those of the knot vectors
        assert tuple(kv.numdofs for kv in qc.knots(bspline, d, s, dbl)) == qc.shape(d, s, dbl)[2], name


def test_launch_logic_is_that_of_the_source():
    src = open(os.path.join(ROOT, 'pyiga_amd', 'csrc', 'kern_quad.hip')).read()
    assert re.search(r'Q_MAXWAVES = %d;' % qc.MAXWAVES, src)
    assert 'w * per_wave * sizeof(double) <= 64 * 1024' in src and qc.LDS_BYTES == 64 * 1024
    assert 'std::min<long long>(8, std::max<long long>(1, s.nlines / 16384))' in src
    assert '(size_t)(grad ? dim : 1) * Nlast + (size_t)(grad ? 2 : 1) * Glast' in src
    assert 'const size_t per_wave = (size_t)nf * al.G;' in src
    assert 'for (int g = lane; g < Gl; g += 64)' in src
    assert not re.search(r'atomic\w*\s*\(', src) and 'RTC_' not in src

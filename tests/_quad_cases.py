"""Case table of the quadrature kernels (pyiga_amd/csrc/kern_quad.hip): the smallest shapes at which each path changes, and the
launch logic of launch_error_sums / launch_quad_sums restated in Python (tests/test_quad_cpu.py ties the table to it)."""
import numpy as np

# name -> (degrees, spans, axes with a double interior knot, geometry)
CASES = {
    '3d_p1': ((1, 1, 1), (3, 2, 4), (), 'identity'),
    '3d_p2': ((2, 2, 2), (3, 2, 4), (), 'annulus'),
    '3d_p3': ((3, 3, 3), (3, 2, 4), (), 'twisted'),
    '3d_p4': ((4, 4, 4), (3, 2, 4), (), 'annulus'),
    '3d_p5': ((5, 5, 5), (3, 2, 4), (), 'twisted'),
    '3d_straddle': ((2, 2, 2), (2, 2, 23), (), 'annulus'),        # Gl = 69: element 21 covers g = 63..65, across the lane-pass boundary
    '3d_straddle5': ((4, 4, 4), (1, 1, 13), (), 'twisted'),       # Gl = 65: q = 5 does not divide 64
    '3d_mixed_double': ((2, 3, 1), (3, 5, 4), (1, 2), 'annulus'),  # fa is not span + const
    '3d_manylines': ((1, 1, 1), (91, 91, 1), (), 'identity'),     # 33124 lines: lpw = 2, a wave reuses its LDS
    '3d_onespan0': ((2, 2, 2), (1, 3, 2), (), 'twisted'),
    '3d_onespan1': ((2, 2, 2), (3, 1, 2), (), 'annulus'),
    '3d_onespan2': ((2, 2, 2), (3, 2, 1), (), 'identity'),
    '2d_p3': ((3, 3), (5, 5), (), 'annulus'),
    '2d_p14': ((1, 4), (5, 5), (), 'bspline_annulus'),
    '2d_double': ((3, 2), (4, 5), (0, 1), 'annulus'),
    '2d_long': ((1, 1), (3, 700), (), 'identity'),                # fewer waves per block from the LDS sizing
}
# value only, the geometry given as a Jacobian array
JACOBIAN_CASE = ((2, 1), (3, 4), (), 'annulus')

MAXWAVES, LDS_BYTES = 4, 64 * 1024


def knots(bspline, degrees, spans, double=()):
    """Open knot vectors on [0, 1]; on the axes of `double` one interior knot is repeated."""
    kvs = []
    for k, (p, n) in enumerate(zip(degrees, spans)):
        kv = bspline.make_knots(p, 0.0, 1.0, n)
        if k in double:
            kv = bspline.KnotVector(np.sort(np.append(kv.kv, kv.kv[kv.p + 2])), kv.p)
        kvs.append(kv)
    return tuple(kvs)


def geo(geometry, name, dim):
    if name == 'identity':
        return geometry.unit_square() if dim == 2 else geometry.unit_cube()
    if name == 'annulus':
        return geometry.quarter_annulus() if dim == 2 else geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.quarter_annulus())
    if name == 'bspline_annulus':
        return geometry.bspline_quarter_annulus()
    assert name == 'twisted' and dim == 3
    return geometry.twisted_box()


def shape(degrees, spans, double=()):
    """(q, G per axis, N per axis): Gauss points per span, Gauss points and dofs per axis"""
    q = max(degrees) + 1
    G = tuple(n * q for n in spans)
    N = tuple(n + p + (1 if k in double else 0) for k, (p, n) in enumerate(zip(degrees, spans)))
    return q, G, N


def nlines(G):
    return G[0] * G[1] if len(G) == 3 else G[0]


def lpw(G):
    """lines per wave: enough waves for the chip before a wave takes more than one line"""
    return int(min(8, max(1, nlines(G) // 16384)))


def waves(per_wave_doubles):
    """waves per block whose LDS lines fit (0: not even one does) -- quad_waves"""
    w = MAXWAVES
    while w >= 1:
        if w * per_wave_doubles * 8 <= LDS_BYTES:
            return w
        w >>= 1
    return 0


def err12_waves(degrees, spans, double, grad):
    q, G, N = shape(degrees, spans, double)
    dim = len(G)
    return waves((dim if grad else 1) * N[-1] + (2 if grad else 1) * G[-1])


def wsum_waves(degrees, spans, double, nf):
    q, G, N = shape(degrees, spans, double)
    return waves(nf * G[-1])


def straddling_elements(degrees, spans):
    """spans of the last axis whose q points lie in two passes of  for (g = lane; g < Gl; g += 64)"""
    q = max(degrees) + 1
    return [s for s in range(spans[-1]) if (s * q) // 64 != (s * q + q - 1) // 64]

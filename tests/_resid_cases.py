"""Case table of the residual kernel (pyiga_amd/csrc/kern_quad.hip: k_res12): the shapes of tests/_quad_cases.py -- the walk is
that of k_err12, so the shapes at which it can go wrong are the same: every q = 2..6, an element that straddles two passes of the
point loop, double knots, more lines than waves, one-span axes, a long last axis -- plus the wave counts the larger line buffers
give, and one last axis that a single wave cannot hold.  The launch logic of launch_residual_sums restated in Python
(tests/test_resid_cpu.py ties the table to it)."""
import _quad_cases as qc

# name -> (degrees, spans, axes with a double interior knot, geometry)
CASES = dict(qc.CASES)
CASES.update({
    '3d_manylines_p2': ((2, 2, 2), (74, 74, 1), (), 'annulus'),  # 49284 lines: lpw = 3, a wave reuses its six lines with a Hessian in them
    '2d_two_waves': ((2, 2), (3, 250), (), 'annulus'),        # 3 * 252 + 2 * 750 = 2256 doubles per wave: two waves per block
    '2d_one_wave': ((2, 2), (2, 500), (), 'annulus'),         # 3 * 502 + 2 * 1500 = 4506: one
})
# 3 * 1002 + 2 * 3000 = 9006 doubles > 8192: not even one wave (k_err12 would still run: 2 * 1002 + 2 * 3000 = 8004)
TOO_LONG = ((2, 2), (1, 1000), (), 'annulus')
# the geometry given as a Jacobian array: refused
JACOBIAN_CASE = qc.JACOBIAN_CASE

MAXWAVES, LDS_BYTES = qc.MAXWAVES, qc.LDS_BYTES
knots, geo, shape, nlines, lpw, waves, straddling_elements = qc.knots, qc.geo, qc.shape, qc.nlines, qc.lpw, qc.waves, qc.straddling_elements


def res12_lines(dim):
    """LDS lines of N_last doubles per wave: the (axis-0 order, mid order) combinations of total order <= 2"""
    return 6 if dim == 3 else 3


def res12_per_wave(degrees, spans, double):
    q, G, N = shape(degrees, spans, double)
    return res12_lines(len(G)) * N[-1] + 2 * G[-1]


def res12_waves(degrees, spans, double):
    return waves(res12_per_wave(degrees, spans, double))

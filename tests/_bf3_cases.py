"""The instantiations of k_bf3 (pyiga_amd/csrc/fused3.hip) and one small patch per instantiation.

Plain helper module (not a conftest): ``tests/test_bf3_coverage_cpu.py`` checks that the table below and the dispatch table of
``launch_bf3`` / ``launch_bf3_c`` cannot drift apart, ``tests/test_gpu_parity.py`` assembles every case on the device.

A k_bf3 instantiation is picked by
  * (P1, P2, Q): P1 = degree + 1 of the swept (mid) axis, P2 = degree + 1 of the last axis, Q = Gauss points per span =
    max degree + 1 over all three axes (the default nqp, pyiga/assemblers.pyx:1338);
  * the form: mass -> slot mask MASS, SYM 3 (per-axis symmetry); stiffness -> STIFF3, SYM 2; convection-diffusion (and the
    non-symmetric form tables) -> STIFF3, SYM 0;
  * MULT: repeated interior knots on the swept axis;
  * TR: repeated knots on the last axis only -- the patch is assembled through its twin, whose mid and last axis are exchanged,
    so the key is that of the exchanged axes.
"""
import collections
import os
import re

import numpy as np

FUSED3_HIP = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'pyiga_amd', 'csrc', 'fused3.hip')

# the form -> (slot mask, SYM) of launch_bf3 (fused3.hip: BF_MASK_*, symk)
FORM_KEY = {'mass': ('MASS', 3), 'stiffness': ('STIFF3', 2), 'convdiff': ('STIFF3', 0), 'form_nonsym': ('STIFF3', 0)}

Key = collections.namedtuple('Key', 'P1 P2 Q mask sym mult tr')


def axis_knots(spec):
    """Knot vector of an axis spec (p, n, rep): n spans of degree p over [0, 1]; rep = 1 single knots, an int m every interior
    knot m times (bspline.make_knots(p, 0, 1, n, mult=m), the same expression), or a tuple of multiplicities, one per
    interior knot (then n = len(rep) + 1)."""
    p, n, rep = spec
    if isinstance(rep, tuple):
        assert len(rep) == n - 1, spec
        inner = np.repeat(np.arange(1, n) / n, rep)
    else:
        inner = np.repeat(np.arange(0., 1., 1. / n)[1:], rep)
    return np.concatenate([np.zeros(p + 1), inner, np.ones(p + 1)])


def _knots_p(kv):
    """(knots, degree) of a KnotVector (``.kv``, ``.p``), a (knots, p) pair or an axis spec (p, n, rep)."""
    if hasattr(kv, 'kv'):
        return np.asarray(kv.kv, dtype=float), int(kv.p)
    if len(kv) == 3 and not hasattr(kv[0], '__len__'):
        return axis_knots(kv), int(kv[0])
    return np.asarray(kv[0], dtype=float), int(kv[1])


def repeated(kv):
    """True if the axis has a repeated interior knot (igx_api.hip: Axis::simple is false)."""
    k, p = _knots_p(kv)
    _, counts = np.unique(k[p + 1:len(k) - p - 1], return_counts=True)
    return bool((counts > 1).any())


def numdofs(kv):
    k, p = _knots_p(kv)
    return len(k) - p - 1


def fused3_degrees(P1, P2, Q, sym3d, mid_simple):
    """fused3.hip: fused3_degrees, restated."""
    if not mid_simple and not (P1 == P2 == Q):
        return False
    if P1 < 2 or P2 < 2 or Q > 6:
        return False
    if P1 == P2 == Q:
        return True
    if not sym3d or Q < 3:
        return False
    gap = 2 if Q <= 5 else 1
    return P1 >= Q - gap and P2 >= Q - gap


def bf3_key(kvs, kind):
    """The k_bf3 instantiation launch_bf3 runs for a 3D spline patch with the default nqp, or None where the stage kernels
    serve the patch instead (unequal degrees with repeated knots on the swept axis, Q > 6, degrees fused3_degrees refuses,
    repeated knots on both the mid and the last axis, degrees k_geoA does not take on axis 0)."""
    mask, sym = FORM_KEY[kind]
    kp = [_knots_p(kv) for kv in kvs]
    p = [d for _, d in kp]
    rep = [repeated(kv) for kv in kvs]
    Q = max(p) + 1
    mid, last, tr = 1, 2, False
    if rep[2]:
        if rep[1]:
            return None
        mid, last, tr = 2, 1, True                  # the twin: mid and last axis exchanged
    P1, P2, mult = p[mid] + 1, p[last] + 1, rep[mid]
    if not fused3_degrees(P1, P2, Q, sym >= 2, not mult):
        return None
    # k_geoA (geoa.hip: geoA_supported): degree 1 .. 5 on axis 0, 2 .. 5 for the convection-diffusion form
    if not 1 <= p[0] <= 5 or (sym == 0 and p[0] < 2):
        return None
    return Key(P1, P2, Q, mask, sym, mult, tr)


# ---- the dispatch table of fused3.hip, read from the source
def read_source(path=FUSED3_HIP):
    with open(path) as f:
        return f.read()


def parse_bf3_cases(src):
    """(P1, P2, Q) of every BF3_CASE(a, b, c) line of launch_bf3 (the #define itself excluded)."""
    body = src[src.index('int launch_bf3('):]
    body = body[body.index('#define BF3_CASE'):]
    body = body[body.index('\n'):body.index('#undef BF3_CASE')]
    return {tuple(int(v) for v in m) for m in re.findall(r'BF3_CASE\(\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*\)', body)}


def _launch_bf3_c(src):
    body = src[src.index('static int launch_bf3_c('):]
    return body[:body.index('\ntemplate')]


def parse_tr_syms(src):
    """SYM values the TR branch of launch_bf3_c launches (every one with MULT: the twin's swept axis has repeated knots)."""
    body = _launch_bf3_c(src)
    tr = body[body.index('if (tr) {'):body.index('constexpr int PM')]
    assert 'symk == 1' not in tr
    return {int(s) for s in re.findall(r'if \(symk == (\d) && mult\)', tr)}


def parse_mult_syms(src):
    """SYM values the non-TR part of launch_bf3_c launches with MULT = true for a patch with repeated knots on the swept axis
    (the equal-degree branches)."""
    body = _launch_bf3_c(src)
    rest = body[body.index('constexpr int PM'):]
    syms = set(int(s) for s in re.findall(r'if \(symk == (\d) && mult\)', rest))
    if re.search(r'if \(symk == 2\) return mult \?', rest):
        syms.add(2)
    if re.search(r'if \(symk == 0\) \{[^}]*mult \?', rest, re.S):
        syms.add(0)
    return syms


SYM_FORM = {3: 'mass', 2: 'stiffness', 0: 'convdiff'}


def reachable_keys(cases=None):
    """Every k_bf3 key a 3D mass, stiffness or convection-diffusion patch can reach, derived from the BF3_CASE list of
    fused3.hip and the MULT / TR branches of launch_bf3_c."""
    src = read_source()
    triples = parse_bf3_cases(src)
    tr_syms, mult_syms = parse_tr_syms(src), parse_mult_syms(src)
    keys = set()
    for P1, P2, Q in triples:
        eq = P1 == P2 == Q
        for kind in ('mass', 'stiffness', 'convdiff'):
            mask, sym = FORM_KEY[kind]
            if not fused3_degrees(P1, P2, Q, sym >= 2, True):
                continue
            if sym == 0 and Q < 3:
                continue                            # (axis 0 of degree >= 2 makes Q > P1: not equal degrees any more)
            keys.add(Key(P1, P2, Q, mask, sym, False, False))
            if eq and P1 >= 3:                      # (degree 1: no knot can be repeated)
                if sym in mult_syms:
                    keys.add(Key(P1, P2, Q, mask, sym, True, False))
                if sym in tr_syms:
                    keys.add(Key(P1, P2, Q, mask, sym, True, True))
    return keys


# ---- the cases: (axis specs (p, n, rep) of axes 0, 1, 2, geometry, forms).  Q = max degree + 1; the comment names (P1, P2, Q).
# Mixed across the list: an axis shorter than 2p + 1 dofs (every row an edge row), unequal dofs per axis, axis 0 of lower
# degree than the other two, NURBS (cylinder) and B-spline (twisted_box) maps, multiplicities 2 .. p with a C^0 knot.
MS = ('mass', 'stiffness')
MSC = ('mass', 'stiffness', 'convdiff')
_CASES = [
    # equal degrees, single knots
    (((1, 3, 1), (1, 6, 1), (1, 5, 1)), 'twisted_box', MS),                      # (2, 2, 2)
    (((1, 4, 1), (2, 2, 1), (2, 7, 1)), 'cylinder', MS),                         # (3, 3, 3): mid axis 4 dofs < 2p + 1
    (((2, 3, 1), (2, 5, 1), (2, 4, 1)), 'twisted_box', ('convdiff',)),           # (3, 3, 3)
    (((2, 2, 1), (3, 4, 1), (3, 6, 1)), 'cylinder', MS),                         # (4, 4, 4)
    (((3, 2, 1), (3, 3, 1), (3, 5, 1)), 'cylinder', ('convdiff',)),              # (4, 4, 4)
    (((4, 1, 1), (4, 2, 1), (4, 7, 1)), 'twisted_box', MS),                      # (5, 5, 5)
    (((2, 3, 1), (4, 5, 1), (4, 2, 1)), 'cylinder', ('convdiff',)),              # (5, 5, 5): last axis 6 dofs < 2p + 1
    (((3, 2, 1), (5, 3, 1), (5, 2, 1)), 'cylinder', MS),                         # (6, 6, 6)
    (((5, 1, 1), (5, 2, 1), (5, 4, 1)), 'twisted_box', ('convdiff',)),           # (6, 6, 6)
    # Q = 3
    (((1, 5, 1), (1, 4, 1), (2, 6, 1)), 'cylinder', MS),                         # (2, 3, 3)
    (((2, 2, 1), (2, 6, 1), (1, 3, 1)), 'twisted_box', MS),                      # (3, 2, 3)
    (((2, 3, 1), (1, 5, 1), (1, 7, 1)), 'cylinder', MS),                         # (2, 2, 3)
    # Q = 4
    (((3, 2, 1), (2, 5, 1), (3, 3, 1)), 'twisted_box', MS),                      # (3, 4, 4)
    (((1, 4, 1), (3, 2, 1), (2, 8, 1)), 'cylinder', MS),                         # (4, 3, 4)
    (((3, 1, 1), (2, 3, 1), (2, 6, 1)), 'cylinder', MS),                         # (3, 3, 4)
    (((2, 2, 1), (1, 6, 1), (3, 4, 1)), 'twisted_box', MS),                      # (2, 4, 4)
    (((3, 2, 1), (3, 4, 1), (1, 5, 1)), 'cylinder', MS),                         # (4, 2, 4)
    (((3, 3, 1), (1, 3, 1), (2, 5, 1)), 'twisted_box', MS),                      # (2, 3, 4)
    (((3, 1, 1), (2, 4, 1), (1, 9, 1)), 'cylinder', MS),                         # (3, 2, 4)
    (((3, 2, 1), (1, 4, 1), (1, 6, 1)), 'cylinder', MS),                         # (2, 2, 4)
    # Q = 5
    (((2, 2, 1), (3, 3, 1), (4, 5, 1)), 'cylinder', MS),                         # (4, 5, 5)
    (((4, 1, 1), (4, 4, 1), (3, 3, 1)), 'twisted_box', MS),                      # (5, 4, 5)
    (((4, 2, 1), (3, 2, 1), (3, 7, 1)), 'cylinder', MS),                         # (4, 4, 5)
    (((1, 3, 1), (2, 4, 1), (4, 3, 1)), 'twisted_box', MS),                      # (3, 5, 5)
    (((3, 2, 1), (4, 2, 1), (2, 6, 1)), 'cylinder', MS),                         # (5, 3, 5)
    (((4, 1, 1), (2, 5, 1), (3, 4, 1)), 'cylinder', MS),                         # (3, 4, 5)
    (((4, 2, 1), (3, 3, 1), (2, 5, 1)), 'twisted_box', MS),                      # (4, 3, 5)
    (((4, 1, 1), (2, 3, 1), (2, 8, 1)), 'cylinder', MS),                         # (3, 3, 5)
    # Q = 6 (a degree gap of one)
    (((2, 2, 1), (4, 2, 1), (5, 3, 1)), 'cylinder', MS),                         # (5, 6, 6)
    (((5, 1, 1), (5, 3, 1), (4, 2, 1)), 'twisted_box', MS),                      # (6, 5, 6)
    (((5, 1, 1), (4, 3, 1), (4, 4, 1)), 'cylinder', MS),                         # (5, 5, 6)
    # MULT: repeated knots on the swept axis, equal degrees
    (((2, 3, 1), (2, 5, 2), (2, 4, 1)), 'cylinder', MSC),                        # (3, 3, 3): C^0 knots
    (((1, 2, 1), (3, 4, (2, 3, 1)), (3, 5, 1)), 'twisted_box', MS),              # (4, 4, 4): double and C^0
    (((2, 2, 1), (3, 3, 2), (3, 2, 1)), 'cylinder', ('convdiff',)),              # (4, 4, 4)
    (((4, 1, 1), (4, 3, (4, 2)), (4, 3, 1)), 'cylinder', MSC),                   # (5, 5, 5): C^0 and double
    (((3, 1, 1), (5, 3, (3, 5)), (5, 2, 1)), 'cylinder', MS),                    # (6, 6, 6)
    (((2, 1, 1), (5, 2, 2), (5, 3, 1)), 'twisted_box', ('convdiff',)),           # (6, 6, 6)
    # TR: repeated knots on the last axis only (the twin)
    (((2, 2, 1), (2, 4, 1), (2, 4, 2)), 'twisted_box', MSC),                     # (3, 3, 3): C^0 knots
    (((3, 1, 1), (3, 4, 1), (3, 4, (3, 1, 2))), 'cylinder', MSC),                # (4, 4, 4): C^0, single and double
    (((2, 2, 1), (4, 2, 1), (4, 3, (2, 3))), 'cylinder', MSC),                   # (5, 5, 5)
    (((4, 1, 1), (5, 2, 1), (5, 2, 5)), 'twisted_box', MS),                      # (6, 6, 6): C^0 knot
    (((2, 1, 1), (5, 2, 1), (5, 3, (2, 4))), 'cylinder', ('convdiff',)),         # (6, 6, 6)
]

Case = collections.namedtuple('Case', 'id axes geo kind key slabs')


def _expand():
    out, seen = [], set()
    for axes, geo, kinds in _CASES:
        for kind in kinds:
            key = bf3_key(axes, kind)
            tag = '%s-%s-%s' % (kind, '-'.join('p%dn%d%s' % (p, n, '' if rep == 1 else 'm' + ''.join(map(str, np.atleast_1d(rep))))
                                                for p, n, rep in axes), geo)
            trip = None if key is None else (key.P1, key.P2, key.Q, key.mult, key.tr)
            out.append(Case(tag, axes, geo, kind, key, trip not in seen))       # row slabs: the first case of each (P1, P2, Q)
            seen.add(trip)
    return out


BF3_CASES = _expand()


# ---- the tile height of k_bf3 along the last axis: BF3Geom<...>::rmax() (fused3.hip) with the launch shape of launch_bf3_c
def bf3_rmax(P1, P2, Q, kind):
    PM = max(P1, P2, Q)
    mask, sym = FORM_KEY[kind]
    if mask == 'MASS':
        nlg, nro = (3 if PM == 5 else 2), 1                     # BF3Cfg<PM, BF_MASK_MASS>
    else:
        nlg, nro = (3 if PM == 5 or (PM == 6 and sym == 0) else 2), 4     # BF3CfgS3<PM, SYMK>
    nset = 2 if sym == 2 else 1
    p1, p2 = P1 - 1, P2 - 1
    W1, W2, TL = 2 * P1 - 1, 2 * P2 - 1, 64 * nlg
    QS = Q + (1 if Q % 2 == 0 else 0)
    NSP = (TL + Q - 1) // Q
    TLP = TL + NSP * (QS - Q)
    VS = Q * P2 * 2 + (0 if (Q * P2 * 2) % 4 == 2 else 2)
    LS = nro * TLP + 2
    NRL = p1 * (p1 + 1) // 2 + p1 + P1
    off_sets = (W1 * LS + 1) & ~1

    def lds(R):
        return ((off_sets + nset * (NRL * R * W2 + 2) + 1) & ~1) + NSP * VS + 2 * (2 * p2 * W2)
    R = TL // Q - p2
    while R > 1 and lds(R) * 8 > 160 * 1024:
        R -= 1
    return R


# tile-edge sweep: (axis specs of axes 0 and 1, degree of the last axis, geometry, form); the last axis runs over a contiguous
# range of dof counts N2 = 2 p + 1 .. 2 RMAX + 2 (one, two and three tiles)
EDGE_SWEEPS = [
    (((1, 1, 1), (2, 1, 1)), 2, 'cylinder', 'stiffness'),      # (3, 3, 3)
    (((3, 1, 1), (3, 1, 1)), 2, 'twisted_box', 'mass'),        # (4, 3, 4): unequal degrees
    (((2, 1, 1), (4, 1, 1)), 4, 'cylinder', 'mass'),           # (5, 5, 5)
    (((4, 1, 1), (3, 1, 1)), 4, 'cylinder', 'stiffness'),      # (4, 5, 5): unequal degrees
    (((2, 1, 1), (5, 1, 1)), 5, 'twisted_box', 'convdiff'),    # (6, 6, 6)
]


def edge_sweep_sizes(axes01, p2, kind):
    """Spans of the last axis for the sweep: N2 = n + p2 from 2 p2 + 1 to 2 RMAX + 2."""
    p = [axes01[0][0], axes01[1][0], p2]
    rmax = bf3_rmax(p[1] + 1, p2 + 1, max(p) + 1, kind)
    return list(range(p2 + 1, 2 * rmax + 3 - p2)), rmax

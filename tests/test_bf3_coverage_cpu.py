"""The instantiations of k_bf3 and the cases that run them cannot drift apart (no GPU needed).

The dispatch table of launch_bf3 (the BF3_CASE lines of pyiga_amd/csrc/fused3.hip) and the degrees fused3_degrees admits must
describe the same set of (P1, P2, Q); every key a patch can reach must be the key of a case in tests/_bf3_cases.BF3_CASES, which
tests/test_gpu_parity.py::test_every_bf3_instantiation_vs_oracle assembles on the device.  A new BF3_CASE line, a wider
fused3_degrees or a new MULT / TR branch without a case fails here."""
import ctypes
import os

import pytest

import _bf3_cases as bc
from conftest import ROOT


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(ROOT, 'pyiga_amd', 'libigx.so')):
        ge.build()
    import pyiga_amd
    return pyiga_amd._lib


def _admitted():
    """(P1, P2, Q) fused3_degrees admits for the symmetric 3D forms with single knots on the swept axis, with Q = max degree + 1
    (the default nqp: no axis has more than Q basis functions per span)."""
    return {(P1, P2, Q) for Q in range(1, 9) for P1 in range(1, Q + 1) for P2 in range(1, Q + 1)
            if bc.fused3_degrees(P1, P2, Q, True, True)}


def test_dispatch_table_equals_the_admitted_degrees():
    """No BF3_CASE line that no patch can reach, no admitted (P1, P2, Q) without a BF3_CASE line: Q <= 6, P >= 2, equal
    degrees, or a degree gap of up to 2 below Q (up to Q = 5) and of 1 at Q = 6."""
    cases = bc.parse_bf3_cases(bc.read_source())
    admitted = _admitted()
    assert cases == admitted, ('dead BF3_CASE lines', sorted(cases - admitted), 'admitted without a case', sorted(admitted - cases))
    assert len(cases) == 27
    assert {(P, P, P) for P in range(2, 7)} <= cases


def test_fused3_degrees_restatement_equals_the_library(lib):
    """The Python restatement of fused3_degrees is the compiled function (igx::fused3_degrees), over every argument up to
    degree 7: widening the library without widening the cases fails here."""
    fn = getattr(lib.load(), '_ZN3igx14fused3_degreesEiiibb')
    fn.restype = ctypes.c_bool
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_bool, ctypes.c_bool]
    for P1 in range(1, 9):
        for P2 in range(1, 9):
            for Q in range(1, 9):
                for sym3d in (False, True):
                    for simple in (False, True):
                        assert bool(fn(P1, P2, Q, sym3d, simple)) == bc.fused3_degrees(P1, P2, Q, sym3d, simple), (P1, P2, Q, sym3d, simple)


def test_mult_and_tr_branches():
    """launch_bf3_c: repeated knots on the swept axis (MULT) and the twin (TR) launch kernels for the mass form (SYM 3), the
    stiffness form (SYM 2) and the non-symmetric form (SYM 0), at equal degrees only."""
    src = bc.read_source()
    assert bc.parse_mult_syms(src) == {3, 2, 0}
    assert bc.parse_tr_syms(src) == {3, 2, 0}


def test_every_reachable_key_has_a_case():
    keys = bc.reachable_keys()
    covered = {c.key for c in bc.BF3_CASES}
    assert None not in covered, [c.id for c in bc.BF3_CASES if c.key is None]
    assert keys - covered == set(), sorted(keys - covered)
    assert covered - keys == set(), sorted(covered - keys)
    # 27 (P1, P2, Q) x {mass, stiffness}, equal degrees 3 .. 6 x {convection-diffusion}, and MULT and TR at equal degrees
    # 3 .. 6 x {mass, stiffness, convection-diffusion}
    assert len(keys) == 27 * 2 + 4 + 12 + 12
    for kind in ('mass', 'stiffness', 'convdiff'):
        mask, sym = bc.FORM_KEY[kind]
        for P in range(3, 7):
            for mult, tr in ((True, False), (True, True)):
                assert bc.Key(P, P, P, mask, sym, mult, tr) in covered, (kind, P, mult, tr)


def test_the_cases_hit_the_edges():
    """The features the cases are shaped for occur in the table: short axes (every row an edge row), unequal dofs per axis,
    axis 0 of lower degree, both geometry kinds, multiplicities 2 .. p with a C^0 knot on the swept and on the last axis."""
    short = unequal = low0 = c0_mid = c0_last = 0
    geos = set()
    for c in bc.BF3_CASES:
        p = [a[0] for a in c.axes]
        N = [bc.numdofs(a) for a in c.axes]
        short += any(n < 2 * q + 1 for n, q in zip(N[1:], p[1:]))
        unequal += len(set(N)) == 3
        low0 += p[0] < min(p[1:])
        geos.add(c.geo)
        for ax, hit in ((1, 'mid'), (2, 'last')):
            q, n, rep = c.axes[ax]
            if max(rep if isinstance(rep, tuple) else (rep,)) == q and q >= 2:
                if hit == 'mid':
                    c0_mid += 1
                else:
                    c0_last += 1
    assert short and unequal and low0 and c0_mid and c0_last, (short, unequal, low0, c0_mid, c0_last)
    assert geos == {'cylinder', 'twisted_box'}


def test_bf3_key_rules():
    """bf3_key on hand-picked patches: the exchanged axes of the twin, the stage kernels where k_bf3 does not apply."""
    K = bc.Key
    assert bc.bf3_key(((2, 3, 1), (3, 4, 1), (1, 5, 1)), 'stiffness') == K(4, 2, 4, 'STIFF3', 2, False, False)
    assert bc.bf3_key(((2, 3, 1), (3, 4, 1), (3, 5, 2)), 'mass') == K(4, 4, 4, 'MASS', 3, True, True)
    assert bc.bf3_key(((2, 3, 1), (3, 4, 2), (3, 5, 2)), 'mass') is None                  # repeated knots on mid and last axis
    assert bc.bf3_key(((2, 3, 1), (3, 4, 2), (2, 5, 1)), 'stiffness') is None             # unequal degrees with MULT
    assert bc.bf3_key(((6, 3, 1), (6, 4, 1), (6, 5, 1)), 'stiffness') is None             # Q = 7
    assert bc.bf3_key(((1, 3, 1), (1, 4, 1), (4, 5, 1)), 'mass') is None                  # a gap of three degrees
    assert bc.bf3_key(((5, 3, 1), (4, 4, 1), (5, 5, 1)), 'mass') == K(5, 6, 6, 'MASS', 3, False, False)
    assert bc.bf3_key(((5, 3, 1), (3, 4, 1), (5, 5, 1)), 'mass') is None                  # a gap of two at Q = 6
    assert bc.bf3_key(((2, 3, 1), (1, 4, 1), (2, 5, 1)), 'convdiff') is None              # non-symmetric: equal degrees only
    assert bc.bf3_key(((1, 3, 1), (2, 4, 1), (2, 5, 1)), 'convdiff') is None              # ... and degree >= 2 on axis 0
    assert bc.bf3_key(((2, 3, 1), (2, 4, 1), (2, 5, 1)), 'form_nonsym') == K(3, 3, 3, 'STIFF3', 0, False, False)

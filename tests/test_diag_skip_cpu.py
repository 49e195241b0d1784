"""The K1 slices that diagonal outer pairs duplicate (sumfact.hip: plan_diag_skip; DESIGN.md sections 3.1, 3.2).

The 3D stiffness chain k_geoA -> k_bf3 keeps eight K1 arrays, one per distinct (axis-0 type, field).  Two couples of them differ
only by which of the two axis-0 basis functions carries the derivative; on an outer pair i0 = j0 the two arrays of a couple are
the same sum, formed from the same products in the same order, so k_geoA writes one of them and k_bf3 reads that one twice.
This file restates the condition the plan tests -- from the terms of the form, not from its name -- and checks the claim about
the bits with the oracle's 1D tables.  No GPU.
"""
import itertools
import struct

import numpy as np
import pytest


# ---- the stiffness form as sumfact_stages.h (form_terms) states it: du^T B dv, one term per (a, b) = (grid axis that carries the
# derivative of the trial function u, ... of the test function v); type of axis k = tu + 2 tv = (k == a) + 2 (k == b); the field is
# the entry of the symmetric matrix B the two gradient components pick: an unordered pair of axes
def stiffness_terms():
    return [dict(t=tuple((k == a) + 2 * (k == b) for k in range(3)), f=frozenset((a, b))) for a in range(3) for b in range(3)]


def slot_table():
    """(mid-axis type t1, last-axis type y) -> (axis-0 type, field): the input of k_bf3's slot; one K1 array per distinct value."""
    slots = {}
    for term in stiffness_terms():
        t0, t1, y = term['t']
        assert (t1, y) not in slots                       # one array per slot: what the fused stage of the symmetric form takes
        slots[(t1, y)] = (t0, term['f'])
    return slots


def couples(slots):
    """Pairs of slots whose arrays have the same field and the axis-0 types 1 (N_i0 N'_j0) and 2 (N'_i0 N_j0): (member of type 2,
    member of type 1).  The plan's test (plan_diag_skip): derived from the slot / source tables."""
    out = []
    for (sa, (ta, fa)), (sb, (tb, fb)) in itertools.permutations(slots.items(), 2):
        if fa == fb and ta == 2 and tb == 1:
            out.append((sa, sb))
    return sorted(out)


def test_slot_table_has_exactly_the_two_couples():
    slots = slot_table()
    assert len(slots) == 9 and len(set(slots.values())) == 8          # nine slots, eight arrays: (2, 1) and (1, 2) share one
    assert slots[(2, 1)] == slots[(1, 2)] and slots[(2, 1)][0] == 0
    # slot (1, 0) with (2, 0) over F01, slot (0, 1) with (0, 2) over F02 -- nothing else
    assert couples(slots) == [((0, 1), (0, 2)), ((1, 0), (2, 0))]
    for kept, skipped in couples(slots):
        assert slots[kept][1] == slots[skipped][1] and (slots[kept][0], slots[skipped][0]) == (2, 1)
    # the members of axis-0 type 1 are the ones a diagonal pair does not store: two of the eight arrays
    assert sorted(s for _, s in couples(slots)) == [(0, 2), (2, 0)]


def test_role_of_last_axis_type_2_is_the_transposed_role_of_type_1():
    """With the couples equal on a diagonal pair, the arrays entering the sweep with last-axis type 2 are those of type 1 with the
    mid-axis type transposed (tu <-> tv), and no other pair of roles is related that way."""
    slots = slot_table()
    src = dict(slots)
    for kept, skipped in couples(slots):
        src[skipped] = slots[kept]                        # what a diagonal block reads

    def tr(t1):
        return (t1 >> 1) | ((t1 & 1) << 1)
    role = {y: {t1: src[(t1, yy)] for (t1, yy) in src if yy == y} for y in range(4)}
    assert role[2] == {tr(t1): a for t1, a in role[1].items()} and len(role[1]) == 2
    # (without the couples the two roles read different arrays)
    plain = {y: {t1: slots[(t1, yy)] for (t1, yy) in slots if yy == y} for y in range(4)}
    assert plain[2] != {tr(t1): a for t1, a in plain[1].items()}


def bits(x):
    return struct.unpack('<q', struct.pack('<d', float(x)))[0]


@pytest.mark.parametrize('p', [1, 2, 3, 4])
def test_axis0_sums_of_a_couple(oracle, p):
    """k_geoA's pair-product sweep adds, plane by plane, (V_a[tv] V_b[tu]) f to the sum of the pair (a: test function i0, b: trial
    function j0; type = tu + 2 tv).  For the types 1 and 2 over the same field the product of a plane is V_a[0] V_b[1] against
    V_a[1] V_b[0]: with a = b the same two factors, and IEEE multiplication commutes -- the same float64 bits after every plane.
    Off the diagonal the sums are different numbers.  (Degree 5 takes the vector sweep, which multiplies in another order: the plan
    keeps the flag off there, geoA_diag_types_commute.)"""
    n = p + 3
    kv = oracle.make_knots(p, 0.0, 1.0, n)
    mesh = np.unique(kv.kv)
    (nodes,), (w,) = oracle.make_tensor_quadrature((mesh,), p + 1)
    V = oracle.compute_values_derivs(kv, nodes, 1)        # (dof, Gauss point, derivative)
    rng = np.random.default_rng(1234 + p)
    f = w * (0.5 + rng.random(len(nodes)))                # a field that is no function of the pair: one value per plane
    N = kv.numdofs
    ndiag = noff = 0
    for i0 in range(N):
        for j0 in range(max(0, i0 - p), i0 + 1):
            s = {1: 0.0, 2: 0.0}
            for g in range(len(nodes)):
                if V[i0, g, 0] == 0.0 and V[i0, g, 1] == 0.0:
                    continue
                for t in (1, 2):
                    tu, tv = t & 1, t >> 1
                    s[t] = s[t] + (V[i0, g, tv] * V[j0, g, tu]) * f[g]
            if i0 == j0:
                assert bits(s[1]) == bits(s[2]), (p, i0)
                ndiag += 1
            else:
                assert bits(s[1]) != bits(s[2]), (p, i0, j0)
                noff += 1
    assert ndiag == N and noff > 0

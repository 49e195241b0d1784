"""Host models of the load-vector kernels (no GPU, no library load).

- ``window_events``: the sliding window of k_lv12 along the mid axis (pyiga_amd/csrc/kern_vector.hip), chunk by chunk: the span
  loop, the dofs that leave at the end of a span (``nleave``), whether a leaving dof holds its whole support (``whole``: stored)
  or a part of it (added onto zeros).  An event is (chunk, dof, 'store' | 'add', ((g1, a), ..)): the Gauss points of the mid axis
  and the local basis index whose products the register held when it was written.
- ``check_window``: every dof receives its whole support exactly once, in registers aligned with it; at most two chunks add to
  a dof; a stored dof is written by one chunk and by nothing else; every chunk is at least P spans long.
- ``apply_window``: the events applied to numbers (store overwrites, add adds onto zeros), for the comparison with the dense
  contraction.
- ``collocation_ld``: values and first derivatives of every basis function at given nodes in long double (Cox-de Boor on the
  host: nothing of the library is involved), dense.
- ``contract_ld``: the load vector  C_0^T (x) C_1^T (x) C_2^T T  in long double from the dense matrices (the zero blocks of a
  span's rows are skipped: the sum is the same).
"""
import numpy as np

LD = np.longdouble


def window_events(a1, clen, nch):
    """The writes of k_lv12 for one Gauss plane and one lane, as the kernel orders them inside a chunk."""
    P, q, n, N = a1.P, a1.q, a1.n, a1.N
    fa, mslo = a1.fa, a1.mslo
    events = []
    for ch in range(nch):
        s_a = ch * clen
        s_b = n if ch == nch - 1 else s_a + clen
        acc = [[] for _ in range(P)]
        sp, l = s_a, 0
        for g1 in range(s_a * q, s_b * q):
            for a in range(P):
                acc[a].append((g1, a))
            l += 1
            if l < q:
                continue
            base = int(fa[sp])
            if sp + 1 < n:
                nleave = int(fa[sp + 1]) - base if sp + 1 < s_b else P
            else:
                nleave = P
            for j in range(nleave):
                i1 = base + j
                if i1 < N:
                    whole = mslo[i1] >= s_a and (sp + 1 < s_b or sp + 1 == n or j < int(fa[min(sp + 1, n - 1)]) - base)
                    events.append((ch, i1, 'store' if whole else 'add', tuple(acc[0])))
                acc = acc[1:] + [[]]
            l = 0
            sp += 1
    return events


def chunk_lengths(a1, clen, nch):
    return [(a1.n if ch == nch - 1 else (ch + 1) * clen) - ch * clen for ch in range(nch)]


def check_window(a1, clen, nch):
    """Assert the properties the kernel's comment claims; returns the number of added (shared) dofs."""
    P, q = a1.P, a1.q
    assert nch >= 1 and (nch - 1) * clen < a1.n
    assert min(chunk_lengths(a1, clen, nch)) >= P, ('a chunk shorter than P spans', clen, nch, a1.n)
    got = {}
    for ch, i1, kind, terms in window_events(a1, clen, nch):
        for g1, a in terms:                       # the register was aligned with the dof it is written to
            assert int(a1.fa[g1 // q]) + a == i1, (ch, i1, g1, a)
        got.setdefault(i1, []).append((ch, kind, terms))
    assert sorted(got) == list(range(a1.N)), 'a dof of the mid axis is never written'
    shared = 0
    for i1, writes in got.items():
        support = [(g1, i1 - int(a1.fa[g1 // q])) for g1 in range(int(a1.mslo[i1]) * q, int(a1.mshi[i1]) * q)]
        terms = sorted(t for _, _, ts in writes for t in ts)
        assert terms == support, ('dof %d does not receive its support exactly once' % i1, clen, nch)
        kinds = [k for _, k, _ in writes]
        if 'store' in kinds:
            assert len(writes) == 1, ('a stored dof is written twice', i1, writes)
        else:
            assert len(writes) <= 2 and len({ch for ch, _, _ in writes}) == len(writes), ('more than two addends', i1)
            shared += 1
    return shared


def apply_window(a1, clen, nch, V1, r, order=None):
    """t2[i1] from the line values r[g1] (already contracted along the last axis) and the table V1[g1][a]; chunks in `order`."""
    out = np.zeros(a1.N)
    events = window_events(a1, clen, nch)
    chunks = list(range(nch)) if order is None else list(order)
    for c in chunks:
        for ch, i1, kind, terms in events:
            if ch != c:
                continue
            v = 0.0
            for g1, a in terms:
                v = v + V1[g1, a] * r[g1]
            if kind == 'store':
                out[i1] = v
            else:
                out[i1] += v
    return out


# ---------------------------------------------------------------------------------------------
# the long-double reference
def _basis_ld(kn, p, i, x):
    """The p + 1 non-zero B-splines of degree p at x (knot span i: kn[i] <= x < kn[i+1]), arrays over the nodes."""
    m = x.shape[0]
    Nv = np.zeros((p + 1, m), dtype=LD)
    Nv[0] = 1
    left = np.zeros((p + 1, m), dtype=LD)
    right = np.zeros((p + 1, m), dtype=LD)
    for j in range(1, p + 1):
        left[j] = x - kn[i + 1 - j]
        right[j] = kn[i + j] - x
        saved = np.zeros(m, dtype=LD)
        for r in range(j):
            temp = Nv[r] / (right[r + 1] + left[j - r])
            Nv[r] = saved + right[r + 1] * temp
            saved = left[j - r] * temp
        Nv[j] = saved
    return Nv


def collocation_ld(kv, nodes):
    """(2, G, N) long double: values and first derivatives of all basis functions of `kv` at `nodes` (dense)."""
    kn = np.asarray(kv.kv, dtype=np.float64).astype(LD)
    p = int(kv.p)
    x = np.asarray(nodes, dtype=np.float64).astype(LD)
    N = kn.size - p - 1
    i = np.clip(np.searchsorted(kn, x, side='right') - 1, p, N - 1)
    vals = _basis_ld(kn, p, i, x)                                # dofs i - p .. i
    ders = np.zeros_like(vals)
    if p >= 1:
        low = _basis_ld(kn, p - 1, i, x)                         # degree p - 1: dofs i - p + 1 .. i
        for k in range(p + 1):
            d = np.zeros(x.shape[0], dtype=LD)
            if k >= 1:
                d = d + low[k - 1] / (kn[i + k] - kn[i - p + k])
            if k < p:
                d = d - low[k] / (kn[i + k + 1] - kn[i - p + k + 1])
            ders[k] = p * d
    C = np.zeros((2, x.shape[0], N), dtype=LD)
    rows = np.arange(x.shape[0])
    for k in range(p + 1):
        C[0, rows, i - p + k] = vals[k]
        C[1, rows, i - p + k] = ders[k]
    return C


def _contract_axis(C, q, T, axis, lo=0, hi=None):
    """out[.., i, ..] = sum_g C[g][i] T[.., g, ..] for lo <= i < hi: span by span, skipping the columns that are zero on a span."""
    T = np.moveaxis(T, axis, 0)
    G, N = C.shape
    hi = N if hi is None else hi
    out = np.zeros((N,) + T.shape[1:], dtype=LD)
    flat = T.reshape(G, -1)
    o = out.reshape(N, -1)
    for s in range(G // q):
        blk = C[s * q:(s + 1) * q]
        cols = np.flatnonzero((blk != 0).any(axis=0))
        if cols.size:
            o[cols] += blk[:, cols].T.dot(flat[s * q:(s + 1) * q])
    return np.moveaxis(out[lo:hi], 0, axis)


def contract_ld(Cs, q, T, derivs=None, absolute=False, g0_lo=0):
    """C_0^T (x) C_1^T [(x) C_2^T] T in long double; derivs[k] = 1 takes the derivative table on axis k; absolute: |C|, |T|
    (the bound's B).  T covers the Gauss planes g0_lo .. of axis 0."""
    dim = len(Cs)
    derivs = derivs or (0,) * dim
    out = np.asarray(T, dtype=LD)
    if absolute:
        out = abs(out)
    for k in reversed(range(dim)):
        C = Cs[k][derivs[k]]
        if absolute:
            C = abs(C)
        if k == 0:
            C = C[g0_lo:g0_lo + out.shape[0]]
        out = _contract_axis(C, q, out, k)
    return out

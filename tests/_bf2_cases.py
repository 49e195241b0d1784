"""The instantiations of k_bf2, k_mirror and k_mirror2 (pyiga_amd/csrc/fused.hip) and small patches shaped for their edges.

Plain helper module (not a conftest): ``tests/test_bf2_coverage_cpu.py`` checks that the tables below and the dispatch of
``launch_bf`` / ``launch_bf2_p`` / ``launch_mirror`` cannot drift apart and that every case has the tile and chunk counts it is
there for; ``tests/test_bf2_kernels_gpu.py`` assembles every case on the device.

What reaches fused.hip (sumfact.hip: sumfact_plan).  k_bf3 takes the symmetric forms in 2D and 3D and the merged non-symmetric
3D forms; ``Plan::BF2`` (k_bf2, then the mirror pass for symmetric forms) is left with
  * a 3D patch ``fused3_offsets_fit`` refuses and ``fused_offsets_fit`` accepts (row blocks of about 0.9 .. 2 GB: no test can
    assemble one);
  * IGX_BF=2 (``fused3_axes`` is false), in 2D together with IGX_PATH=fused (``fused_applicable`` wants it there); the 3D
    convection-diffusion form then runs k_bf2 on its merged slots, without a mirror pass;
  * a non-symmetric form on a 2D patch under IGX_PATH=fused whose slots are the full first-order set 0x135F: ``fused3_axes``
    refuses non-symmetric 2D forms.  This is also the only way to TWO arrays in one slot (na = 2): a parametric jet form
    (igx_patch_set_pform) that names a pair of masks twice.  In 3D the non-symmetric forms merge two terms of a slot into one
    array (with or without k_geoA) and a third one sends the form to the stage kernels, and the symmetric kinds have one term
    per slot.

A k_bf2 instantiation is picked by (P, mask, na): P = degree + 1 of the swept (mid) and the last axis, the slot mask of the form
(bit 4 y + t1: an array enters the sweep with last-axis type y and mid-axis type t1) and the arrays per slot.  The mirror pass
is picked by WW = 2 p + 1: k_mirror2<WW, VAR> on a 3D patch for the widths its switch lists, k_mirror<WW> otherwise.
"""
import collections
import os
import re

import _bf3_cases as bc

FUSED_HIP = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'pyiga_amd', 'csrc', 'fused.hip')

Key = collections.namedtuple('Key', 'P mask na')                 # k_bf2<P, NY, mask, na>: NY = 1 for the mass mask, else 4
Mirror = collections.namedtuple('Mirror', 'kernel WW VAR')       # k_mirror<WW> (VAR None) or k_mirror2<WW, VAR>
Route = collections.namedtuple('Route', 'key mirror geoA')

SLOTS = (256, 512, 768, 1024)        # one to four resident blocks of k_bf2 on each of the chip's 256 CUs
NCU = 256


# ---- the terms of a form and their slots (sumfact_stages.h: form_terms; sumfact.hip: sumfact_plan, add_slot)
def _stiffness_types(dim):
    return [tuple((k == a) + 2 * (k == b) for k in range(dim)) for a in range(dim) for b in range(dim)]


def form_slots(dim, kind, pterms=None):
    """{(y, t1): arrays} of the sweep: last-axis type y, mid-axis type t1 (type = tu + 2 tv).  kind 'pform': pterms is the
    list of (mask_v, mask_u) of a parametric jet form, bit a of a mask differentiates grid axis a."""
    if kind == 'mass':
        types = [(0,) * dim]
    elif kind == 'stiffness':
        types = _stiffness_types(dim)
    elif kind == 'convdiff':                         # stiffness + (beta . grad u) v
        types = _stiffness_types(dim) + [tuple(int(k == a) for k in range(dim)) for a in range(dim)]
    elif kind == 'pform':
        types = [tuple(((mu >> a) & 1) + 2 * ((mv >> a) & 1) for a in range(dim)) for mv, mu in pterms]
    else:
        raise ValueError(kind)
    slots = collections.Counter()
    for t in types:
        slots[(0 if kind == 'mass' else t[dim - 1], t[dim - 2])] += 1
    return dict(slots)


def bf_signature(slots):
    """fused.hip: bf_signature -> (ny, mask, na)."""
    mask = sum(1 << (4 * y + t1) for (y, t1) in slots)
    return (1 if max(y for y, _ in slots) == 0 else 4), mask, max(slots.values())


def fused_supported(ny, mask, na, masks):
    """fused.hip: fused_supported."""
    return (ny == 1 and mask == masks['MASS'] and na == 1) or (ny == 4 and mask == masks['STIFF3'] and na <= 2) or \
           (ny == 4 and mask == masks['STIFF2'] and na == 1)


def _pairs(N, p):
    """1D index pairs (i, j) of an axis with single interior knots (Axis::S)."""
    return N * (2 * p + 1) - p * (p + 1)


def fused_offsets_fit(c0max, S_mid, S_last, G_mid, G_last):
    """fused.hip: fused_offsets_fit (tests/test_abi_cpu.py compares the compiled one with the same arithmetic)."""
    LIM = 0x7fff0000
    if max(S_mid, S_last, G_mid, G_last) > LIM:
        return False
    return c0max * S_mid <= LIM // 8 and c0max * S_mid * S_last <= LIM // 8 and G_mid * G_last <= LIM // 8


def _knobs(knobs):
    k = dict(knobs or {})
    assert set(k) <= {'IGX_PATH', 'IGX_BF'}, k
    return {None: 0, 'fused': 1, 'unfused': 2, 'single': 3}[k.get('IGX_PATH')], int(k.get('IGX_BF', '0'))


def fused_applicable(axes, path):
    """sumfact.hip: fused_applicable: single knots, equal degrees and q = P on the swept and the last axis, P = 2 .. 6, the
    32-bit offsets; in 2D on request only."""
    dim = len(axes)
    if path == 2 or (dim == 2 and path != 1):
        return False
    q = max(a[0] for a in axes) + 1
    (p1, n1, _), (p2, n2, _) = axes[dim - 2], axes[dim - 1]
    if bc.repeated(axes[dim - 2]) or bc.repeated(axes[dim - 1]) or p1 + 1 != q or p2 + 1 != q or not 2 <= q <= 6:
        return False
    return fused_offsets_fit(2 * axes[0][0] + 1 if dim == 3 else 1, _pairs(n1 + p1, p1), _pairs(n2 + p2, p2), n1 * q, n2 * q)


def bf2_route(axes, kind, knobs, pterms=None, src=None):
    """What sumfact_plan and launch_mirror run from fused.hip for a spline patch on a cylinder / twisted box / quarter annulus
    (specs (p, n, rep)): Route(k_bf2 key, mirror kernel or None, k_geoA in front), or None where another chain takes the patch.
    (Small patches: fused3_offsets_fit holds, so k_bf3 takes every patch it has a kernel for unless IGX_BF=2.)"""
    d = parse_dispatch(src)
    path, bf = _knobs(knobs)
    dim = len(axes)
    sym = kind in ('mass', 'stiffness')
    if not fused_applicable(axes, path):
        return None
    # fused3_axes: the bf == 2 branch; in 2D only symmetric forms under IGX_PATH=fused (equal degrees: fused3_degrees holds)
    axes3 = bf != 2 and (dim == 3 or sym)
    if axes3:
        return None
    slots = form_slots(dim, kind, pterms)
    if dim == 3 and not sym:
        # merged slots: two terms of a slot become one K1 array with two sources, a third one leaves the fused stage
        if max(slots.values()) > 2:
            return None
        slots = dict.fromkeys(slots, 1)
    ny, mask, na = bf_signature(slots)
    if na > 2 or not fused_supported(ny, mask, na, d['masks']):
        return None
    P = axes[dim - 1][0] + 1
    key = Key(P, {v: k for k, v in d['masks'].items()}[mask], na)
    mirror = None
    if sym:
        WW = 2 * P - 1
        (p1, n1, _), (p2, n2, _) = axes[dim - 2], axes[dim - 1]
        if dim == 3 and fused_offsets_fit(2 * axes[0][0] + 1, _pairs(n1 + p1, p1), _pairs(n2 + p2, p2), 0, 0) and WW in d['mirror2']:
            mirror = Mirror('k_mirror2', WW, d['mirror2'][WW])
        else:
            mirror = Mirror('k_mirror', WW, None)
    # k_geoA (geoa.hip: geoA_supported) in front of the 3D symmetric kinds: degree 1 .. 5 on axis 0, a geometry of degree 1 or 2
    # along axis 0 with at most half as many spans as axis 0 has Gauss points (the cylinder and the twisted box: one span)
    # (the convection-diffusion form: from degree 2 on)
    geoA = dim == 3 and (1 if sym else 2) <= axes[0][0] <= 5
    return Route(key, mirror, geoA)


# ---- fused.hip, read from the source
def read_source(path=FUSED_HIP):
    with open(path) as f:
        return f.read()


def _func(src, start, end='\n}\n'):
    s = src[src.index(start):]
    return s[:s.index(end)]


def _ternary(expr, env):
    """Value of a C expression made of integers, names of env, `NAME == int ? a : b` and parentheses."""
    expr = expr.strip()
    while expr.startswith('(') and _close(expr, 0) == len(expr) - 1:
        expr = expr[1:-1].strip()
    depth, q = 0, -1
    for i, c in enumerate(expr):
        depth += {'(': 1, ')': -1}.get(c, 0)
        if c == '?' and depth == 0:
            q = i
            break
    if q < 0:
        return env[expr] if expr in env else int(expr, 0)
    depth, nest, colon = 0, 0, -1
    for i in range(q + 1, len(expr)):
        c = expr[i]
        depth += {'(': 1, ')': -1}.get(c, 0)
        if depth == 0 and c == '?':
            nest += 1
        if depth == 0 and c == ':':
            if nest == 0:
                colon = i
                break
            nest -= 1
    name, val = [s.strip() for s in expr[:q].split('==')]
    return _ternary(expr[q + 1:colon], env) if env[name] == int(val) else _ternary(expr[colon + 1:], env)


def _close(s, i):
    depth = 0
    for k in range(i, len(s)):
        depth += {'(': 1, ')': -1}.get(s[k], 0)
        if depth == 0:
            return k
    return -1


def _define(src, name):
    return int(re.search(r'#define %s (\d+)' % name, src).group(1))


_PARSED = {}


def parse_dispatch(src=None):
    """The instantiation sets of fused.hip:
         'P'        the `case` lines of launch_bf
         'sets'     (NY, mask name, NA) of the four `if` lines of launch_bf2_p (condition and template arguments agree)
         'masks'    BF_MASK_* by name
         'mirror2'  {WW: VAR} of the first switch of launch_mirror, 'mirror1' the WW of the second
         'rcm1'     {WW: RCM} of MirrorGeom, 'rcm2' {WW: RCM} of Mirror2Geom at the VAR launched, 'IB', 'VAR'."""
    if src is None and None in _PARSED:
        return _PARSED[None]
    text = read_source() if src is None else src
    d = {}
    m = re.search(r'constexpr int BF_MASK_MASS = (\w+), BF_MASK_STIFF3 = (\w+), BF_MASK_STIFF2 = (\w+);', text)
    d['masks'] = dict(zip(('MASS', 'STIFF3', 'STIFF2'), (int(v, 16) for v in m.groups())))
    body = _func(text, 'int launch_bf(hipStream_t st')
    cases = re.findall(r'case (\d+): return launch_bf2_p<(\d+)>\(', body)
    assert cases and all(a == b for a, b in cases), cases
    d['P'] = {int(a) for a, _ in cases}
    body = _func(text, 'static int launch_bf2_p(')
    sets = set()
    lines = re.findall(r'if \(ny == (\d) && mask == BF_MASK_(\w+) && na == (\d)\) return launch_bf2_c<P, (\d), BF_MASK_(\w+), (\d)>\(', body)
    assert len(lines) == body.count('return launch_bf2_c<'), body
    for ny, mk, na, tny, tmk, tna in lines:
        assert (ny, mk, na) == (tny, tmk, tna), (ny, mk, na, tny, tmk, tna)
        sets.add((int(ny), mk, int(na)))
    d['sets'] = sets
    d['VAR'], d['IB'] = _define(text, 'MIRROR_VAR'), _define(text, 'MIRROR_IB')
    body = _func(text, 'int launch_mirror(hipStream_t st')
    first, second = body.split('switch (2 * AL.p + 1)')[1:]
    d['mirror2'] = {int(a): (d['VAR'] if v == 'MIRROR_VAR' else int(v))
                    for a, b, v in re.findall(r'case (\d+): return launch_mirror2_k<(\d+), (\w+)>\(', first) if a == b}
    assert len(d['mirror2']) == first.count('launch_mirror2_k<') and 'launch_mirror_k<' not in first
    d['mirror1'] = {int(a) for a, b in re.findall(r'case (\d+): return launch_mirror_k<(\d+)>\(', second) if a == b}
    assert len(d['mirror1']) == second.count('launch_mirror_k<')
    # the 3D branch is the one that may take k_mirror2
    assert re.search(r'if \(pt->dim == 3 && fused_offsets_fit\(c0max, AM\.S, AL\.S, 0, 0\)\) \{\s*#endif\s*switch', body)
    g1 = re.search(r'struct MirrorGeom \{\s*static constexpr int RCM = ([^;]+);', text).group(1)
    g2 = re.search(r'struct Mirror2Geom \{\s*static constexpr int RCM = ([^;]+);', text).group(1)
    d['rcm1'] = {WW: _ternary(g1, {'WW': WW}) for WW in d['mirror1']}
    d['rcm2'] = {WW: _ternary(g2, {'WW': WW, 'VAR': VAR}) for WW, VAR in d['mirror2'].items()}
    # the launch arithmetic restated in mirror_plan
    assert '(1536 + base - 1) / base, std::max(1, rows / 8)' in _func(text, 'static int launch_mirror_k(')
    assert '(2048 + base - 1) / base, std::max(1, rows / 8)' in _func(text, 'static int launch_mirror2_k(')
    if src is None:
        _PARSED[None] = d
    return d


def compiled_bf2_keys(d=None):
    d = d or parse_dispatch()
    return {Key(P, mk, na) for P in d['P'] for _, mk, na in d['sets']}


def compiled_mirror_keys(d=None):
    d = d or parse_dispatch()
    return {Mirror('k_mirror2', WW, VAR) for WW, VAR in d['mirror2'].items()} | {Mirror('k_mirror', WW, None) for WW in d['mirror1']}


# entries: key -> the reason no patch can launch it
UNREACHABLE = {}


# ---- launch arithmetic
def rows_per_tile(cdll, key, d=None):
    """BF2Geom::RMAX of the instantiation: the library's own arithmetic (igx_fused_rows_per_tile)."""
    d = d or parse_dispatch()
    r = cdll.igx_fused_rows_per_tile(key.P, d['masks'][key.mask], key.na)
    assert r >= 1, (key, r)
    return r


def chunk_plan(cdll, npairs, ntiles, mid_rows, slots, P):
    """(mrows, nmchunks, main_blocks, tail_k, tail_mrows) of bf2_choose_chunks (igx_fused_chunk_plan)."""
    import ctypes
    out = (ctypes.c_int * 5)()
    rc = cdll.igx_fused_chunk_plan(npairs, ntiles, mid_rows, slots, P, out)
    assert rc == 0, (rc, npairs, ntiles, mid_rows, slots, P)
    return tuple(out)


def mirror_plan(mirror, ntp, rows, N2, d=None):
    """launch_mirror_k / launch_mirror2_k: (RC, nchunks, i1_rows, ni1) for ntp target pairs, `rows` target rows of the mid axis
    and N2 dofs of the last axis."""
    d = d or parse_dispatch()
    rcm = d['rcm2'][mirror.WW] if mirror.kernel == 'k_mirror2' else d['rcm1'][mirror.WW]
    want = 2048 if mirror.kernel == 'k_mirror2' else 1536
    nchunks = (N2 + rcm - 1) // rcm
    RC = (N2 + nchunks - 1) // nchunks
    base = ntp * nchunks
    ni1 = max(1, min((want + base - 1) // base, max(1, rows // 8)))
    i1_rows = (rows + ni1 - 1) // ni1
    return RC, nchunks, i1_rows, (rows + i1_rows - 1) // i1_rows


def outer_pairs(axes):
    """Outer pairs of a symmetric form: (i0, j0 <= i0) of axis 0 in 3D (as many targets j0 >= i0 for the mirror pass), the one
    trivial pair in 2D."""
    if len(axes) == 2:
        return 1
    p0, n0, _ = axes[0]
    return (n0 + p0) * (p0 + 1) - p0 * (p0 + 1) // 2


def launch_shape(cdll, case, slots):
    """Tile, chunk and mirror-chunk counts of the whole patch of a case on a chip that holds `slots` blocks of k_bf2."""
    d = parse_dispatch()
    dim = len(case.axes)
    N = [bc.numdofs(a) for a in case.axes]
    rmax = rows_per_tile(cdll, case.key, d)
    ntiles = (N[-1] + rmax - 1) // rmax
    npairs = outer_pairs(case.axes) if case.mirror else 1
    mid_rows = N[dim - 2]
    mrows, nmchunks, main_blocks, tail_k, tail_mrows = chunk_plan(cdll, npairs, ntiles, mid_rows, slots, case.key.P)
    out = dict(rmax=rmax, ntiles=ntiles, R2=(N[-1] + ntiles - 1) // ntiles, npairs=npairs, mid_rows=mid_rows, mrows=mrows,
               nmchunks=nmchunks, main_blocks=main_blocks, tail_k=tail_k, tail_mrows=tail_mrows)
    if case.mirror:
        RC, nch, i1_rows, ni1 = mirror_plan(case.mirror, npairs, mid_rows, N[-1], d)
        out.update(RCM=(d['rcm2'] if case.mirror.kernel == 'k_mirror2' else d['rcm1'])[case.mirror.WW], RC=RC, mchunks=nch,
                   i1_rows=i1_rows, ni1=ni1)
    return out


# ---- the cases
# want: what the case is there for, checked on the CPU with the library's launch arithmetic (test_bf2_coverage_cpu.py):
#   'tiles': n     tiles of the last axis          'full_tile'   N2 == RMAX         'edge_rows'  N2 <= 2 p (no interior row)
#   'chunked'      nmchunks > 1 at every slots     'one_chunk'   mid axis of one span
#   'mchunks': n   chunks of the mirror pass       'full_mchunk' N2 == RCM          'ni1'        ni1 >= 2
#   'ragged'       k_mirror2: i1_rows % IB != 0    'tail'        tail_k > 0 at every slots
Case = collections.namedtuple('Case', 'id axes geo kind knobs key mirror want slabs pterms')

KNOBS_3D = {'IGX_BF': '2'}
KNOBS_2D = {'IGX_PATH': 'fused', 'IGX_BF': '2'}
KNOBS_NA2 = {'IGX_PATH': 'fused'}
GEOS = {3: ('cylinder', 'twisted_box'), 2: ('quarter_annulus', 'bspline_quarter_annulus')}

# Tile heights BF2Geom::rmax() by (mask, na) for P = 2 .. 6, worked out by hand from fused.hip: only to shape the table below
# without the library; test_bf2_coverage_cpu.py compares them with igx_fused_rows_per_tile, which the tests rely on.
RMAX = {('MASS', 1): (63, 40, 29, 34, 16), ('STIFF3', 1): (63, 40, 29, 33, 16), ('STIFF3', 2): (63, 40, 29, 21, 16),
        ('STIFF2', 1): (63, 40, 29, 21, 16)}
RCM1 = {3: 128, 5: 128, 7: 112, 9: 66, 11: 40}
RCM2 = {5: 64, 7: 56, 9: 33}

# the nine terms (mask_v, mask_u) of the full first-order jet of a 2D form -- jet index r: 0 the value, 1 d/dx (the last grid
# axis, mask 2), 2 d/dy (axis 0, mask 1) -- and the entry named twice
JET_MASK = (0, 2, 1)
NA2_TWICE = ((1, 2), (0, 0), (2, 2))              # (r, s) of the table entries given as two arrays


def na2_pterms():
    """(r, s, half) of the terms of the na = 2 form: every entry (r, s) of the 3 x 3 table once, those of NA2_TWICE as two
    halves whose coefficients add up to the entry."""
    out = []
    for r in range(3):
        for s in range(3):
            out.append((r, s, 0))
            if (r, s) in NA2_TWICE:
                out.append((r, s, 1))
    return out


# coefficients of the table (functions of the physical point = the parameters on the unit square): entry (r, s) multiplies
# D_r v D_s u; not symmetric, the 2 x 2 block of second-order entries positive definite
NA2_TABLE = [['2.0 + x * y', '0.25 * x', '1.0 + y'],
             ['y', '1.5 + x', '0.25 * y'],
             ['-0.5 * x', '0.5 * x', '2.0 + y * y']]
NA2_SPLIT = '0.375 + 0.25 * x * y'                # first half of a split entry as a fraction of it (the second: one minus it)


def _tag(kind, axes, geo, extra=''):
    return '%s-%s-%s%s' % (kind, '-'.join('p%dn%d' % (p, n) for p, n, _ in axes), geo, extra)


def _mk(kind, axes, geo, want, slabs=None, extra=''):
    dim = len(axes)
    pterms = None
    if kind == 'pform':
        knobs, pterms = KNOBS_NA2, na2_pterms()
        key = Key(axes[-1][0] + 1, 'STIFF3', 2)
        mirror = None
    else:
        knobs = KNOBS_3D if dim == 3 else KNOBS_2D
        P = axes[-1][0] + 1
        key = Key(P, 'MASS' if kind == 'mass' else 'STIFF3' if dim == 3 else 'STIFF2', 1)
        WW = 2 * P - 1
        mirror = Mirror('k_mirror2', WW, 1 if WW == 9 else 0) if dim == 3 and WW in RCM2 else Mirror('k_mirror', WW, None)
        if kind == 'convdiff':
            mirror = None
    return Case(_tag(kind, axes, geo, extra), tuple(axes), geo, kind, dict(knobs), key, mirror, dict(want), slabs, pterms)


def _edge_cases():
    """Every reachable k_bf2 instantiation on five sizes of the last axis -- one span; 2 p dofs (every row an edge row); RMAX (one
    full tile); RMAX + 1 (two tiles of the rebalanced height); 2 RMAX + 1 (three) -- with the other axes alternating: the swept
    axis one span or 4 P and more dofs (cut into chunks), axis 0 of lower degree or one span, the geometries in turn."""
    out = []
    for dim, kinds in ((3, ('mass', 'stiffness')), (2, ('mass', 'stiffness', 'pform'))):
        for kind in kinds:
            for p in range(1, 6):
                P = p + 1
                mk = 'MASS' if kind == 'mass' else 'STIFF3' if dim == 3 or kind == 'pform' else 'STIFF2'
                rmax = RMAX[(mk, 2 if kind == 'pform' else 1)][p - 1]
                sizes = [(p + 1, dict(tiles=1, edge_rows=True)), (2 * p, dict(tiles=1, edge_rows=True)), (rmax, dict(tiles=1, full_tile=True)),
                         (rmax + 1, dict(tiles=2)), (2 * rmax + 1, dict(tiles=3))]
                seen = set()
                for k, (N2, want) in enumerate(sizes):
                    if N2 in seen:
                        continue
                    seen.add(N2)
                    chunked = k in (0, 3, 4)
                    n_mid = 4 * P + (0, 0, 0, 3, 1)[k] - p if chunked else 1      # 4 P, 4 P + 3, 4 P + 1 dofs, or one span
                    want = dict(want, **({'chunked': True} if chunked else {'one_chunk': True}))
                    if dim == 3:
                        # axis 0: a lower degree (from p = 2 on) on several spans or on one; one span of degree 1 next to the long axes
                        ax0 = [(max(1, p - 1), 3, 1), (max(1, p - 1), 1, 1), (1, p + 1, 1), (1, 1, 1), (1, 1, 1)][k]
                        axes = (ax0, (p, n_mid, 1), (p, N2 - p, 1))
                    else:
                        axes = ((p, n_mid, 1), (p, N2 - p, 1))
                    geo = 'unit_square' if kind == 'pform' else GEOS[dim][k % 2]
                    out.append(_mk(kind, axes, geo, want))
    return out


def _mirror_cases():
    """Every mirror instantiation with N2 = RCM (one chunk) and RCM + 1 (two chunks of the rebalanced height) and 16 or more rows
    on the mid axis (ni1 >= 2); k_mirror2 once with i1_rows a multiple of IB = 3 and once not (the last group repeats a row it
    must not write)."""
    out = []
    for p in range(1, 6):
        WW = 2 * p + 1
        rcm3 = RCM2.get(WW, RCM1[WW])
        # 3D: three target pairs (axis 0: one span of degree 1); 18 rows -> two blocks of 9 = 3 groups of 3, 16 -> 8 = 3 + 3 + 2
        out.append(_mk('mass', ((1, 1, 1), (p, 18 - p, 1), (p, rcm3 - p, 1)), 'cylinder', dict(mchunks=1, full_mchunk=True, ni1=True, exact=True), extra='-mirror'))
        out.append(_mk('stiffness' if p <= 3 else 'mass', ((1, 1, 1), (p, 16 - p, 1), (p, rcm3 + 1 - p, 1)), 'twisted_box',
                       dict(mchunks=2, ni1=True, ragged=True), extra='-mirror'))
        # 2D: k_mirror<WW>
        out.append(_mk('stiffness', ((p, 16 - p, 1), (p, RCM1[WW] - p, 1)), 'quarter_annulus', dict(mchunks=1, full_mchunk=True, ni1=True), extra='-mirror'))
        out.append(_mk('mass', ((p, 19 - p, 1), (p, RCM1[WW] + 1 - p, 1)), 'bspline_quarter_annulus', dict(mchunks=2, ni1=True), extra='-mirror'))
    return out


# the tail split of bf2_choose_chunks: p = 1 (27 entries per row), 1537 outer pairs x 2 tiles = 3074 blocks per chunk and 8 rows
# on the swept axis: two whole rounds and more for one to six resident blocks per CU (SLOTS asks for four; a block of the
# p = 1 mass kernel has six waves, so a CU holds five at most), the rest of the blocks in two chunks of four rows.  Found with
# igx_fused_chunk_plan (test_bf2_coverage_cpu.py checks it).  9.6 million nonzeros: the oracle takes three seconds.
TAIL_SLOTS = tuple(256 * k for k in range(1, 7))
TAIL_AXES = ((1, 768, 1), (1, 7, 1), (1, 63, 1))


def _tail_case():
    return _mk('mass', TAIL_AXES, 'twisted_box', dict(tiles=2, tail=True), extra='-tail')


def _slab_cases():
    """Row slabs, one 3D and one 2D case per degree.  3D: slabs of axis 0 (the outer pairs).  2D: slabs of the swept axis itself
    (mid_lo, mid_hi = r0_hi + p for the mirror sources, gmid_lo), on a patch that is cut into chunks and two tiles."""
    out = []
    for p in range(1, 6):
        P = p + 1
        kind = 'stiffness' if p % 2 else 'mass'
        rmax = RMAX[('STIFF3' if kind == 'stiffness' else 'MASS', 1)][p - 1]
        axes = ((1, 3, 1), (p, 4 * P + 1 - p, 1), (p, rmax + 1 - p, 1))
        N0 = 4
        out.append(_mk(kind, axes, GEOS[3][p % 2], dict(tiles=2, chunked=True), slabs=sorted({0, 1, N0 // 2, N0}), extra='-slabs'))
        kind = 'mass' if p % 2 else 'stiffness'
        rmax = RMAX[('STIFF2' if kind == 'stiffness' else 'MASS', 1)][p - 1]
        N0 = 4 * P + 3
        axes = ((p, N0 - p, 1), (p, rmax + 1 - p, 1))
        out.append(_mk(kind, axes, GEOS[2][p % 2], dict(tiles=2, chunked=True), slabs=sorted({0, 1, p, N0 // 2, N0 - 1, N0}), extra='-slabs'))
    return out


def _convdiff_cases():
    """The non-symmetric use of k_bf2 in 3D (all outer pairs, no diagonal blocks, no mirror pass): the convection-diffusion form
    under IGX_BF=2, per degree once behind the stage-A kernel with merged slots (axis 0 of degree 1; two tiles, chunks) and once
    behind k_geoA (axis 0 of degree 2 and more; one span on the swept axis, edge rows only)."""
    out = []
    for p in range(1, 6):
        P = p + 1
        rmax = RMAX[('STIFF3', 1)][p - 1]
        out.append(_mk('convdiff', ((1, 2, 1), (p, 4 * P + 1 - p, 1), (p, rmax + 1 - p, 1)), GEOS[3][p % 2], dict(tiles=2, chunked=True)))
        if p >= 2:
            out.append(_mk('convdiff', ((min(p, 2 + p % 2), 5, 1), (p, 1, 1), (p, p, 1)), GEOS[3][(p + 1) % 2], dict(tiles=1, edge_rows=True, one_chunk=True)))
    return out


EDGE_CASES = _edge_cases() + _convdiff_cases()
MIRROR_CASES = _mirror_cases()
TAIL_CASE = _tail_case()
SLAB_CASES = _slab_cases()
BF2_CASES = EDGE_CASES + MIRROR_CASES + [TAIL_CASE] + SLAB_CASES

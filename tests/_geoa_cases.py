"""The instantiations of k_geoA (pyiga_amd/csrc/geoa.hip) and one patch per (instantiation, form).

Plain helper module (not a conftest), the counterpart of ``tests/_bf3_cases.py`` for the first kernel of the chain:
``tests/test_geoa_coverage_cpu.py`` checks that the restatement below and the dispatch of ``launch_geoA`` cannot drift apart,
``tests/test_gpu_parity.py`` assembles every case on the device against the CPU oracle.

A k_geoA instantiation is ``k_geoA<P, NS, P0G, NC, MF, FORM, D2>``:
  * P: degree + 1 of axis 0 (the swept axis);
  * NS: sweep waves -- 8; 1 for the mass form where GA_MASS8 does not apply (P = 6); in 2D 1 (mass) or 4 (stiffness);
  * P0G: degree + 1 of the geometry map along axis 0 (2 or 3);
  * NC: components of the control net (B-spline: dim, NURBS: dim + 1);
  * MF: the matrix-core sweep (opt-in, IGX_GEOA=mfma);
  * FORM: 0 mass / stiffness, 1 convection-diffusion, 2 / 3 non-symmetric / symmetric coefficient table;
  * D2: the 2D chain.
The key of a case is (instantiation, form): the NS = 8 kernels of FORM 0 serve the mass and the stiffness form.
"""
import collections
import math
import os
import re

import numpy as np

import _bf3_cases as bc

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'pyiga_amd', 'csrc')
GEOA_HIP = os.path.join(CSRC, 'geoa.hip')
SUMFACT_HIP = os.path.join(CSRC, 'sumfact.hip')

Key = collections.namedtuple('Key', 'P NS P0G NC MF FORM D2')
FORM_OF = {'mass': 0, 'stiffness': 0, 'convdiff': 1, 'form_nonsym': 2, 'form_sym': 3}

# ---- the restated constants (test_geoa_coverage_cpu.py compares each with the source)
GA_MASS8 = 1                     # geoa.hip: the mass form on the eight-wave block ...
GA_MASS8_MAXP = 5                # ... up to this P (GEOA_P: !(GA_MASS8 && PV <= 5))
P_3D = (2, 6)                    # geoA_supported, 3D: 2 <= P <= 6
P_CONVDIFF_MIN = 3               # ... the convection-diffusion form from P = 3
P_2D = (2, 5)                    # geoA_supported, 2D
P_FORM = (3, 6)                  # geoA_form_supported
P0G_RANGE = (2, 3)               # the geometry's degree + 1 along axis 0, every form
MF_P = (4, 5)                    # the matrix-core branch of launch_geoA: P, p0g == 2, q == P, eight slots
MF_P0G = 2
NC_3D = (3, 4)
NC_2D = (2, 3)
NFT_SYM, NFT_NONSYM = 10, 13     # form_table_plan: fields of a point in LDS (GA_NFT)
CHUNK_WANT = 2048                # sumfact.hip: sweep_chunks
CHUNK_MIN_3D = 4                 # ... chunks of at least 4 P spans (3D)
CHUNK_MIN_2D = 2                 # geoa2d_min_chunk: 2 P spans (2D)
SINGLE2D_MAX_BLOCKS = 256        # sumfact.hip: single2d_wanted (tiles of at most 8 x 8 rows: kern_basis.hip, single2d_plan)


# ---- geometry maps: seeded control nets in numpy, built into both the product's geometry and the oracle's dict
Geo = collections.namedtuple('Geo', 'deg0 knots0 nurbs seed')
_GEO_OTHER_3D = ((2, (0.37,)), (1, (0.61,)))          # degree, interior knots of axes 1 and 2 (not nested in any space mesh)
_GEO_OTHER_2D = ((2, (0.43,)),)


def open_knots(p, interior):
    return np.concatenate([np.zeros(p + 1), np.asarray(interior, dtype=float), np.ones(p + 1)])


def geo_axes(geo, dim):
    """(knots, degree) of every axis of the map."""
    other = _GEO_OTHER_3D if dim == 3 else _GEO_OTHER_2D
    return [(open_knots(geo.deg0, geo.knots0), geo.deg0)] + [(open_knots(p, k), p) for p, k in other]


def geo_gspans(geo):
    """Spans of the map along axis 0 (geoa.hip: gax[0].N - gax[0].P + 1; single knots)."""
    return len(geo.knots0) + 1


def geo_net(geo, dim):
    """(axes, control net with components (x, y[, z]) last, weights or None): a perturbed box, x along the last axis."""
    axes = geo_axes(geo, dim)
    N = [len(k) - p - 1 for k, p in axes]
    grids = np.meshgrid(*(np.linspace(0., 1., n) for n in N), indexing='ij')
    rng = np.random.default_rng(geo.seed)
    if dim == 3:
        z, y, x = grids
        C = np.stack([x * (1.5 + 0.3 * y), y + 0.2 * np.sin(2. * z), z * (1. + 0.25 * x)], axis=-1)
    else:
        y, x = grids
        C = np.stack([x * (1.2 + 0.3 * y), y + 0.15 * np.sin(2. * x)], axis=-1)
    C = C + 0.02 * rng.standard_normal(C.shape)
    w = 1.0 + 0.3 * rng.random(N) if geo.nurbs else None
    return axes, C, w


def product_geo(iga, geo, dim):
    axes, C, w = geo_net(geo, dim)
    kvs = tuple(iga.bspline.KnotVector(k, p) for k, p in axes)
    if geo.nurbs:
        return iga.geometry.NurbsFunc(kvs, C.copy(), w.copy())
    return iga.bspline.BSplineFunc(kvs, C.copy())


def oracle_geo(orc, geo, dim):
    """The oracle's dict(kvs, coeffs, nurbs) from the same arrays (NURBS: premultiplied, weight last)."""
    axes, C, w = geo_net(geo, dim)
    kvs = [orc.KnotVector(k, p) for k, p in axes]
    if geo.nurbs:
        return dict(kvs=kvs, coeffs=np.concatenate([C * w[..., None], w[..., None]], axis=-1), nurbs=True)
    return dict(kvs=kvs, coeffs=C, nurbs=False)


# ---- coefficient tables: 4x4 of None (absent), a constant or an expression in x, y, z -- the same text is C (for
# igx_patch_set_form_expr) and Python (for the oracle)
def _strip(e):
    x = e.strip()
    while len(x) >= 2 and x[0] == '(' and x[-1] == ')':
        depth = 0
        for i, ch in enumerate(x[:-1]):
            depth += 1 if ch == '(' else -1 if ch == ')' else 0
            if depth == 0:
                return x
        x = x[1:-1].strip()
    return x


def _const(e):
    try:
        return float(_strip(e))
    except ValueError:
        return None


def table_symmetry(T):
    """(sym, blocksym) as igx_patch_set_form_expr decides them: entry (r, c) and (c, r) alike -- both absent, the same
    constant or the same expression text."""
    def same(a, b):
        if (a is None) != (b is None):
            return False
        if a is None:
            return True
        ca, cb = _const(a), _const(b)
        if (ca is None) != (cb is None):
            return False
        return ca == cb if ca is not None else a == b
    sym = blocksym = True
    for r in range(4):
        for c in range(r + 1, 4):
            if not same(T[r][c], T[c][r]):
                sym = False
                if r >= 1:
                    blocksym = False
    return sym, blocksym


def form_table_fields(T):
    """sumfact.hip: form_table_plan, the part after the patch checks: (fits, sym, fields, arrays)."""
    sym, blocksym = table_symmetry(T)
    has = lambda r, c: T[r][c] is not None
    any00 = has(0, 0)
    any0s = any(has(0, k) for k in range(1, 4))
    anyr0 = any(has(k, 0) for k in range(1, 4))
    anyrs = any(has(k, c) for k in range(1, 4) for c in range(1, 4))
    fslot, nf = {}, 0
    slot_src = collections.defaultdict(list)
    for a in range(4):
        for b in range(4):
            nz = (any00 if b == 0 else any0s) if a == 0 else (anyr0 if b == 0 else anyrs)
            if not nz:
                continue
            ca, cb = (b, a) if a > b and (sym or (blocksym and b >= 1)) else (a, b)
            if (ca, cb) not in fslot:
                if nf >= (NFT_SYM if sym else NFT_NONSYM):
                    return False, sym, nf + 1, 0
                fslot[(ca, cb)] = nf
                nf += 1
            t = [(1 if (b >= 1 and ax == 3 - b) else 0) + 2 * (1 if (a >= 1 and ax == 3 - a) else 0) for ax in range(3)]
            slot_src[(t[2], t[1])].append((t[0], fslot[(ca, cb)]))
    arrs = []
    for v in slot_src.values():
        if len(v) > 4:
            return False, sym, nf, 0
        v = sorted(v)
        if v not in arrs:
            arrs.append(v)
    if not arrs or len(arrs) > 8:
        return False, sym, nf, len(arrs)
    if not sym and list(slot_src) == [(0, 0)]:
        return False, sym, nf, len(arrs)
    return True, sym, nf, len(arrs)


def table_oracle(T):
    """The table as the oracle takes it: constants, functions of (x, y, z), None."""
    def entry(e):
        if e is None:
            return None
        c = _const(e)
        if c is not None:
            return c
        return lambda x, y, z, e=e: eval(e, {'__builtins__': {}}, dict(x=x, y=y, z=z)) + 0.0 * x
    return [[entry(e) for e in row] for row in T]


def _table(diag=None, d00=None, row0=None, col0=None, offd=None):
    """A table from its parts: diag -> (k, k), d00 -> (0, 0), row0[k] -> (0, k + 1) (convection of u), col0[k] -> (k + 1, 0),
    offd {(r, s): e} -> (r, s) of the diffusion block."""
    T = [[None] * 4 for _ in range(4)]
    if d00 is not None:
        T[0][0] = d00
    for k in range(3):
        if diag is not None:
            T[k + 1][k + 1] = diag[k]
        if row0 is not None and row0[k] is not None:
            T[0][k + 1] = row0[k]
        if col0 is not None and col0[k] is not None:
            T[k + 1][0] = col0[k]
    for (r, s), e in (offd or {}).items():
        T[r][s] = e
    return T


TABLES = {
    # symmetric: constant diffusion, function-valued reaction, absent off-diagonal entries
    'sym_react': _table(diag=('1.5', '2.0', '0.75'), d00='1.0 + x * y'),
    # symmetric anisotropic diffusion with function-valued off-diagonal pairs, no reaction
    'sym_aniso': _table(diag=('2.0 + z', '1.0', '1.5 + 0.25 * x'), offd={(1, 2): '0.25 * y', (2, 1): '0.25 * y', (2, 3): '0.1', (3, 2): '0.1'}),
    # symmetric with every kind of entry: ten fields
    'sym_full': _table(diag=('1.0', '2.0 + x', '1.5'), d00='0.5', row0=('0.3 * z', None, '0.2'), col0=('0.3 * z', None, '0.2'),
                       offd={(1, 3): 'x * z', (3, 1): 'x * z'}),
    # non-symmetric: diffusion + convection of u
    'nonsym_conv': _table(diag=('2.0', '1.0 + 0.5 * z', '1.0'), row0=('y', '-x', '1.0')),
    # non-symmetric, the most GA_NFT holds: reaction, convection both ways (different), symmetric diffusion block -- 13 fields
    'nonsym_13': _table(diag=('1.0 + x * x', '2.0', '1.5'), d00='3.0', row0=('y', '1.0 + z', '0.5'), col0=('-0.5 * x', None, '0.25 * y'),
                        offd={(1, 2): '0.2', (2, 1): '0.2'}),
    # decision edge: a non-symmetric diffusion block and convection both ways -- more than 13 fields: not on the fast chain
    'nonsym_wide': _table(diag=('1.0', '2.0', '1.5'), row0=('y', None, '0.5'), col0=(None, '0.25 * x', None),
                          offd={(1, 2): '0.2', (2, 1): '-0.3 * z'}),
}


# ---- which instantiation a patch runs: sumfact_assemble / assemble_form_table -> launch_geoA, restated
def _axis_info(axes):
    p = [a[0] for a in axes]
    rep = [bc.repeated(a) for a in axes]
    n = [a[1] for a in axes]
    return p, rep, n


def _geo_ok(P, P0G, gspans, G, lo, hi):
    return lo <= P <= hi and P0G_RANGE[0] <= P0G <= P0G_RANGE[1] and 2 * gspans <= G


def single2d_excluded(axes):
    """2D: even the largest tile of the single-launch kernel (8 x 8 rows) needs more than one resident round of blocks, so
    single2d_wanted is false and k_geoA runs."""
    N = [bc.numdofs(a) for a in axes]
    return math.ceil(N[0] / 8) * math.ceil(N[1] / 8) > SINGLE2D_MAX_BLOCKS


def geoa_route(axes, geo, kind, table=None, mfma=False):
    """(key, twin): the k_geoA instantiation a patch of default nqp runs for `kind` (None: no k_geoA -- field kernels and the
    stage-A kernel, or the single-launch 2D kernel), and whether the chain runs on the axis-exchanged twin (repeated knots on
    the last axis only)."""
    dim = len(axes)
    p, rep, n = _axis_info(axes)
    q = max(p) + 1
    P, P0G, G, gsp = p[0] + 1, geo.deg0 + 1, n[0] * q, geo_gspans(geo)
    NC = dim + (1 if geo.nurbs else 0)
    FORM = FORM_OF[kind]
    if dim == 2:
        if kind not in ('mass', 'stiffness') or not single2d_excluded(axes) or not _geo_ok(P, P0G, gsp, G, *P_2D):
            return None, False
        return Key(P, 1 if kind == 'mass' else 4, P0G, NC, False, 0, True), False
    # twin (igx_patch_create): repeated knots on the last axis only; its fast chain needs equal degrees = nqp - 1 on the
    # exchanged axes (fused3_axes of the twin, whose swept axis has repeated knots) and k_geoA (sumfact_twin_kinds)
    twin_axes = not rep[1] and rep[2]
    twin_chain = twin_axes and p[1] == p[2] == q - 1
    if kind in ('mass', 'stiffness'):
        if not _geo_ok(P, P0G, gsp, G, *P_3D):
            return None, False
        NS = 1 if kind == 'mass' and not (GA_MASS8 and P <= GA_MASS8_MAXP) else 8
        MF = mfma and kind == 'stiffness' and P in MF_P and q == P and P0G == MF_P0G
        return Key(P, NS, P0G, NC, MF, 0, False), twin_chain
    key = None
    if kind == 'convdiff':
        # the eight merged slots exist where the fused stage runs: single knots on the last axis, equal degrees = nqp - 1 on
        # the mid and the last axis (fused_applicable / fused3_axes(pt, false)); a twin serves it under the same condition
        if _geo_ok(P, P0G, gsp, G, P_CONVDIFF_MIN, P_3D[1]) and p[1] == p[2] == q - 1 and (not rep[2] or twin_chain):
            key = Key(P, 8, P0G, NC, False, 1, False)
        return key, key is not None and twin_chain
    # a coefficient table (form_table_plan): k_geoA<FORM = 2 | 3>, then k_bf3 -- on the twin if the patch has one
    fits, sym, _, _ = form_table_fields(table)
    if kind != ('form_sym' if sym else 'form_nonsym'):
        raise ValueError('table does not match the form %s' % kind)
    if rep[2]:
        axes_ok = twin_chain                            # (the twin exists only where its mass / stiffness chain does)
    else:
        axes_ok = bc.fused3_degrees(p[1] + 1, p[2] + 1, q, sym, not rep[1])
    if fits and axes_ok and _geo_ok(P, P0G, gsp, G, *P_FORM):
        key = Key(P, 8, P0G, NC, False, 3 if sym else 2, False)
    return key, key is not None and twin_chain


def geoa_key(axes, geo, kind, table=None, mfma=False):
    return geoa_route(axes, geo, kind, table, mfma)[0]


def expect_bf3(axes, kind, key):
    """k_bf3 finishes the chain (3D): the restatement of launch_bf3's choice (tests/_bf3_cases.py); for a table, wherever it is
    on the fast chain.  False in 2D (the stage kernels of the default 2D chain)."""
    if len(axes) == 2:
        return False
    if kind.startswith('form'):
        return key is not None
    return bc.bf3_key(axes, kind) is not None


# ---- the dispatch of geoa.hip, read from the source
def read_source(path=GEOA_HIP):
    with open(path) as f:
        return f.read()


def _body(src, start, end):
    s = src[src.index(start):]
    return s[:s.index(end)]


def _macro_cases(src, name):
    """Arguments of every NAME(...) use between the end of `#define NAME` and `#undef NAME`."""
    start = src.index('#define %s(' % name)
    body = src[start + len(_macro_def(src, name)):src.index('#undef %s' % name)]
    return [tuple(int(v) for v in m.split(',')) for m in re.findall(r'\b%s\(\s*(\d+(?:\s*,\s*\d+)*)\s*\)' % name, body)]


def _macro_def(src, name):
    s = src[src.index('#define %s(' % name):]
    out = []
    for line in s.split('\n'):
        out.append(line)
        if not line.rstrip().endswith('\\'):
            break
    return '\n'.join(out)


def parse_dispatch(src=None):
    """Everything launch_geoA and its helpers decide on, read from geoa.hip."""
    src = src or read_source()
    d = {}
    d['GEOA_P'] = sorted(c[0] for c in _macro_cases(src, 'GEOA_P'))
    d['GEOA_N'] = sorted(c[0] for c in _macro_cases(src, 'GEOA_N'))
    d['GEOA_2D'] = sorted(c[0] for c in _macro_cases(src, 'GEOA_2D'))
    # GEOA_T(P, FORM) under `if (form->sym)` and under `else`
    tb = _body(src, 'if (form->sym) switch', '#undef GEOA_T')
    sym_part, nonsym_part = tb.split('else switch')
    d['GEOA_T_sym'] = sorted(tuple(int(v) for v in m) for m in re.findall(r'GEOA_T\(\s*(\d+)\s*,\s*(\d+)\s*\)', sym_part))
    d['GEOA_T_nonsym'] = sorted(tuple(int(v) for v in m) for m in re.findall(r'GEOA_T\(\s*(\d+)\s*,\s*(\d+)\s*\)', nonsym_part))
    # p0g branches: launch_geoA_g's switch and the ternaries of the FORM >= 1 macros
    g = _body(src, 'static int launch_geoA_g(', '\n}')
    d['p0g_g'] = sorted(int(m) for m in re.findall(r'case (\d+): return launch_geoA_k<P, NS, (?:\d+)>', g))
    assert all(a == b for a, b in re.findall(r'case (\d+): return launch_geoA_k<P, NS, (\d+)>', g)), 'p0g case and template argument differ'
    for name in ('GEOA_T', 'GEOA_N'):
        m = _macro_def(src, name)
        conds = [int(v) for v in re.findall(r'p0g == (\d+) \?', m)]
        args = [int(v) for v in re.findall(r'launch_geoA_k<PV, 8, (\d+), false, (?:FV|\d+)>', m)]
        assert conds == args, (name, conds, args)
        d['p0g_' + name] = sorted(conds)
    m2 = _macro_def(src, 'GEOA_2D')
    d['ns_p0g_2d'] = sorted({(int(a), int(b)) for a, b in re.findall(r'launch_geoA_2d<PV, (\d+), (\d+)>', m2)})
    d['ns_2d_mass'] = sorted({int(a) for a, b in re.findall(r'nslots == 1 \? \(p0g == 2 \? launch_geoA_2d<PV, (\d+), (\d+)>', m2)})
    # nc branches
    k = _body(src, 'static int launch_geoA_k(', '\n}')
    ncs = re.findall(r'k_geoA<P, NS, P0G, (\d+), MF, FORM>', k)
    assert re.search(r'if \(nc == %s\) k_geoA<P, NS, P0G, %s,' % (ncs[0], ncs[0]), k), 'nc branch of launch_geoA_k'
    d['nc_3d'] = sorted(int(v) for v in ncs)
    k2 = _body(src, 'static int launch_geoA_2d(', '\n}')
    ncs2 = re.findall(r'k_geoA<P, NS, P0G, (\d+), false, 0, true>', k2)
    assert re.search(r'if \(nc == %s\) k_geoA<P, NS, P0G, %s,' % (ncs2[0], ncs2[0]), k2), 'nc branch of launch_geoA_2d'
    d['nc_2d'] = sorted(int(v) for v in ncs2)
    # the matrix-core branch
    lg = _body(src, 'int launch_geoA(', '\n} // namespace')
    mf = re.search(r'if \((nslots == 8 && pt->geoa_mf && pt->knobs.geoa_mf && [^{]*)\) \{(.*?)\n    \}', lg, re.S)
    d['mf_cond'] = mf.group(1)
    d['mf_P'] = sorted(int(v) for v in re.findall(r'A0\.P == (\d+)', mf.group(1)))
    d['mf_launch'] = sorted(tuple(int(v) for v in m) for m in re.findall(r'launch_geoA_k<(\d+), (\d+), (\d+), true>', mf.group(2)))
    d['mf_p0g'] = [int(v) for v in re.findall(r'p0g == (\d+)', mf.group(1))]
    d['mf_q_eq_P'] = 'A0.q == A0.P' in mf.group(1)
    # GA_MASS8 and the GEOA_P choice of NS
    d['GA_MASS8'] = int(re.search(r'#define GA_MASS8 (\d+)', src).group(1))
    mp = _macro_def(src, 'GEOA_P')
    m = re.search(r'\(nslots == 1 && !\(GA_MASS8 && PV <= (\d+)\)\) \? launch_geoA_g<PV, (\d+)>\(.*?\) : launch_geoA_g<PV, (\d+)>', mp)
    d['mass8_maxp'], d['ns_mass_one'], d['ns_default'] = int(m.group(1)), int(m.group(2)), int(m.group(3))
    # degree guards
    sup = _body(src, 'bool geoA_supported(', '\n}')
    two, three = sup.split('if (pt->dim != 3')
    m = re.search(r'if \(P < (\d+) \|\| P > (\d+) \|\| p0g < (\d+) \|\| p0g > (\d+)\) return false;', two)
    d['guard_2d'] = tuple(int(v) for v in m.groups())
    d['guard_2d_nslots'] = re.search(r'nslots != \(kind == IGX_MASS \? (\d+) : (\d+)\)', two).groups()
    m = re.search(r'if \(P < (\d+) \|\| P > (\d+)\) return false;', three)
    d['guard_3d_P'] = tuple(int(v) for v in m.groups())
    d['guard_convdiff_min'] = int(re.search(r'kind == IGX_CONVDIFF && \(P < (\d+)', three).group(1))
    m = re.search(r'if \(p0g < (\d+) \|\| p0g > (\d+)\) return false;', three)
    d['guard_3d_p0g'] = tuple(int(v) for v in m.groups())
    d['guard_3d_nslots'] = re.search(r'nslots != \(kind == IGX_MASS \? (\d+) : (\d+)\)', three).groups()
    d['gspans_rule'] = [bool(re.search(r'return 2 \* gspans <= \(long long\)pt->ax\[0\]\.G;', x)) for x in (two, three)]
    fs = _body(src, 'bool geoA_form_supported(', '\n}')
    m = re.search(r'if \(P < (\d+) \|\| P > (\d+) \|\| p0g < (\d+) \|\| p0g > (\d+)\) return false;', fs)
    d['guard_form'] = tuple(int(v) for v in m.groups())
    d['gspans_rule'].append(bool(re.search(r'return 2 \* gspans <= \(long long\)pt->ax\[0\]\.G;', fs)))
    d['GA_NFT'] = int(re.search(r'constexpr int GA_NFT = (\d+);', src).group(1))
    return d


def parse_sumfact(src=None):
    """The constants of sweep_chunks, geoa2d_min_chunk and form_table_plan (sumfact.hip)."""
    if src is None:
        with open(SUMFACT_HIP) as f:
            src = f.read()
    sc = _body(src, 'static SweepChunks sweep_chunks(', '\n}')
    g2 = _body(src, 'static int geoa2d_min_chunk(', '\n}')
    fp = _body(src, 'static FormPlan form_table_plan(', '\n}')
    return {'want': int(re.search(r'const long long want = (\d+);', sc).group(1)),
            'min_len': int(re.search(r'if \(min_len <= 0\) min_len = (\d+) \* P;', sc).group(1)),
            'too_short': int(re.search(r'nspans < (\d+) \* min_len', sc).group(1)),
            'min_2d': int(re.search(r'return v > 0 \? v : (\d+) \* P;', g2).group(1)),
            'nft': tuple(int(v) for v in re.search(r'if \(nf >= \(fp\.sym \? (\d+) : (\d+)\)\) return fp;', fp).groups()),
            'max_src': int(re.search(r'if \(v\.size\(\) > (\d+)\) return fp;', fp).group(1)),
            'max_arr': int(re.search(r'if \(arrs\.empty\(\) \|\| arrs\.size\(\) > (\d+)\) return fp;', fp).group(1))}


FORMS_3D = ('mass', 'stiffness', 'convdiff', 'form_nonsym', 'form_sym')


def reachable_keys(d=None):
    """Every (key, form) a patch can reach, derived from the dispatch of geoa.hip alone."""
    d = d or parse_dispatch()
    keys = set()
    lo, hi = d['guard_3d_P']
    plo, phi = d['guard_3d_p0g']
    P0Gs = [g for g in d['p0g_g'] if plo <= g <= phi]
    for P in d['GEOA_P']:
        if not lo <= P <= hi:
            continue
        for P0G in P0Gs:
            for NC in d['nc_3d']:
                ns_mass = d['ns_mass_one'] if not (d['GA_MASS8'] and P <= d['mass8_maxp']) else d['ns_default']
                keys.add((Key(P, ns_mass, P0G, NC, False, 0, False), 'mass'))
                keys.add((Key(P, d['ns_default'], P0G, NC, False, 0, False), 'stiffness'))
    for P, NS, P0G in d['mf_launch']:
        if P in d['mf_P'] and P0G in d['mf_p0g'] and lo <= P <= hi:
            for NC in d['nc_3d']:
                keys.add((Key(P, NS, P0G, NC, True, 0, False), 'stiffness'))
    for P in d['GEOA_N']:
        if d['guard_convdiff_min'] <= P <= hi:
            for P0G in d['p0g_GEOA_N']:
                if plo <= P0G <= phi:
                    for NC in d['nc_3d']:
                        keys.add((Key(P, 8, P0G, NC, False, 1, False), 'convdiff'))
    flo, fhi, fplo, fphi = d['guard_form']
    for lst, form in ((d['GEOA_T_sym'], 'form_sym'), (d['GEOA_T_nonsym'], 'form_nonsym')):
        for P, F in lst:
            if flo <= P <= fhi:
                for P0G in d['p0g_GEOA_T']:
                    if fplo <= P0G <= fphi:
                        for NC in d['nc_3d']:
                            keys.add((Key(P, 8, P0G, NC, False, F, False), form))
    lo2, hi2, plo2, phi2 = d['guard_2d']
    nsm, nss = (int(v) for v in d['guard_2d_nslots'])
    for P in d['GEOA_2D']:
        if lo2 <= P <= hi2:
            for NS, P0G in d['ns_p0g_2d']:
                if plo2 <= P0G <= phi2:
                    for NC in d['nc_2d']:
                        keys.add((Key(P, NS, P0G, NC, False, 0, True), 'mass' if NS == nsm else 'stiffness'))
    return keys


def kernel_name(key):
    """The demangled name rocprofv3 reports for an instantiation."""
    b = lambda v: 'true' if v else 'false'
    return 'void igx::k_geoA<%d, %d, %d, %d, %s, %d, %s>(igx::GeoAArgs)' % (key.P, key.NS, key.P0G, key.NC, b(key.MF), key.FORM, b(key.D2))


# ---- the chunks of the axis-0 sweep (sumfact.hip: sweep_chunks, geoa2d_min_chunk), restated
def sweep_chunks(blocks_without, nspans, P, min_len=0):
    """(chunk length in spans, number of chunks): blockIdx.y of k_geoA."""
    if min_len <= 0:
        min_len = CHUNK_MIN_3D * P
    if blocks_without >= CHUNK_WANT or nspans < 2 * min_len:
        return nspans, 1
    n = max(min(-(-CHUNK_WANT // blocks_without), nspans // min_len), 1)
    length = -(-nspans // n)
    return length, -(-nspans // length)


def geoa_chunks(axes):
    """The chunks k_geoA sweeps axis 0 of a whole patch in (default nqp)."""
    p, _, n = _axis_info(axes)
    q = max(p) + 1
    NPL = n[1] * q * (n[2] * q if len(axes) == 3 else 1)
    return sweep_chunks(-(-NPL // 64), n[0], p[0] + 1, CHUNK_MIN_2D * (p[0] + 1) if len(axes) == 2 else 0)


# ---- the cases: one per reachable (key, form)
Case = collections.namedtuple('Case', 'id axes geo kind table coeff mfma key twin bf3 slabs edge')
_COEFFS = ('affine', 'expr', 'sampled')


def _mk_case(axes, geo, kind, table=None, coeff=None, mfma=False, edge=False):
    key, twin = geoa_route(axes, geo, kind, TABLES[table] if table else None, mfma)
    ax = '-'.join('p%dn%d%s' % (p, n, '' if rep == 1 else 'm' + ''.join(map(str, np.atleast_1d(rep)))) for p, n, rep in axes)
    gtag = '%s%dg%d' % ('nurbs' if geo.nurbs else 'bsp', geo.deg0, geo_gspans(geo))
    extra = [t for t in (table, coeff, 'mfma' if mfma else None, 'edge' if edge else None) if t]
    tag = '-'.join([kind, ax, gtag] + extra)
    return Case(tag, axes, geo, kind, table, coeff, mfma, key, twin, expect_bf3(axes, kind, key), False, edge)


def _c0(p, n):
    """Multiplicities of the n - 1 interior knots of an axis 0 with repeated knots: double, single, ..., one C^0 knot."""
    m = [1] * (n - 1)
    m[0] = min(2, p)
    m[-1] = p
    return tuple(m)


def _build_cases():
    cases = []
    seed = [100]

    def geo(deg0, nurbs, gsp):
        seed[0] += 1
        knots = {2: (0.41,), 3: (0.29, 0.63), 4: (0.23, 0.52, 0.77)}[gsp]
        return Geo(deg0, knots, nurbs, seed[0])
    i = 0
    # 3D mass and stiffness: P = 2 .. 6, geometry of degree 1 / 2 along axis 0, B-spline / NURBS
    for P in range(2, 7):
        p0 = P - 1
        for deg0 in (1, 2):
            for nurbs in (False, True):
                for kind in ('mass', 'stiffness'):
                    v = i % 5
                    i += 1
                    g = geo(deg0, nurbs, 2 + (i % 2))
                    n0 = 3 + (i % 3)
                    if v == 0 or p0 == 1 and v in (2, 3):       # equal degrees, short mid axis
                        axes = ((p0, n0, 1), (p0, 2, 1), (p0, 4, 1))
                    elif v == 1 and p0 <= 4:                     # axis 0 one degree below nqp - 1
                        axes = ((p0, n0, 1), (p0 + 1, 3, 1), (p0 + 1, 2, 1))
                    elif v == 1:                                 # axis 0 above the others
                        axes = ((p0, n0, 1), (p0 - 1, 3, 1), (p0 - 1, 3, 1))
                    elif v == 2:                                 # repeated knots on axis 0 up to a C^0 knot; the twin
                        axes = ((p0, 4, _c0(p0, 4)), (p0, 3, 1), (p0, 3, 2))
                    elif v == 3:                                 # repeated knots on mid and last axis: stage B + final kernels
                        axes = ((p0, n0, 1), (p0, 3, 2), (p0, 2, p0))
                    else:                                        # unequal degrees on mid and last axis
                        axes = ((p0, n0, 1), (max(p0 - 1, 1), 4, 1), (p0, 3, 1))
                    cases.append(_mk_case(axes, g, kind))
    # the matrix-core sweep: stiffness, P = 4, 5 (q == P), geometry of degree 1 along axis 0
    for P in (4, 5):
        for nurbs in (False, True):
            p0 = P - 1
            axes = ((p0, 4, 1), (p0 - 1, 3, 1), (p0, 3, 1)) if nurbs else ((p0, 3, _c0(p0, 3)), (p0, 3, 1), (p0, 2, 1))
            cases.append(_mk_case(axes, geo(1, nurbs, 2), 'stiffness', mfma=True))
    # convection-diffusion: P = 3 .. 6 (equal degrees on mid and last axis = nqp - 1)
    j = 0
    for P in range(3, 7):
        p0 = P - 1
        for deg0 in (1, 2):
            for nurbs in (False, True):
                v = j % 4
                coeff = _COEFFS[j % 3]
                j += 1
                if v == 0:
                    axes = ((p0, 3, 1), (p0, 2, 1), (p0, 3, 1))
                elif v == 1 and p0 <= 4:                         # axis 0 below the others
                    axes = ((p0, 4, 1), (p0 + 1, 2, 1), (p0 + 1, 3, 1))
                elif v == 1 or v == 2:                           # the twin; a C^0 knot on axis 0
                    axes = ((p0, 4, _c0(p0, 4)), (p0, 2, 1), (p0, 3, p0))
                else:                                            # repeated knots on the mid axis (k_bf3 MULT)
                    axes = ((p0, 3, 1), (p0, 3, 2), (p0, 2, 1))
                cases.append(_mk_case(axes, geo(deg0, nurbs, 2), 'convdiff', coeff=coeff))
    # coefficient tables: P = 3 .. 6
    j = 0
    for form, tables in (('form_sym', ('sym_react', 'sym_aniso', 'sym_full')), ('form_nonsym', ('nonsym_conv', 'nonsym_13'))):
        for P in range(3, 7):
            p0 = P - 1
            for deg0 in (1, 2):
                for nurbs in (False, True):
                    v = j % 4
                    table = tables[j % len(tables)]
                    j += 1
                    if v == 0:
                        axes = ((p0, 3, 1), (p0, 3, 1), (p0, 2, 1))
                    elif v == 1 and p0 <= 4:
                        axes = ((p0, 3, 1), (p0 + 1, 2, 1), (p0 + 1, 3, 1))
                    elif v == 1 or v == 2:                       # the twin; a C^0 knot on axis 0
                        axes = ((p0, 4, _c0(p0, 4)), (p0, 2, 1), (p0, 3, 2))
                    elif form == 'form_sym' and p0 >= 2:         # unequal degrees on mid and last axis (symmetric tables only)
                        axes = ((p0, 3, 1), (p0, 3, 1), (p0 - 1, 4, 1))
                    else:                                        # repeated knots on the mid axis
                        axes = ((p0, 3, 1), (p0, 3, 2), (p0, 2, 1))
                    cases.append(_mk_case(axes, geo(deg0, nurbs, 2), form, table=table))
    # twin cases with a NURBS map of degree 2 along axis 0, every form
    for kind, table, coeff in (('mass', None, None), ('stiffness', None, None), ('convdiff', None, 'sampled'),
                               ('form_sym', 'sym_full', None), ('form_nonsym', 'nonsym_13', None)):
        cases.append(_mk_case(((3, 3, 1), (3, 2, 1), (3, 3, (3, 1))), geo(2, True, 2), kind, table=table, coeff=coeff))
    # 2D: P = 2 .. 5, mass (NS = 1) and stiffness (NS = 4); above the single-launch crossover (a long axis 1)
    k = 0
    for P in range(2, 6):
        p0 = P - 1
        for deg0 in (1, 2):
            for nurbs in (False, True):
                for kind in ('mass', 'stiffness'):
                    v = k % 4
                    k += 1
                    n0 = 9 + (k % 4)
                    if v == 0:
                        a0, p1 = (p0, n0, 1), p0
                    elif v == 1:                                 # axis 0 below axis 1
                        a0, p1 = (p0, n0, 1), min(p0 + 1, 5)
                    elif v == 2 and p0 >= 2:                     # repeated knots on axis 0 up to a C^0 knot
                        a0, p1 = (p0, n0, _c0(p0, n0)), p0
                    else:                                        # axis 1 below axis 0, repeated knots on it
                        a0, p1 = (p0, n0, 1), max(p0 - 1, 1)
                    N0 = bc.numdofs(a0)
                    n1 = (SINGLE2D_MAX_BLOCKS // math.ceil(N0 / 8) + 1) * 8 - p1 + 13
                    a1 = (p1, n1, 1) if v != 3 or p1 < 2 else (p1, n1 // 2, 2)
                    cases.append(_mk_case((a0, a1), geo(deg0, nurbs, 2), kind))
    # decision edges: 2 * gspans == G is taken, one geometry span more is not; a map of degree 3 along axis 0; a non-symmetric
    # table with more than 13 fields
    cases.append(_mk_case(((3, 1, 1), (3, 2, 1), (3, 2, 1)), Geo(1, (0.3,), False, 201), 'stiffness', edge=True))
    cases.append(_mk_case(((3, 1, 1), (3, 2, 1), (3, 2, 1)), Geo(1, (0.3, 0.55), False, 202), 'stiffness', edge=True))
    cases.append(_mk_case(((3, 1, 1), (3, 2, 1), (3, 2, 1)), Geo(1, (0.3, 0.55), True, 203), 'mass', edge=True))
    cases.append(_mk_case(((2, 3, 1), (2, 2, 1), (2, 3, 1)), Geo(3, (0.45,), True, 204), 'mass', edge=True))
    cases.append(_mk_case(((3, 3, 1), (3, 2, 1), (3, 3, 1)), Geo(1, (0.45,), False, 205), 'form_nonsym', table='nonsym_wide', edge=True))
    # row slabs: the first case of every (P, P0G, NC, FORM, D2)
    seen, out = set(), []
    for c in cases:
        t = None if c.key is None else (c.key.P, c.key.P0G, c.key.NC, c.key.FORM, c.key.D2)
        out.append(c._replace(slabs=t is not None and t not in seen))
        seen.add(t)
    return out


GEOA_CASES = _build_cases()
EDGE_NONE = {c.id for c in GEOA_CASES if c.edge and c.key is None}


# ---- the chunked axis-0 sweep: (name, axes of mid and last axis, degree of axis 0, geometry degree / NURBS, form, table / coefficient)
CHUNK_SWEEPS = [
    ('stiffness-p3-nurbs2', ((3, 1, 1), (3, 1, 1)), 3, (2, True), 'stiffness', None),
    ('mass-p4-bsp1', ((4, 1, 1), (4, 1, 1)), 4, (1, False), 'mass', None),
    ('convdiff-p3-nurbs1', ((3, 1, 1), (3, 1, 1)), 3, (1, True), 'convdiff', 'affine'),
    ('form_sym-p4-bsp2', ((4, 1, 1), (4, 1, 1)), 4, (2, False), 'form_sym', 'sym_full'),
    ('stiffness2d-p3-nurbs2', ((3, 700, 1),), 3, (2, True), 'stiffness', None),
]


def chunk_sweep_sizes(mid_last, p0):
    """Spans of axis 0 that give 1, 2, 3 and 4 chunks, every remainder of the last chunk: for n chunks the sizes n * m + r,
    r = 0 .. n - 1, m the least chunk length (the first of them, minus one, stays a single chunk)."""
    P = p0 + 1
    m = (CHUNK_MIN_2D if len(mid_last) == 1 else CHUNK_MIN_3D) * P
    sizes = [2 * m - 1]
    for n in (2, 3, 4):
        sizes += [n * m + r for r in range(n)]
    return sizes


def chunk_axis0(mid_last, p0, n0):
    """(axis spec, interior geometry knots of axis 0, chunk length, chunks): a C^0 knot and a geometry span boundary inside the
    P - 1 warm-up spans before a chunk start -- the C^0 knot one span before the first chunk start, the geometry knot in the
    middle of the second span before the last chunk start."""
    axes = ((p0, n0, 1),) + tuple(mid_last)
    length, nch = geoa_chunks(axes)
    starts = [k * length for k in range(1, nch)]
    if not starts:
        return (p0, n0, 1), (0.5 + 0.5 / n0,), length, nch
    mult = [1] * (n0 - 1)
    mult[starts[0] - 2] = p0                            # interior knot k (1-based) sits at span boundary k: here starts[0] - 1
    gk = ((starts[-1] - 1.5) / n0,)
    return (p0, n0, tuple(mult)), gk, length, nch

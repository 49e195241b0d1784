"""The geometry-field kernels, k_grid_geo, k_coeff_affine and the single-launch 2D kernel k_single2d
(pyiga_amd/csrc/kern_basis.hip): the host decisions restated, and one small patch per instantiation, path and edge.

Plain helper module (not a conftest), the counterpart of ``tests/_geoa_cases.py``: ``tests/test_fields_coverage_cpu.py`` checks
that the restatement below and the source cannot drift apart and that the cases reach what they are there for,
``tests/test_fields_kernels_gpu.py`` runs every case on the device against the long-double model of ``tests/_fields_model.py``.

Restated: geo_fields_plan (line-wise or point-wise, lines per block, LDS bytes, the 64 KiB limit), single2d_supported,
single2d_plan (shape table, the 150 KiB limit, SINGLE2D_ROUND, SMALLEST_WANTED, geo_columns, the LDS image) and single2d_wanted
(sumfact.hip: SINGLE2D_MAX_BLOCKS, SINGLE2D_MAX_TILE).
"""
import collections
import os
import re

import numpy as np

import _bf3_cases as bc
import _entries_model as em
import _fields_model as fm

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'pyiga_amd', 'csrc')
KERN_BASIS_HIP = os.path.join(CSRC, 'kern_basis.hip')
SUMFACT_HIP = os.path.join(CSRC, 'sumfact.hip')

# ---- the restated constants (test_fields_coverage_cpu.py compares each with the source)
LINES_PASS = 256                 # geo_fields_plan: threads of a block of k_geo_fields_lines = points of one pass
LINES_SEARCH = 8                 # ... lines per block tried for a whole number of passes when a line is longer than one
LINES_LDS_LIMIT = 64 * 1024      # ... line coefficients above this: the point-wise kernel
POINTS_BLOCK = 128               # threads of a block of k_geo_fields, k_grid_geo, k_coeff_affine
MAX_COMP = 4                     # igx_internal.h
SHAPES = ((8, 8), (6, 6), (4, 4), (2, 4), (2, 2), (1, 2), (1, 1))      # single2d_plan
SMALLEST_WANTED = 3              # ... a small patch shrinks its tile down to SHAPES[3]
SINGLE2D_LDS_LIMIT = 150 * 1024
SINGLE2D_ROUND = 256
SINGLE2D_MAX_P = 6               # single2d_supported: P <= 6 on both axes
SINGLE2D_MAX_BLOCKS = 256        # sumfact.hip: single2d_wanted
SINGLE2D_MAX_TILE = 36

# instantiations: (kernel, template arguments)
INSTANTIATIONS = ([('k_geo_fields_lines', (d, nc, f)) for d, nc in ((2, 2), (2, 3), (3, 3), (3, 4)) for f in (False, True)] +
                  [('k_geo_fields', (d, f)) for d in (2, 3) for f in (False, True)] +
                  [('k_grid_geo', (2,)), ('k_grid_geo', (3,)), ('k_coeff_affine', (3,)),
                   ('k_single2d', ('MASS',)), ('k_single2d', ('STIFFNESS',))])


# ---------------------------------------------------------------------------------------------
# the source
def read_source(path=KERN_BASIS_HIP):
    with open(path) as f:
        return f.read()


def _body(src, start, end='\n}\n'):
    s = src[src.index(start):]
    return s[:s.index(end)]


def parse_source(src=None, sumfact=None):
    """Every constant and dispatch line restated above, read from kern_basis.hip and sumfact.hip."""
    src = src or read_source()
    sumfact = sumfact or read_source(SUMFACT_HIP)
    d = {}
    gp = _body(src, 'GeoFieldsPlan geo_fields_plan(')
    d['lines_cond'] = 'if (pt->geo_kind != IGX_GEO_JACOBIAN && !pt->boxed) {' in gp
    d['lines_LN'] = 'const int LN = (dim == 3) ? pt->dev.L2 : pt->dev.L1;' in gp
    d['lpb_pass'] = [int(v) for v in re.search(r'int LPB = std::max\(1, (\d+) / LN\);\s*if \(LN > (\d+)\)', gp).groups()]
    m = re.search(r'for \(int l = 1; l <= (\d+); \+\+l\)\s*if \(\(l \* LN\) % (\d+) == 0\) \{ LPB = l; break; \}', gp)
    d['lpb_search'], d['lpb_mod'] = int(m.group(1)), int(m.group(2))
    d['lds_formula'] = 'const size_t lds = (size_t)LPB * pt->gax[dim - 1].N * pt->ncomp * dim * sizeof(double);' in gp
    m = re.search(r'if \(lds <= (\d+) \* (\d+)\) \{ plan\.lines = true; plan\.LPB = LPB; plan\.lds = lds; \}', gp)
    d['lds_limit'] = int(m.group(1)) * int(m.group(2))
    lg = _body(src, 'int launch_geo_fields(')
    d['launch_uses_plan'] = 'const GeoFieldsPlan plan = geo_fields_plan(pt);' in lg and 'if (plan.lines) {' in lg
    d['lines_block'] = int(re.search(r'dim3 grid\(\(unsigned\)\(\(nlines \+ LPB - 1\) / LPB\)\), block\((\d+)\);', lg).group(1))
    d['lines_bounds'] = int(re.search(r'__launch_bounds__\((\d+)\) k_geo_fields_lines', src).group(1))
    inst = set()
    ml = lg[lg.index('#define LAUNCH_LINES('):lg.index('#undef LAUNCH_LINES')]
    forms = set(re.findall(r'k_geo_fields_lines<D_, NC_, (true|false)><<<', ml))
    cond = re.search(r'if \(dim == 2\) \{ if \(nurbs\) LAUNCH_LINES\((\d), (\d)\); else LAUNCH_LINES\((\d), (\d)\); \}\s*'
                     r'else \{ if \(nurbs\) LAUNCH_LINES\((\d), (\d)\); else LAUNCH_LINES\((\d), (\d)\); \}', ml)
    g = [int(v) for v in cond.groups()]
    d['lines_dispatch'] = {'2d': ((g[0], g[1]), (g[2], g[3])), '3d': ((g[4], g[5]), (g[6], g[7]))}      # (nurbs, B-spline)
    assert 'if (kind == IGX_FORM) k_geo_fields_lines<D_, NC_, true>' in ml and 'else k_geo_fields_lines<D_, NC_, false>' in ml
    for k in range(0, 8, 2):
        inst |= {('k_geo_fields_lines', (g[k], g[k + 1], f == 'true')) for f in forms}
    mp = lg[lg.index('#define LAUNCH_PTS('):lg.index('#undef LAUNCH_PTS')]
    assert 'k_geo_fields<D_, F_><<<grid, block, 0, st>>>' in mp
    pts = re.search(r'if \(dim == 2\) \{ if \(kind == IGX_FORM\) LAUNCH_PTS\((\d), (\w+)\); else LAUNCH_PTS\((\d), (\w+)\); \}\s*'
                    r'else \{ if \(kind == IGX_FORM\) LAUNCH_PTS\((\d), (\w+)\); else LAUNCH_PTS\((\d), (\w+)\); \}', mp).groups()
    d['pts_dispatch'] = [(int(pts[k]), pts[k + 1] == 'true') for k in range(0, 8, 2)]
    inst |= {('k_geo_fields', v) for v in d['pts_dispatch']}
    d['pts_block'] = int(re.search(r'dim3 grid\(\(unsigned\)\(\(total \+ (\d+)\) / (\d+)\)\), block\((\d+)\);\n#define LAUNCH_PTS', lg).group(3))
    inst |= {('k_grid_geo', (int(v),)) for v in re.findall(r'k_grid_geo<(\d)><<<', src)}
    inst |= {('k_coeff_affine', (int(v),)) for v in re.findall(r'k_coeff_affine<(\d)><<<', src)}
    inst |= {('k_single2d', (v,)) for v in re.findall(r'k_single2d<IGX_(\w+)><<<', src)}
    d['instantiations'] = inst
    d['grid_block'] = [int(v) for v in re.findall(r'dim3 grid\(\(unsigned\)\(\(total \+ 127\) / 128\)\), block\((\d+)\);', src)]
    # the single-launch kernel
    d['supported'] = re.search(r'bool single2d_supported\(const igx_patch \*pt, int kind\)\n\{\n    return (.*);\n\}', src).group(1)
    sp = _body(src, 'static bool single2d_plan(')
    d['shapes'] = tuple((int(a), int(b)) for a, b in re.findall(r'\{(\d+), (\d+)\}', re.search(r'static const int shapes\[\]\[2\] = \{(.*)\};', sp).group(1)))
    m = re.search(r'constexpr int NSHAPE = (\d+), SMALLEST_WANTED = (\d+);', sp)
    d['nshape'], d['smallest_wanted'] = int(m.group(1)), int(m.group(2))
    m = re.search(r'while \(k < NSHAPE && \(bytes = image\(k, A\)\) > (\d+) \* (\d+)\) \+\+k;', sp)
    d['s2d_lds_limit'] = int(m.group(1)) * int(m.group(2))
    d['shrink'] = 'while (k < SMALLEST_WANTED && blocks(k + 1) <= SINGLE2D_ROUND) ++k;' in sp
    d['round'] = int(re.search(r'constexpr long long SINGLE2D_ROUND = (\d+);', src).group(1))
    d['image'] = all(line in sp for line in (
        'S.NG0 = (S.R0 + A0.p) * q; S.WIN = (S.R1 + A1.p) * q;',
        'S.NCOL = spline ? geo_columns(S.R1) : 0;',
        'const size_t doubles = (size_t)NF * S.NG0 * S.WIN + (size_t)S.R0 * (2 * A0.P - 1) * NY * S.WIN + (size_t)S.NG0 * A0.P * 2 +',
        '(size_t)S.WIN * A1.P * 2 + (size_t)S.NG0 * S.NCOL * MAX_COMP * 2;',
        'const size_t ints = (size_t)3 * (S.R0 + 2 * A0.p) + 3 * S.R0 + (size_t)3 * (S.R1 + 2 * A1.p) + 3 * S.R1 + 16;',
        'return doubles * sizeof(double) + ints * sizeof(int);',
        'const int NF = kind == IGX_MASS ? 1 : 3, NY = kind == IGX_MASS ? 1 : 4, q = A0.q;',
        'const long long nr0 = whole_patch ? A0.N : std::max(pt->r0_hi - pt->r0_lo, 0);',
        'auto blocks = [&](int k) { return ((A1.N + shapes[k][1] - 1) / shapes[k][1]) * ((nr0 + shapes[k][0] - 1) / shapes[k][0]); };'))
    d['geo_columns'] = all(line in sp for line in (
        'for (int i1a = 0; i1a < A1.N; i1a += R1) {',
        'const double x0 = A1.nodes[(size_t)A1.mslo[i1a] * q], x1 = A1.nodes[(size_t)A1.mshi[i1b - 1] * q - 1];',
        'const long long between = std::upper_bound(g.kv.begin(), g.kv.end(), x1) - std::upper_bound(g.kv.begin(), g.kv.end(), x0);',
        'most = std::max(most, (int)between + g.P);',
        'return std::min(most, g.N);'))
    d['ncol_kernel'] = ('colb = A.gv.fa[1][g1b];' in src and 'ncol = A.gv.fa[1][g1b + w1 - 1] + A.gv.P[1] - colb;' in src and
                        'const int s1b = A1.mslo[i1a], g1b = s1b * q, w1 = A1.mshi[i1b - 1] * q - g1b;' in src)
    d['max_comp'] = int(re.search(r'constexpr int MAX_COMP = (\d+);', read_source(os.path.join(CSRC, 'igx_internal.h'))).group(1))
    d['query_uses_plan'] = 'if (!single2d_plan(pt, kind, A, bytes, whole_patch)) return IGX_OK;' in _body(src, 'int single2d_plan_query(')
    d['launch_uses_s2d_plan'] = 'if (!single2d_plan(pt, kind, A, bytes)) {' in _body(src, 'int launch_single2d(')
    d['sumfact_min_p'] = int(re.search(r'if \(pt->ax\[k\]\.p < (\d+) \|\| pt->ax\[k\]\.p > IGX_MAX_SF_DEGREE\) return 0;', sumfact).group(1))
    d['max_blocks'] = int(re.search(r'constexpr long long SINGLE2D_MAX_BLOCKS = (\d+);', sumfact).group(1))
    d['max_tile'] = int(re.search(r'constexpr int SINGLE2D_MAX_TILE = (\d+);', sumfact).group(1))
    w = _body(sumfact, 'bool single2d_wanted(')
    d['wanted'] = all(line in w for line in (
        'if (pt->knobs.final_sel || !single2d_supported(pt, kind)) return false;',
        'if (pt->knobs.path == 3) return true;',
        'if (pt->knobs.path != 0) return false;',
        'const long long nb = single2d_blocks(pt, kind, &rows, true);',
        'return nb >= 0 && nb <= SINGLE2D_MAX_BLOCKS && rows <= SINGLE2D_MAX_TILE;'))
    return d


SUPPORTED_TEXT = ('pt->dim == 2 && (kind == IGX_MASS || kind == IGX_STIFFNESS) && pt->ax[0].q == pt->ax[1].q && '
                  'pt->ax[0].P <= 6 && pt->ax[1].P <= 6')


# ---------------------------------------------------------------------------------------------
# geometry maps: seeded control nets, a perturbed box with x along the last axis (as tests/_geoa_cases.py builds them), with
# free knots on every axis
GeoSpec = collections.namedtuple('GeoSpec', 'axes nurbs seed')          # axes: ((degree, interior knots), ..) per grid axis


def geo_net(spec):
    """(axes [(knots, degree)], control net (.., dim), weights or None)."""
    dim = len(spec.axes)
    axes = [(np.concatenate([np.zeros(p + 1), np.asarray(k, dtype=float), np.ones(p + 1)]), p) for p, k in spec.axes]
    N = [len(k) - p - 1 for k, p in axes]
    grids = np.meshgrid(*(np.linspace(0., 1., n) for n in N), indexing='ij')
    rng = np.random.default_rng(spec.seed)
    if dim == 3:
        z, y, x = grids
        C = np.stack([x * (1.5 + 0.3 * y), y + 0.2 * np.sin(2. * z), z * (1. + 0.25 * x)], axis=-1)
    else:
        y, x = grids
        C = np.stack([x * (1.2 + 0.3 * y), y + 0.15 * np.sin(2. * x)], axis=-1)
    C = C + 0.02 * rng.standard_normal(C.shape) / max(N)
    w = 1.0 + 0.3 * rng.random(N) if spec.nurbs else None
    return axes, C, w


def model_map(spec):
    axes, C, w = geo_net(spec)
    if spec.nurbs:
        return fm.Map(axes, np.concatenate([C * w[..., None], w[..., None]], axis=-1), True)
    return fm.Map(axes, C, False)


def product_geo(iga, spec):
    axes, C, w = geo_net(spec)
    kvs = tuple(iga.bspline.KnotVector(k, p) for k, p in axes)
    if spec.nurbs:
        return iga.geometry.NurbsFunc(kvs, C.copy(), w.copy())
    return iga.bspline.BSplineFunc(kvs, C.copy())


# ---------------------------------------------------------------------------------------------
# the discretisation of a case on the host
class Space:
    """Knot vectors, Gauss rule and integer tables of a case (pyiga_amd.bspline is host-only Python)."""
    def __init__(self, axes, nqp=None, with_V=False):
        from pyiga_amd import bspline
        self.kvs = tuple(bspline.KnotVector(bc.axis_knots(a), a[0]) for a in axes)
        self.dim = len(axes)
        self.q = int(nqp) if nqp else max(a[0] for a in axes) + 1
        gw = np.polynomial.legendre.leggauss(self.q)[1]
        self.gauss = []
        for kv in self.kvs:
            mesh = np.asarray(kv.mesh, dtype=np.float64)
            h = 0.5 * (mesh[1:] - mesh[:-1])
            self.gauss.append((em.gauss_nodes(kv, self.q), (h[:, None] * gw[None, :]).ravel()))
        V = [None] * self.dim
        if with_V:
            V = [np.moveaxis(em.active_deriv_ld(kv, g[0], 1), (0, 1, 2), (2, 1, 0)) for kv, g in zip(self.kvs, self.gauss)]
        self.tables = [em.axis_table(kv, self.q, v) for kv, v in zip(self.kvs, V)]
        self.G = tuple(t.n * t.q for t in self.tables)

    def window(self, win):
        if win[0] == 'whole':
            return em.whole_window(self.tables)
        if win[0] == 'slab':
            return em.slab_window(self.tables, win[1])
        return em.box_window(self.tables, win[1])


# ---------------------------------------------------------------------------------------------
# launch_geo_fields, restated
def lines_per_block(LN):
    lpb = max(1, LINES_PASS // LN)
    if LN > LINES_PASS:
        for l in range(1, LINES_SEARCH + 1):
            if (l * LN) % LINES_PASS == 0:
                lpb = l
                break
    return lpb


def fields_plan(dim, LN, geo, boxed):
    """What DevicePatch.fields_plan returns.  geo: GeoSpec or 'jac'."""
    if geo == 'jac':
        return {'lines': False, 'lpb': 0, 'lds': 0, 'nc': 0}
    nc = dim + (1 if geo.nurbs else 0)
    p, k = geo.axes[dim - 1]
    lpb = lines_per_block(LN)
    lds = lpb * (len(k) + p + 1) * nc * dim * 8
    if boxed or lds > LINES_LDS_LIMIT:
        return {'lines': False, 'lpb': 0, 'lds': 0, 'nc': nc}
    return {'lines': True, 'lpb': lpb, 'lds': lds, 'nc': nc}


def fields_instantiation(dim, plan, form):
    if plan['lines']:
        return ('k_geo_fields_lines', (dim, plan['nc'], form))
    return ('k_geo_fields', (dim, form))


# coefficient data of a case: smooth seeded arrays on the resident grid
def coeff_array(shape, seed, lo=0.5):
    rng = np.random.default_rng(seed)
    a = rng.random(4)
    idx = np.meshgrid(*(np.linspace(0., 1., n) for n in shape), indexing='ij')
    return lo + 1.0 + sum(0.3 * np.sin((2. + a[k]) * x + a[-1]) for k, x in enumerate(idx))


# physical tables by name: the set of present (r, s); symmetric tables share the arrays of (r, s) and (s, r)
def table_present(name, dim):
    nj = dim + 1
    der = [(r, s) for r in range(1, nj) for s in range(1, nj)]
    return {'value_only': ([(0, 0)], True),
            'deriv_nonsym': (der, False),
            'mixed_sym': ([(0, 0)] + [(0, s) for s in range(1, nj)] + [(r, 0) for r in range(1, nj)] + der, True),
            'mixed_nonsym': ([(0, s) for s in range(1, nj)] + [(r, r) for r in range(1, nj)] + [(1, 2)], False)}[name]


def form_table(name, dim, shape, seed):
    """(4 x 4 nested list of arrays or None for DevicePatch.set_form, form_ab)."""
    present, sym = table_present(name, dim)
    T = [[None] * 4 for _ in range(4)]
    for r, s in present:
        key = (min(r, s), max(r, s)) if sym else (r, s)
        T[r][s] = coeff_array(shape, seed + 17 * key[0] + key[1], lo=0.0 if r != s else 1.0)
    return T, em.physical_form_ab(dim, set(present))


FCase = collections.namedtuple('FCase', 'id dim axes nqp geo kind win extra')


def _fc(tag, axes, nqp, geo, kind, win=('whole',), extra=None):
    return FCase(tag, len(axes), tuple(axes), nqp, geo, kind, win, extra)


def _g2(nurbs, seed, k1=(0.43,), p1=2, k0=(0.31,), p0=1):
    return GeoSpec(((p0, k0), (p1, k1)), nurbs, seed)


def _g3(nurbs, seed, k2=(0.61,), p2=1, k1=(0.37,), p1=2, k0=(0.45,), p0=1):
    return GeoSpec(((p0, k0), (p1, k1), (p2, k2)), nurbs, seed)


_MANY = tuple(np.round(np.linspace(0.07, 0.93, 9), 3))          # nine interior knots: eleven or more control points


def _build_field_cases():
    c = []
    a1 = lambda n: (1, n, 1)
    # 2D line kernel: every line length where the lines per block change, <2, 2> and <2, 3>, FORM false and true
    c.append(_fc('2d-LN2-mass-bsp', (a1(2), a1(1)), 2, _g2(False, 1), 'mass'))
    c.append(_fc('2d-LN2-stiff-nurbs-slab', (a1(3), a1(1)), 2, _g2(True, 2), 'stiffness', ('slab', (3, 4))))
    c.append(_fc('2d-LN256-stiff-nurbs', (a1(1), a1(64)), 4, _g2(True, 3), 'stiffness'))
    c.append(_fc('2d-LN257-mass-bsp', (a1(2), a1(257)), 1, _g2(False, 4), 'mass'))
    c.append(_fc('2d-LN258-stiff-nurbs', (a1(2), a1(129)), 2, _g2(True, 5), 'stiffness'))
    c.append(_fc('2d-LN259-form-nurbs', ((2, 1, 1), a1(37)), 7, _g2(True, 6), 'form_phys', extra='mixed_nonsym'))
    c.append(_fc('2d-LN260-stiff-bsp', (a1(1), a1(65)), 4, _g2(False, 7), 'stiffness'))
    c.append(_fc('2d-LN288-form-nurbs', (a1(3), a1(96)), 3, _g2(True, 8), 'form_phys', extra='mixed_sym'))
    c.append(_fc('2d-LN320-pform-bsp', (a1(1), a1(64)), 5, _g2(False, 9), 'form_par'))
    c.append(_fc('2d-LN384-stiff-bsp', (a1(1), a1(128)), 3, _g2(False, 10), 'stiffness'))
    c.append(_fc('2d-LN512-mass-nurbs', (a1(1), a1(128)), 4, _g2(True, 11), 'mass'))
    c.append(_fc('2d-LN576-stiff-nurbs-slab', (a1(3), a1(192)), 3, _g2(True, 12), 'stiffness', ('slab', (2, 4))))
    c.append(_fc('2d-LN576-form-bsp', (a1(3), a1(192)), 3, _g2(False, 13), 'form_phys', extra='deriv_nonsym'))
    c.append(_fc('2d-LN12-form-bsp-value', ((2, 3, 1), (2, 4, 1)), None, _g2(False, 14), 'form_phys', extra='value_only'))
    # 2D: line coefficients above 64 KiB at 128 lines per block -> the point-wise kernel on a spline geometry
    c.append(_fc('2d-fallback-stiff-nurbs', (a1(3), a1(1)), 2, _g2(True, 15, k1=_MANY), 'stiffness'))
    c.append(_fc('2d-fallback-form-nurbs-slab', (a1(3), a1(1)), 2, _g2(True, 16, k1=_MANY), 'form_phys', ('slab', (3, 4)), 'mixed_sym'))
    c.append(_fc('2d-nofallback-stiff-bsp', (a1(3), a1(1)), 2, _g2(False, 17, k1=_MANY), 'stiffness'))
    # 3D line kernel <3, 3>, <3, 4>: 42 lines per block against G1 = 4 lines per plane; every kind
    ax3 = ((1, 3, 1), (1, 2, 1), (1, 3, 1))
    c.append(_fc('3d-mass-bsp', ax3, None, _g3(False, 21), 'mass'))
    c.append(_fc('3d-stiff-nurbs-slab', ax3, None, _g3(True, 22), 'stiffness', ('slab', (2, 4))))
    c.append(_fc('3d-convdiff-sampled-bsp', ((2, 2, 1), (1, 3, 1), (2, 2, 1)), None, _g3(False, 23), 'convdiff', extra='sampled'))
    c.append(_fc('3d-convdiff-affine-nurbs-slab', ((2, 3, 1), (1, 3, 1), (2, 2, 1)), None, _g3(True, 24), 'convdiff', ('slab', (3, 5)), 'affine'))
    c.append(_fc('3d-form-sym-nurbs', ax3, None, _g3(True, 25), 'form_phys', extra='mixed_sym'))
    c.append(_fc('3d-form-nonsym-bsp-slab', ax3, None, _g3(False, 26), 'form_phys', ('slab', (0, 2)), 'mixed_nonsym'))
    c.append(_fc('3d-form-deriv-nurbs', ((1, 2, 1), (2, 2, 1), (1, 5, 1)), None, _g3(True, 27), 'form_phys', extra='deriv_nonsym'))
    c.append(_fc('3d-pform-bsp', ax3, None, _g3(False, 28), 'form_par'))
    # 3D: a last axis of two points (128 lines per block) under a map with ten control points along it -> point-wise
    c.append(_fc('3d-fallback-stiff-bsp', ((1, 2, 1), (1, 3, 1), (1, 1, 1)), None, _g3(False, 29, k2=_MANY[:8], p2=1), 'stiffness'))
    c.append(_fc('3d-fallback-form-nurbs', ((1, 2, 1), (1, 3, 1), (1, 1, 1)), None, _g3(True, 30, k2=_MANY[:8], p2=1), 'form_phys', extra='mixed_sym'))
    # point-wise kernel: span boxes (b1, b2 > 0), Jacobian arrays on the whole patch and on a slab
    ax2 = ((2, 4, 1), (2, 5, 1))
    c.append(_fc('2d-box-stiff-nurbs', ax2, None, _g2(True, 31), 'stiffness', ('box', ((1, 3), (2, 5)))))
    c.append(_fc('2d-box-form-bsp', ax2, None, _g2(False, 32), 'form_phys', ('box', ((0, 2), (1, 4))), 'mixed_nonsym'))
    ax3b = ((2, 3, 1), (1, 4, 1), (2, 3, 1))
    c.append(_fc('3d-box-mass-bsp', ax3b, None, _g3(False, 33), 'mass', ('box', ((1, 2), (1, 3), (1, 3)))))
    c.append(_fc('3d-box-convdiff-affine-nurbs', ax3b, None, _g3(True, 34), 'convdiff', ('box', ((0, 2), (2, 4), (1, 2))), 'affine'))
    c.append(_fc('3d-box-convdiff-sampled-bsp', ax3b, None, _g3(False, 35), 'convdiff', ('box', ((1, 3), (1, 4), (2, 3))), 'sampled'))
    c.append(_fc('3d-box-form-nurbs', ax3b, None, _g3(True, 36), 'form_phys', ('box', ((1, 3), (1, 2), (1, 3))), 'mixed_sym'))
    c.append(_fc('2d-jac-stiff', ax2, None, 'jac', 'stiffness'))
    c.append(_fc('2d-jac-mass-slab', ax2, None, 'jac', 'mass', ('slab', (3, 6))))
    c.append(_fc('2d-jac-form-slab', ax2, None, 'jac', 'form_phys', ('slab', (4, 6)), 'mixed_sym'))
    c.append(_fc('3d-jac-stiff', ax3b, None, 'jac', 'stiffness'))
    c.append(_fc('3d-jac-mass-slab', ax3b, None, 'jac', 'mass', ('slab', (3, 5))))
    c.append(_fc('3d-jac-form', ax3b, None, 'jac', 'form_phys', extra='deriv_nonsym'))
    c.append(_fc('3d-jac-pform-slab', ax3b, None, 'jac', 'form_par', ('slab', (4, 5))))
    return c


FIELD_CASES = _build_field_cases()
JAC_SEED = 90                      # the map whose float64 Jacobian a Jacobian-array case is given


def jac_spec(dim):
    return _g2(True, JAC_SEED) if dim == 2 else _g3(True, JAC_SEED)


def field_case_plan(case):
    sp = Space(case.axes, case.nqp)
    w = sp.window(case.win)
    LN = w.L2 if case.dim == 3 else w.L1
    plan = fields_plan(case.dim, LN, case.geo, case.win[0] == 'box')
    return sp, w, plan


def field_inputs(case, sp=None, window=None):
    """Everything the model and the device are given: dict(jac_full, jac, coeff_full, coeff, form, table, pterms, resident)."""
    sp = sp or Space(case.axes, case.nqp)
    w = window or sp.window(case.win)
    box = case.win[0] == 'box'
    shape_w = (w.G0, w.L1, w.L2)[:case.dim]
    resident = shape_w if box else sp.G                     # the grid the coefficient arrays are given on
    cut = (lambda a: a) if box else (lambda a: a[w.g0:w.g0 + w.G0])
    out = dict(resident=resident, jac=None, jac_full=None, coeff=None, coeff_full=None, form=None, table=None, pterms=None)
    if case.geo == 'jac':
        # (for a box the library takes the array of the box alone: DevicePatch(jacobian=..., bbox=...))
        lo = [(w.g0, w.G0), (w.b1, w.L1), (w.b2, w.L2)][:case.dim] if box else [(0, g) for g in sp.G]
        nodes = [sp.gauss[a][0][l:l + n] for a, (l, n) in enumerate(lo)]
        J = fm.eval_map(model_map(jac_spec(case.dim)), nodes, np.float64)[1]
        out['jac_full'], out['jac'] = J, cut(J)
    seed = 1000 + sum(ord(ch) for ch in case.id)
    if case.kind == 'convdiff':
        if case.extra == 'affine':
            out['coeff'] = out['coeff_full'] = ('affine', (1.5, 0.25, -0.5, 0.75))
        else:
            out['coeff_full'] = coeff_array(resident, seed)
            out['coeff'] = cut(out['coeff_full'])
    if case.kind == 'form_phys':
        T, ab = form_table(case.extra, case.dim, resident, seed)
        out['table'] = T
        nj = case.dim + 1
        out['form'] = ('phys', [[None if T[r][s] is None else cut(T[r][s]) for s in range(nj)] for r in range(nj)], ab)
    if case.kind == 'form_par':
        full = (1 << case.dim) - 1
        masks = [(0, 0), (full, 1), (1, full), (2, 2)]
        out['pterms'] = [(mv, mu, coeff_array(resident, seed + k)) for k, (mv, mu) in enumerate(masks)]
        out['form'] = ('par', [cut(t[2]) for t in out['pterms']])
    return out


def model_fields(case, dtype, sp=None, window=None, inp=None, mutate=None, lpb=1):
    sp = sp or Space(case.axes, case.nqp)
    w = window or sp.window(case.win)
    inp = inp or field_inputs(case, sp, w)
    kind = 'form' if case.kind.startswith('form') else case.kind
    geo = None if case.geo == 'jac' else model_map(case.geo)
    return fm.fields(kind, case.dim, w, sp.gauss, dtype, geo=geo, jac=inp['jac'], coeff=inp['coeff'], form=inp['form'], mutate=mutate, lpb=lpb)


def field_mutants(case, plan):
    """The mutants of _fields_model that apply to a case."""
    m = ['drop_point']
    q = case.nqp or max(a[0] for a in case.axes) + 1
    if q >= 3:                                              # (one or two points per span of a uniform mesh: equal weights)
        m.append('gw_neighbour')
    if case.geo != 'jac':
        m.append('colb')
        if case.geo.nurbs:
            m.append('no_wprime')
        if case.win[0] == 'slab':
            m.append('slab_plane')
    if case.win[0] == 'box' and case.win[1][1][0] > 0:
        m.append('no_b1')
    if case.kind == 'stiffness' and case.dim == 2:
        m.append('swap_f12')
    if plan['lines'] and plan['lpb'] > 1:
        m.append('drop_line')
    if case.kind == 'form_par':                             # (GW * coefficient: the geometry does not enter)
        m = [x for x in m if x not in ('colb', 'no_wprime')]
    return m


# ---------------------------------------------------------------------------------------------
# k_grid_geo: (id, GeoSpec of the map's axes, components, nodes per axis)
GCase = collections.namedtuple('GCase', 'id spec ncomp grid')


def grid_map(case):
    """fm.Map with `ncomp` components: the geometry net, cut or extended by seeded components."""
    axes, C, w = geo_net(case.spec)
    rng = np.random.default_rng(case.spec.seed + 500)
    extra = 0.5 + rng.random(C.shape[:-1] + (MAX_COMP,))
    C = np.concatenate([C, extra], axis=-1)[..., :case.ncomp]
    if case.spec.nurbs:
        return fm.Map(axes, np.concatenate([C * w[..., None], w[..., None]], axis=-1), True)
    return fm.Map(axes, C, False)


def _build_grid_cases():
    c = []
    u7 = np.array([0., 0.1, 0.31, 0.31, 0.5, 0.77, 1.])             # both end points, a knot (0.31), a repeated node
    g2k = GeoSpec(((1, (0.31,)), (2, (0.43, 0.43, 0.6))), False, 41)   # a repeated interior knot
    for ncomp in range(1, MAX_COMP + 1):
        c.append(GCase('2d-bsp-nc%d' % ncomp, g2k, ncomp, (u7, np.array([0., 0.43, 0.43, 0.5, 0.6, 1.]))))
    for ncomp in range(1, MAX_COMP):
        c.append(GCase('2d-nurbs-nc%d' % ncomp, g2k._replace(nurbs=True, seed=42), ncomp, (np.array([0.2, 1.]), u7)))
    g3k = GeoSpec(((1, (0.45,)), (2, (0.37,)), (2, (0.5, 0.5))), False, 43)
    u3 = np.array([0., 0.5, 1.])
    for ncomp in (1, 3, 4):
        c.append(GCase('3d-bsp-nc%d' % ncomp, g3k, ncomp, (u3, np.array([0.37, 0.9]), np.array([0., 0.25, 0.5, 0.5, 1.]))))
    for ncomp in (1, 2, 3):
        c.append(GCase('3d-nurbs-nc%d' % ncomp, g3k._replace(nurbs=True, seed=44), ncomp, (np.array([1.]), u3, np.array([0., 0.5, 0.75, 1.]))))
    # totals of 127, 128 and 129 points (one block of 128 threads, its edge, one point into the second)
    lin = lambda n: np.linspace(0., 1., n)
    c.append(GCase('2d-total127', g2k._replace(nurbs=True, seed=45), 2, (lin(1), lin(127))))
    c.append(GCase('2d-total128', g2k, 2, (lin(8), lin(16))))
    c.append(GCase('2d-total129', g2k, 2, (lin(3), lin(43))))
    c.append(GCase('3d-total127', g3k, 3, (lin(1), lin(127), lin(1))))
    c.append(GCase('3d-total128', g3k._replace(nurbs=True, seed=46), 3, (lin(4), lin(4), lin(8))))
    c.append(GCase('3d-total129', g3k, 3, (lin(3), lin(1), lin(43))))
    return c


GRID_CASES = _build_grid_cases()


# ---------------------------------------------------------------------------------------------
# k_single2d: the host plan, restated
def _findspan_geo(knots, p, u):
    return em.findspan(np.asarray(knots, dtype=np.float64), p, u)


def geo_columns(sp, geo, R1):
    """single2d_plan's bound on the geometry control columns of axis 1 under the Gauss window of a tile."""
    t, nodes = sp.tables[1], sp.gauss[1][0]
    p, k = geo.axes[1]
    gk = np.concatenate([np.zeros(p + 1), np.asarray(k, dtype=float), np.ones(p + 1)])
    most = 0
    for i1a in range(0, t.N, R1):
        i1b = min(i1a + R1, t.N)
        x0, x1 = nodes[t.mslo[i1a] * t.q], nodes[t.mshi[i1b - 1] * t.q - 1]
        between = int(np.searchsorted(gk, x1, side='right') - np.searchsorted(gk, x0, side='right'))
        most = max(most, between + p + 1)
    return min(most, len(gk) - p - 1)


def kernel_ncol(sp, geo, R1):
    """The largest ncol any tile of k_single2d computes: fa[1][g1b + w1 - 1] + P - colb."""
    t, nodes = sp.tables[1], sp.gauss[1][0]
    p, k = geo.axes[1]
    gk = np.concatenate([np.zeros(p + 1), np.asarray(k, dtype=float), np.ones(p + 1)])
    most = 0
    for i1a in range(0, t.N, R1):
        i1b = min(i1a + R1, t.N)
        g1b = t.mslo[i1a] * t.q
        w1 = t.mshi[i1b - 1] * t.q - g1b
        colb = _findspan_geo(gk, p, nodes[g1b]) - p
        most = max(most, _findspan_geo(gk, p, nodes[g1b + w1 - 1]) - p + p + 1 - colb)
    return most


def single2d_supported(sp, kind):
    return sp.dim == 2 and kind in ('mass', 'stiffness') and all(t.p + 1 <= SINGLE2D_MAX_P for t in sp.tables)


def _image(sp, geo, kind, k):
    t0, t1 = sp.tables
    NF, NY, q = (1, 1, sp.q) if kind == 'mass' else (3, 4, sp.q)
    R0, R1 = SHAPES[k]
    NG0, WIN = (R0 + t0.p) * q, (R1 + t1.p) * q
    NCOL = 0 if geo == 'jac' else geo_columns(sp, geo, R1)
    doubles = NF * NG0 * WIN + R0 * (2 * (t0.p + 1) - 1) * NY * WIN + NG0 * (t0.p + 1) * 2 + WIN * (t1.p + 1) * 2 + NG0 * NCOL * MAX_COMP * 2
    ints = 3 * (R0 + 2 * t0.p) + 3 * R0 + 3 * (R1 + 2 * t1.p) + 3 * R1 + 16
    return dict(R0=R0, R1=R1, NG0=NG0, WIN=WIN, NCOL=NCOL, lds=doubles * 8 + ints * 4)


def single2d_plan(sp, geo, kind, path='default', row0=None, whole_patch=False):
    """What DevicePatch.single2d_plan returns for a patch of the rows row0 (None: whole)."""
    zero = dict(supported=False, wanted=False, R0=0, R1=0, NG0=0, WIN=0, NCOL=0, lds=0, blocks=0)
    if not single2d_supported(sp, kind):
        return zero
    t0, t1 = sp.tables

    def plan(nr0):
        blocks = lambda k: -(-t1.N // SHAPES[k][1]) * -(-nr0 // SHAPES[k][0])
        k = 0
        while k < len(SHAPES) and _image(sp, geo, kind, k)['lds'] > SINGLE2D_LDS_LIMIT:
            k += 1
        if k == len(SHAPES):
            return None
        while k < SMALLEST_WANTED and blocks(k + 1) <= SINGLE2D_ROUND:
            k += 1
        return dict(_image(sp, geo, kind, k), blocks=blocks(k))
    whole = plan(t0.N)
    if path == 'single':
        wanted = True
    else:
        wanted = whole is not None and whole['blocks'] <= SINGLE2D_MAX_BLOCKS and whole['R0'] * whole['R1'] <= SINGLE2D_MAX_TILE
    mine = whole if (whole_patch or row0 is None) else plan(row0[1] - row0[0])
    if mine is None:
        return dict(zero, supported=True, wanted=wanted)
    return dict(mine, supported=True, wanted=wanted)


SCase = collections.namedtuple('SCase', 'id axes nqp geo path slabs')
_FINE = ((2, (0.3, 0.3, 0.66)), (2, (0.2, 0.2, 0.37, 0.5, 0.81)))     # finer than the spaces below, not nested, a repeated
                                                                       # interior knot per axis, 0.5 on a space knot

S2D_CASES = [
    # small patches (2 x 4 rows): the edges of the basis and of the geometry
    SCase('p23-bsp', ((2, 3, 1), (3, 4, 1)), None, _g2(False, 51), 'default', ((1, 4), (0, 1))),
    SCase('p12-nurbs', ((1, 3, 1), (2, 3, 1)), None, _g2(True, 52), 'default', ((1, 3),)),
    SCase('p31-bsp', ((3, 2, 1), (1, 5, 1)), None, _g2(False, 53), 'default', ((3, 5),)),
    # degree 0 on one axis: the sum-factorised assembly refuses the patch (sumfact_supported: 1 <= p), so k_single2d is never
    # reached -- the device test asserts the refusal
    SCase('p02-nurbs', ((0, 3, 1), (2, 3, 1)), None, _g2(True, 66), 'default', ()),
    SCase('p20-bsp', ((2, 3, 1), (0, 5, 1)), None, _g2(False, 67), 'default', ()),
    SCase('p22-q5-jac', ((2, 3, 1), (2, 4, 1)), 5, 'jac', 'default', ((1, 4),)),
    SCase('mult-axis0-nurbs', ((3, 4, (2, 1, 3)), (2, 3, 1)), None, _g2(True, 54), 'default', ((3, 8),)),
    SCase('mult-axis1-bsp', ((2, 3, 1), (3, 4, (3, 2, 1))), None, _g2(False, 55), 'default', ((1, 2),)),
    SCase('one-tile', ((1, 1, 1), (1, 2, 1)), None, _g2(True, 56), 'default', ()),
    SCase('fine-geo-nurbs', ((2, 2, 1), (2, 4, 1)), None, GeoSpec(_FINE, True, 57), 'default', ((1, 3),)),
    SCase('fine-geo-bsp-q4', ((1, 3, 1), (2, 6, 1)), 4, GeoSpec(_FINE, False, 58), 'default', ((1, 4),)),
    SCase('p22-single', ((2, 3, 1), (2, 3, 1)), None, _g2(True, 59), 'single', ((2, 5),)),
    # degree 5: the LDS limit decides (stiffness: 2 x 2, 1 x 2 and 1 x 1 rows)
    SCase('p5-q8', ((5, 2, 1), (5, 2, 1)), 8, _g2(True, 60), 'default', ((1, 4),)),
    SCase('p5-q9', ((5, 2, 1), (5, 2, 1)), 9, GeoSpec(_FINE, False, 61), 'default', ((3, 4),)),
    SCase('p5-q11-jac', ((5, 1, 1), (5, 2, 1)), 11, 'jac', 'default', ((2, 5),)),
    SCase('p54-q11-nurbs', ((5, 2, (3,)), (4, 2, 1)), 11, _g2(True, 62), 'default', ()),
    # long thin patches: more than one round of the smaller tiles (4 x 4 and 6 x 6 rows by default, 8 x 8 on request)
    SCase('long-4x4', ((1, 5, 1), (1, 398, 1)), None, _g2(False, 63, k1=(0.1234, 0.5, 0.87)), 'default', ((1, 6),)),
    SCase('long-6x6', ((2, 8, 1), (1, 512, 1)), None, _g2(True, 64), 'default', ((1, 10),)),
    SCase('long-8x8', ((1, 6, 1), (2, 768, 1)), None, _g2(False, 65, k1=(0.2, 0.2, 0.61)), 'single', ((3, 7),)),
    SCase('long-8x8-jac', ((1, 8, 1), (1, 770, 1)), None, 'jac', 'single', ((1, 9),)),
]
S2D_KINDS = ('mass', 'stiffness')
SUMFACT_MIN_P = 1                  # sumfact.hip: sumfact_supported


def s2d_refused(case):
    """igx_assemble(algo = sumfact) refuses the patch before any plan is made."""
    return min(a[0] for a in case.axes) < SUMFACT_MIN_P


def s2d_jac(case, sp):
    """The Jacobian array of a Jacobian-array case: the float64 Jacobian of a NURBS map on the whole Gauss grid."""
    return fm.eval_map(model_map(jac_spec(2)), [g[0] for g in sp.gauss], np.float64)[1]


def reachable_shapes(max_n=40):
    """Tile shapes some admissible patch reaches, by enumeration over degrees, nqp and sizes (a Jacobian array: NCOL = 0, the
    smallest LDS image).  Returns {shape index: (kind, p0, p1, q, N0, N1, path)} of the first patch found."""
    found = {}
    for kind in S2D_KINDS:
        NF, NY = (1, 1) if kind == 'mass' else (3, 4)
        for p0 in range(0, SINGLE2D_MAX_P):
            for p1 in range(0, SINGLE2D_MAX_P):
                for q in range(1, 17):
                    fits = None
                    for k, (R0, R1) in enumerate(SHAPES):
                        NG0, WIN = (R0 + p0) * q, (R1 + p1) * q
                        doubles = NF * NG0 * WIN + R0 * (2 * p0 + 1) * NY * WIN + NG0 * (p0 + 1) * 2 + WIN * (p1 + 1) * 2
                        ints = 3 * (R0 + 2 * p0) + 3 * R0 + 3 * (R1 + 2 * p1) + 3 * R1 + 16
                        if doubles * 8 + ints * 4 <= SINGLE2D_LDS_LIMIT:
                            fits = k
                            break
                    if fits is None:
                        continue
                    for N0, N1 in ((max(p0 + 1, 2), max(p1 + 1, 2)), (max(p0 + 1, 3), 513), (max(p0 + 1, 5), 513), (max(p0 + 1, 7), 770), (8, 2000)):
                        blocks = lambda k: -(-N1 // SHAPES[k][1]) * -(-N0 // SHAPES[k][0])
                        k = fits
                        while k < SMALLEST_WANTED and blocks(k + 1) <= SINGLE2D_ROUND:
                            k += 1
                        default = blocks(k) <= SINGLE2D_MAX_BLOCKS and SHAPES[k][0] * SHAPES[k][1] <= SINGLE2D_MAX_TILE
                        found.setdefault(k, (kind, p0, p1, q, N0, N1, 'default' if default else 'single'))
    return found

"""The cases that run every path of the load-vector kernels (pyiga_amd/csrc/kern_vector.hip, the generated copy of k_lv12 in
pyiga_amd/csrc/rtc.hip) and the launch shapes of the spline evaluation (pyiga_amd/csrc/kern_spline.hip), and what decides them.

A plain helper module (no GPU needed to import it, no library load): tests/test_lv_coverage_cpu.py checks on the host that the
tables below reach what they claim and that the restated dispatch is the one in the source, tests/test_lv_kernels_gpu.py and
tests/test_spline_eval_gpu.py run them.

- ``axis_tables(kv, q)``: the per-axis tables of AxisDev the dispatch looks at (P, N, n, q, G, fa, mslo, mshi).
- ``lv12_refusals`` / ``lv12_shape``: the restatement of kern_vector.hip's lv12_shape: the reasons why k_lv12 does not serve a
  patch, and for one it serves the chunks of the mid axis (``clen`` spans each, ``nch`` of them: a short last chunk joins its
  neighbour) and the LDS bytes (``lds12``).
- ``last_axis_fast`` / ``expected_path``: which kernel contracts the last axis: 'lv12' (k_lv12 + axis 0: two launches),
  'last128' / 'last256' (k_contract_last with 128 / 256 threads, LPB lines per block: 16 in 3D, 4 in 2D), 'generic'
  (k_contract_axis).
- ``npass = ceil(N2 / 64)`` (the NPASS template argument is max(2, npass)), ``npc = ceil(G2 / 128)`` (16-byte pieces per lane).
- ``spline12_waves`` / ``spline_lpw``: the launch shape of k_spline12.

The case tables: ``INSTANCE_CASES`` (one line per reachable (P, NPASS) of k_lv12 and the C4 line), ``CHUNK_CASES`` (several
chunks of the mid axis, repeated knots across chunk boundaries), ``FALLBACK_CASES`` (one per refusal reason, both block sizes of
k_contract_last with a ragged last block, the generic kernel, 2D), ``SPLINE_CASES``.
"""
import os
import re
from typing import NamedTuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERN_VECTOR_HIP = os.path.join(ROOT, 'pyiga_amd', 'csrc', 'kern_vector.hip')
KERN_SPLINE_HIP = os.path.join(ROOT, 'pyiga_amd', 'csrc', 'kern_spline.hip')
RTC_HIP = os.path.join(ROOT, 'pyiga_amd', 'csrc', 'rtc.hip')

# constants of kern_vector.hip / kern_spline.hip (test_lv_coverage_cpu.py reads them from the source and compares)
VEC_MAXSUP = 36
LV_MAXPASS = 4
LV_WAVES = 4
LV_MAXPC = 5
LV_MAX_G2 = 640
LV_LDS_LIMIT = 64 * 1024
LV_UNITS = 8192                  # waves the chunk rule aims at
LV_MIN_CHUNK = 8                 # spans (or P, if that is more)
LAST_LDS_LIMIT = 48 * 1024
LAST_TB_SPLIT = 128              # N > 128: 256 threads
LPB = {3: 16, 2: 4}
SP_MAXWAVES = 4
SP_LDS_LIMIT = 64 * 1024
SP_MAX_LPW = 8
SP_LINES_PER_LPW = 16384
LV12_PS = (2, 3, 4, 5, 6)
LV12_NPASSES = (2, 3, 4)

# the refusal condition of lv12_shape, conjunct by conjunct (whitespace-normalised source text -> reason)
LV12_CONJUNCTS = {
    'a2.P >= 2': 'P', 'a2.P <= 6': 'P', 'a1.P == a2.P': 'degrees', 'PQ <= VEC_MAXSUP': 'PQ>36',
    'a2.N <= 64 * LV_MAXPASS': 'N2>256', 'a2.G % 2 == 0': 'oddG2', 'a2.G <= 640': 'G2>640', 'lds12 <= 64 * 1024': 'lds',
    'a1.n >= a1.P': 'shortmid',
}
# the chunk rule of lv12_shape, statement by statement (whitespace-normalised)
LV12_CHUNK_RULE = (
    'const long long G0 = pd.ax[0].G;',
    'int nch = (int)std::min<long long>(std::max<long long>(1, (8192 + G0 - 1) / std::max<long long>(G0, 1)), std::max(1, a1.n / std::max(a1.P, 8)));',
    'int clen = (a1.n + nch - 1) / nch;',
    'clen = std::max(clen, a1.P);',
    'nch = (a1.n + clen - 1) / clen;',
    'if (nch > 1 && a1.n - (nch - 1) * clen < a1.P) { --nch; }',
)
LV12_LDS_EXPR = 'const size_t lds12 = ((size_t)((PQ * a2.N + 1) & ~1) + LV_WAVES * (size_t)((a2.G + 1) & ~1)) * sizeof(double);'
LAST_AXIS_FAST_EXPR = 'return ax.N <= 256 && ax.P * ax.q <= VEC_MAXSUP && (size_t)2 * ax.G * sizeof(double) <= 48 * 1024;'
REASONS = ('2d', 'degrees', 'oddG2', 'G2>640', 'N2>256', 'PQ>36', 'lds', 'shortmid')


# ---------------------------------------------------------------------------------------------
# knot vectors and axis tables
def make_kv(spec):
    """(p, n, mult) or (p, n, mult, ((mesh index, extra copies), ..)): make_knots, then single interior knots repeated."""
    from pyiga_amd import bspline
    p, n, mult = spec[:3]
    kv = bspline.make_knots(p, 0.0, 1.0, n, mult=mult)
    if len(spec) > 3 and spec[3]:
        extra = np.concatenate([np.repeat(kv.mesh[m], c) for m, c in spec[3]])
        kv = bspline.KnotVector(np.sort(np.concatenate((kv.kv, extra))), p)
    return kv


class Axis(NamedTuple):
    p: int
    P: int
    N: int
    n: int
    q: int
    G: int
    fa: np.ndarray         # first active dof of every span
    mslo: np.ndarray       # first span of every dof's support
    mshi: np.ndarray       # one past its last span


def axis_tables(kv, q):
    p = int(kv.p)
    fa = np.asarray(kv.mesh_span_indices(), dtype=np.int64) - p
    ms = np.asarray(kv.mesh_support_idx_all(), dtype=np.int64)
    n = int(kv.numspans)
    return Axis(p, p + 1, int(kv.numdofs), n, int(q), n * int(q), fa, ms[:, 0], ms[:, 1])


def synthetic_axis(p, n, mult, q):
    """The tables of make_knots(p, 0, 1, n, mult) without the knot vector (the exhaustive window test builds thousands)."""
    fa = np.arange(n, dtype=np.int64) * mult
    N = p + 1 + (n - 1) * mult
    i = np.arange(N, dtype=np.int64)
    mslo = np.searchsorted(fa + p, i, side='left')           # first span whose active range fa .. fa + p reaches i
    mshi = np.searchsorted(fa, i, side='right')              # one past the last span with fa <= i
    return Axis(p, p + 1, N, n, int(q), n * int(q), fa, mslo.astype(np.int64), mshi.astype(np.int64))


# ---------------------------------------------------------------------------------------------
# the dispatch of launch_load_vector, restated
def lds12(a2):
    PQ = a2.P * a2.q
    return (((PQ * a2.N + 1) & ~1) + LV_WAVES * ((a2.G + 1) & ~1)) * 8


def lv12_refusals(axes):
    """The reasons why lv12_shape refuses the patch (empty: k_lv12 serves it)."""
    if len(axes) != 3:
        return {'2d'}
    a1, a2 = axes[1], axes[2]
    out = set()
    if not 2 <= a2.P <= 6:
        out.add('P')
    if a1.P != a2.P:
        out.add('degrees')
    if a2.P * a2.q > VEC_MAXSUP:
        out.add('PQ>36')
    if a2.N > 64 * LV_MAXPASS:
        out.add('N2>256')
    if a2.G % 2:
        out.add('oddG2')
    if a2.G > LV_MAX_G2:
        out.add('G2>640')
    if lds12(a2) > LV_LDS_LIMIT:
        out.add('lds')
    if a1.n < a1.P:
        out.add('shortmid')
    return out


def chunk_rule(n1, P, G0, merge=True):
    """(clen, nch) of the mid axis: enough waves for the chip, never shorter than P spans; the short last chunk joins its
    neighbour (`merge`: the switch exists for the mutation test of the window model)."""
    nch = min(max(1, (LV_UNITS + G0 - 1) // max(G0, 1)), max(1, n1 // max(P, LV_MIN_CHUNK)))
    clen = (n1 + nch - 1) // nch
    clen = max(clen, P)
    nch = (n1 + clen - 1) // clen
    if merge and nch > 1 and n1 - (nch - 1) * clen < P:
        nch -= 1
    return clen, nch


def lv12_shape(axes):
    """None where k_lv12 does not serve the patch, else (clen, nch, lds12).  The chunks come from the Gauss planes of the whole
    axis 0, also for a row slab: a slab repeats its rows of the whole vector bit for bit only with the same chunks."""
    if lv12_refusals(axes):
        return None
    a0, a1, a2 = axes
    clen, nch = chunk_rule(a1.n, a1.P, a0.G)
    return clen, nch, lds12(a2)


def last_axis_fast(ax):
    return ax.N <= 256 and ax.P * ax.q <= VEC_MAXSUP and 2 * ax.G * 8 <= LAST_LDS_LIMIT


def expected_path(axes):
    if not lv12_refusals(axes):
        return 'lv12'
    last = axes[-1]
    if last_axis_fast(last):
        return 'last256' if last.N > LAST_TB_SPLIT else 'last128'
    return 'generic'


def npass_of(N2):
    return (N2 + 63) // 64


def npc_of(G2):
    return (G2 // 2 + 63) >> 6


def last_lines(axes):
    """Grid lines k_contract_last walks (blocks of LPB of them)."""
    return int(np.prod([a.G for a in axes[:-1]]))


# ---------------------------------------------------------------------------------------------
# the launch shape of k_spline12, restated
def spline12_waves(dim, grad, Nlast):
    per_wave = (dim if grad else 1) * Nlast * 8
    w = SP_MAXWAVES
    while w >= 1:
        if w * per_wave <= SP_LDS_LIMIT:
            return w
        w >>= 1
    return 0


def spline_lpw(nlines):
    return min(SP_MAX_LPW, max(1, nlines // SP_LINES_PER_LPW))


# ---------------------------------------------------------------------------------------------
# parsing the sources
def read(path):
    with open(path) as f:
        return f.read()


def _norm(text):
    return re.sub(r'\s+', ' ', text)


def _function_body(src, signature):
    """Text of the function whose definition starts with `signature` (up to its closing brace at column 0)."""
    i = src.index(signature)
    j = src.index('\n}\n', i)
    return src[i:j]


def parse_constants(vec_src, spl_src):
    out = {}
    for name, src in (('VEC_MAXSUP', vec_src), ('LV_MAXPASS', vec_src), ('LV_WAVES', vec_src), ('SP_MAXWAVES', spl_src)):
        m = re.search(r'constexpr int %s = (\d+);' % name, src)
        out[name] = int(m.group(1)) if m else None
    return out


def parse_lv12_conjuncts(vec_src):
    """The conjuncts of `if (!( ... )) return false;` in lv12_shape, whitespace-normalised."""
    body = _norm(_function_body(vec_src, 'bool lv12_shape('))
    m = re.search(r'if \(!\((.*?)\)\) return false;', body)
    return [c.strip() for c in m.group(1).split('&&')]


def parse_lv12_statements(vec_src):
    """The statements of lv12_shape (whitespace-normalised, comments removed)."""
    body = _function_body(vec_src, 'bool lv12_shape(')
    body = re.sub(r'//[^\n]*', '', body)
    return _norm(body)


def parse_last_axis_fast(vec_src):
    body = _norm(_function_body(vec_src, 'int launch_load_vector('))
    m = re.search(r'auto last_axis_fast = \[\]\(const AxisDev &ax\) \{ (.*?) \};', body)
    return m.group(1) if m else None


def parse_tb_lpb(vec_src):
    """[(threshold of N, LPB)] of the two k_contract_last launches (3D first, then 2D)."""
    body = _function_body(vec_src, 'int launch_load_vector(')
    return [(int(a), int(b)) for a, b in re.findall(r'const int tb = a\d\.N > (\d+) \? 256 : 128, LPB = (\d+);', body)]


def parse_lv12_switch(vec_src):
    """(labels of the LV12(P) switch, NPASS values of the three branches, MAXPC values, the npass expression)."""
    body = _function_body(vec_src, 'int launch_load_vector(')
    m = re.search(r'switch \(a2\.P\) \{(.*?)\}', body)
    labels = [int(x) for x in re.findall(r'LV12\((\d+)\);', m.group(1))] if m else None
    m = re.search(r'#define LV12P\(W_, PP, PC\) do \{ if \(npass <= 2\) LV12K\(W_, PP, PC, (\d+)\); else if \(npass == 3\) LV12K\(W_, PP, PC, (\d+)\); '
                  r'else LV12K\(W_, PP, PC, (\d+)\); \} while \(0\)', body)
    npasses = tuple(int(x) for x in m.groups()) if m else None
    m = re.search(r'if \(d_W\) LV12P\(true, PP, (\d+)\); else LV12P\(false, PP, (\d+)\);', body)
    maxpc = tuple(int(x) for x in m.groups()) if m else None
    m = re.search(r'const int npass = ([^;]*);', body)
    return labels, npasses, maxpc, m.group(1) if m else None


def parse_lv12_kernel_npc(src):
    """The npc expression of k_lv12 (and of its generated copy)."""
    return re.findall(r'const int npc = ([^;]*);', src)


def parse_rtc(rtc_src):
    """What selects the generated copy: the constexpr line of the body and the npass of launch_lv12_expr / rtc_compile_lv12."""
    i = rtc_src.index('static const char *const RTC_LV12_BODY')
    body = rtc_src[i:rtc_src.index(')IGX";', i)]
    m = re.search(r'constexpr int P = (\w+), MAXPC = (\d+), NPASS = (\w+), LV_WAVES = (\d+);', body)
    launch = _function_body(rtc_src, 'int launch_lv12_expr(')
    n = re.search(r'const int npass = ([^;]*);', launch)
    compile_ = _function_body(rtc_src, 'int rtc_compile_lv12(')
    r = re.search(r'P < (\d+) \|\| P > (\d+) \|\| npass < (\d+) \|\| npass > (\d+)', compile_)
    return (m.groups() if m else None, n.group(1) if n else None, tuple(int(x) for x in r.groups()) if r else None, body)


def kernel_window_text(src, start, stop):
    """The text of a k_lv12 copy between two markers, whitespace-normalised with the lv_cdp aliases of kern_vector.hip spelled
    as the tables they alias: what the two copies must share."""
    i = src.index(start)
    j = src.index(stop, i)
    t = _norm(src[i:j])
    return t.replace('fa1[', 'a1.fa[').replace('mslo1[', 'a1.mslo[').replace('k < npass && ', '')


def parse_spline(spl_src):
    """(LDS limit expression of spline12_waves, the lpw expression of launch_spline_eval)."""
    body = _function_body(spl_src, 'static int spline12_waves(')
    m = re.search(r'if \(w \* per_wave <= ([^)]*)\) return w;', body)
    per = re.search(r'const size_t per_wave = ([^;]*);', body)
    launch = _function_body(spl_src, 'int launch_spline_eval(')
    lp = re.search(r'const int lpw = ([^;]*);', launch)
    return m.group(1) if m else None, per.group(1) if per else None, lp.group(1) if lp else None


# ---------------------------------------------------------------------------------------------
# the cases
class LvCase(NamedTuple):
    id: str
    axes: tuple            # (p, n, mult[, repeated interior knots]) per axis
    path: str              # 'lv12' | 'last128' | 'last256' | 'generic'
    geo: str = 'curved'    # 'curved': line x quarter annulus (2D: quarter annulus); 'cube': the unit cube / square
    nqp: int = None        # Gauss points per span (default: max p + 1)
    P: int = None          # lv12: the switch label ..
    npass: int = None      # .. ceil(N2 / 64) ..
    npc: int = None        # .. and ceil(G2 / 128)
    N2: int = None
    G2: int = None
    chunks: tuple = None   # lv12: (clen, nch)
    reason: str = None     # fall-backs: the one reason lv12_shape refuses for

    @property
    def dim(self):
        return len(self.axes)

    def kvs(self):
        return tuple(make_kv(a) for a in self.axes)

    def q(self):
        return int(self.nqp) if self.nqp else max(a[0] for a in self.axes) + 1

    def tables(self):
        q = self.q()
        return tuple(axis_tables(kv, q) for kv in self.kvs())

    def slab_cut(self):
        """First dof plane of the second row slab: its support starts past the first span, so its Gauss slab has g0_lo > 0."""
        a0 = self.tables()[0]
        r = int(np.flatnonzero(a0.mslo > 0)[0])
        return max(r, a0.N // 2)


def _a(p, n, mult=1, rep=()):
    return (p, n, mult, tuple(rep)) if rep else (p, n, mult)


# one line per (P, NPASS) of k_lv12<WEIGHT, P, 5, NPASS> (both WEIGHT: load_vector and the jet functional run every line): axis 0
# has two spans, the mid axis P to 16, the last axis is the smallest that reaches the NPASS (issue table); plus the C4 line
INSTANCE_CASES = [
    LvCase('P2_np2', (_a(1, 2), _a(1, 5), _a(1, 7)), 'lv12', P=2, npass=1, npc=1, N2=8, G2=14, chunks=(5, 1)),
    LvCase('P2_np3', (_a(1, 2), _a(1, 4), _a(1, 128)), 'lv12', P=2, npass=3, npc=2, N2=129, G2=256, chunks=(4, 1)),
    LvCase('P2_np4', (_a(1, 2), _a(1, 3), _a(1, 192)), 'lv12', P=2, npass=4, npc=3, N2=193, G2=384, chunks=(3, 1)),
    LvCase('P3_np2', (_a(2, 2), _a(2, 4), _a(2, 10)), 'lv12', P=3, npass=1, npc=1, N2=12, G2=30, chunks=(4, 1)),
    LvCase('P3_np3', (_a(2, 2), _a(2, 5), _a(2, 128)), 'lv12', P=3, npass=3, npc=3, N2=130, G2=384, chunks=(5, 1)),
    LvCase('P3_np4', (_a(2, 2), _a(2, 3), _a(2, 192)), 'lv12', 'cube', P=3, npass=4, npc=5, N2=194, G2=576, chunks=(3, 1)),
    LvCase('P4_np2', (_a(3, 2), _a(3, 5), _a(3, 40)), 'lv12', P=4, npass=1, npc=2, N2=43, G2=160, chunks=(5, 1)),
    LvCase('P4_np3', (_a(3, 2), _a(3, 4), _a(3, 126)), 'lv12', P=4, npass=3, npc=4, N2=129, G2=504, chunks=(4, 1)),
    LvCase('P4_np4', (_a(3, 2), _a(3, 6), _a(3, 64, 3)), 'lv12', P=4, npass=4, npc=2, N2=193, G2=256, chunks=(6, 1)),
    LvCase('P5_np2', (_a(4, 2), _a(4, 5), _a(4, 12)), 'lv12', P=5, npass=1, npc=1, N2=16, G2=60, chunks=(5, 1)),
    LvCase('P5_np3', (_a(4, 2), _a(4, 5), _a(4, 126)), 'lv12', 'cube', P=5, npass=3, npc=5, N2=130, G2=630, chunks=(5, 1)),
    LvCase('P5_np4', (_a(4, 2), _a(4, 7), _a(4, 48, 4)), 'lv12', P=5, npass=4, npc=2, N2=193, G2=240, chunks=(7, 1)),
    LvCase('P6_np2', (_a(5, 2), _a(5, 6), _a(5, 8)), 'lv12', P=6, npass=1, npc=1, N2=13, G2=48, chunks=(6, 1)),
    LvCase('P6_np3', (_a(5, 2), _a(5, 6), _a(5, 26, 5)), 'lv12', P=6, npass=3, npc=2, N2=131, G2=156, chunks=(6, 1)),
    LvCase('P6_np4', (_a(5, 2), _a(5, 7), _a(5, 39, 5)), 'lv12', P=6, npass=4, npc=2, N2=196, G2=234, chunks=(7, 1)),
    # the last axis of BASELINE config 4 (p = 4, 128 spans) with a short axis 0 and mid axis: G2 = 640 exactly
    LvCase('c4_line', (_a(4, 2), _a(4, 6), _a(4, 128)), 'lv12', 'cube', P=5, npass=3, npc=5, N2=132, G2=640, chunks=(6, 1)),
]

# several chunks of the mid axis (axis 0 is short: nch = n1 / max(P, 8) before the rounding of the chunk length)
CHUNK_CASES = [
    LvCase('ch_P2', (_a(1, 2), _a(1, 17), _a(1, 4)), 'lv12', P=2, npass=1, npc=1, N2=5, G2=8, chunks=(9, 2)),
    # 67 spans at P = 3: eight chunks of 9, the last of 4
    LvCase('ch_P3_n67', (_a(2, 2), _a(2, 67), _a(2, 4)), 'lv12', P=3, npass=1, npc=1, N2=6, G2=12, chunks=(9, 8)),
    LvCase('ch_P4_n67', (_a(3, 2), _a(3, 67), _a(3, 5)), 'lv12', P=4, npass=1, npc=1, N2=8, G2=20, chunks=(9, 8)),
    LvCase('ch_P5', (_a(4, 2), _a(4, 24), _a(4, 4)), 'lv12', P=5, npass=1, npc=1, N2=8, G2=20, chunks=(8, 3)),
    # 65 spans at p = 5: eight chunks of 9 would leave 2 spans, fewer than P: the last chunk joins its neighbour
    LvCase('ch_P6_n65', (_a(5, 2), _a(5, 65), _a(5, 4)), 'lv12', P=6, npass=1, npc=1, N2=9, G2=24, chunks=(9, 7)),
    # repeated knots on the mid axis: double, C^0 (p = 3 and p = 2), and a mix: of four chunks of 8 spans, triple knots ON the
    # boundary 8, a double knot one span past the boundary 16, one span before the boundary 24, and a triple one inside chunk 0
    LvCase('ch_mult2', (_a(3, 2), _a(3, 40, 2), _a(3, 5)), 'lv12', P=4, npass=1, npc=1, N2=8, G2=20, chunks=(8, 5)),
    LvCase('ch_c0_p3', (_a(3, 2), _a(3, 40, 3), _a(3, 5)), 'lv12', P=4, npass=1, npc=1, N2=8, G2=20, chunks=(8, 5)),
    LvCase('ch_c0_p2', (_a(2, 2), _a(2, 33, 2), _a(2, 4)), 'lv12', P=3, npass=1, npc=1, N2=6, G2=12, chunks=(9, 4)),
    LvCase('ch_mixed', (_a(3, 2), _a(3, 32, 1, ((5, 2), (8, 2), (17, 1), (23, 1))), _a(3, 5)), 'lv12', P=4, npass=1, npc=1, N2=8, G2=20,
           chunks=(8, 4)),
    LvCase('ch_np3', (_a(2, 2), _a(2, 16), _a(2, 128)), 'lv12', P=3, npass=3, npc=3, N2=130, G2=384, chunks=(8, 2)),
    # many Gauss planes: the number of chunks comes from the 8192 waves (ceil(8192 / 120) = 69), not from the chunk length
    LvCase('ch_g0cap', (_a(1, 60), _a(1, 600), _a(1, 1)), 'lv12', 'cube', P=2, npass=1, npc=1, N2=2, G2=2, chunks=(9, 67)),
]

# what k_lv12 refuses: one case per reason (that reason alone), both block sizes of k_contract_last with a line count that is no
# multiple of LPB, the generic kernel, 2D
FALLBACK_CASES = [
    LvCase('fb_degrees', (_a(3, 6), _a(2, 5), _a(4, 4)), 'last128', reason='degrees'),                    # 750 lines
    LvCase('fb_oddG2_n133', (_a(2, 3), _a(2, 5), _a(2, 131)), 'last256', reason='oddG2'),                 # 135 lines, N2 = 133
    LvCase('fb_G2_648', (_a(3, 2), _a(3, 4), _a(3, 162)), 'last256', 'cube', reason='G2>640'),
    LvCase('fb_N2_301', (_a(1, 2), _a(1, 3), _a(1, 300)), 'generic', reason='N2>256'),
    LvCase('fb_PQ42', (_a(6, 2), _a(5, 6), _a(5, 4)), 'generic', reason='PQ>36'),                         # nqp = 7 from axis 0
    LvCase('fb_nqp13', (_a(2, 2), _a(2, 4), _a(2, 4)), 'generic', nqp=13, reason='PQ>36'),                # P q = 39
    LvCase('fb_lds', (_a(5, 2), _a(5, 6), _a(5, 48, 5)), 'last256', reason='lds'),                        # 36 * 241 + 4 * 288 doubles
    LvCase('fb_shortmid', (_a(3, 2), _a(3, 3), _a(3, 6)), 'last128', reason='shortmid'),
    LvCase('fb_last_mult2', (_a(2, 3), _a(2, 5), _a(2, 7, 2)), 'last128', reason='oddG2'),                # repeated knots on the last axis
    LvCase('fb_2d_fast', (_a(2, 5), _a(2, 9, 2)), 'last128', reason='2d'),                                # 15 lines
    LvCase('fb_2d_n141', (_a(2, 3), _a(1, 140)), 'last256', reason='2d'),                                 # 9 lines
    LvCase('fb_2d_generic', (_a(1, 3), _a(1, 300)), 'generic', reason='2d'),
]

ALL_CASES = INSTANCE_CASES + CHUNK_CASES + FALLBACK_CASES
BY_ID = {c.id: c for c in ALL_CASES}
LV12_CASES = [c for c in ALL_CASES if c.path == 'lv12']
# the adjoint pair of tests/test_lv_kernels_gpu.py: one NPASS = 3 case and one chunked case with repeated knots
ADJOINT_CASES = ('P3_np3', 'ch_mixed')


class SplineCase(NamedTuple):
    id: str
    degrees: tuple
    spans: tuple
    grad: bool
    waves: int             # spline12_waves (0: refused on the host)
    lpw: int

    @property
    def dim(self):
        return len(self.degrees)

    def nlines(self):
        q = max(self.degrees) + 1
        return int(np.prod([n * q for n in self.spans[:-1]]))

    def nlast(self):
        return self.spans[-1] + self.degrees[-1]


SPLINE_CASES = [
    SplineCase('3d_lines364', (1, 1, 1), (182, 182, 1), True, 4, 8),       # 364 x 364 grid lines: lpw = 8
    SplineCase('3d_last700', (1, 1, 1), (2, 2, 699), True, 2, 1),
    SplineCase('3d_last1400', (1, 1, 1), (2, 2, 1399), True, 1, 1),
    SplineCase('3d_last2800', (1, 1, 1), (2, 2, 2799), True, 0, 1),
    SplineCase('2d_last1100', (1, 1), (2, 1099), True, 2, 1),
]
SPLINE_BY_ID = {c.id: c for c in SPLINE_CASES}

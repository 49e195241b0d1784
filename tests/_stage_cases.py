"""The stage chain of the global sum factorisation -- k_stageA, k_stageB, k_combine, k_final, k_final_q, k_final_mfma
(pyiga_amd/csrc/sumfact.hip, sumfact_stages.h, sumfact_hi.hip) -- restated, and one small patch per compiled instantiation.

Plain helper module (not a conftest), the counterpart of ``tests/_bf3_cases.py`` and ``tests/_geoa_cases.py`` for the kernels
that serve every patch the fast chain refuses: ``tests/test_stage_coverage_cpu.py`` checks that the restatement, the ledger and
the dispatch lines of the sources cannot drift apart, ``tests/test_stage_kernels_gpu.py`` assembles every case on the device
against the CPU oracle.

An axis is a spec (p, n, rep) as in ``_bf3_cases.axis_knots``; P = p + 1 functions per span; q = max degree + 1 Gauss points
per span on every axis (the default nqp, all the oracle computes).  The instantiations:
  * ``k_stageA<P, Q, SYM, ONE, PF>``: P of axis 0, Q = P (compile-time q) or 0, lower pairs only, one type per group (the host
    splits two-type groups), next-span field prefetch (2D);
  * ``k_stageB<P, Q>``: P of axis 1; its body is chosen per last-axis type by the number of terms NTERM = 1 .. 9, and from
    NTERM = 5 on the body takes q at run time whatever Q is;
  * ``k_final<P, NY, Q, KPY, SIMPLE>``, ``k_final_q<P, NY>``, ``k_final_mfma<NY, NCH>``: P of the last axis, NY = 1 or 4 K arrays.
"""
import collections
import math
import os
import re
import types

import numpy as np

import _bf3_cases as bc
import _geoa_cases as gc
import _solver_cases as sc

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'pyiga_amd', 'csrc')
SUMFACT_HIP = os.path.join(CSRC, 'sumfact.hip')
STAGES_H = os.path.join(CSRC, 'sumfact_stages.h')
SUMFACT_HI_HIP = os.path.join(CSRC, 'sumfact_hi.hip')
IGX_H = os.path.join(CSRC, '..', '..', 'include', 'igx.h')

# ---- the restated constants (test_stage_coverage_cpu.py compares each with the sources)
WANT = 2048                      # sweep_chunks: blocks a sweep launch should have
MIN_LEN = 4                      # ... chunks of at least 4 P spans (3D); stage A in 2D: P spans
TOO_SHORT = 2                    # ... no chunks below 2 * min_len spans
BS_A = 256                       # run_stage0: threads per block of k_stageA
BS_B = (128, 256)                # run_mid: threads per block of k_stageB below / from P = HI_P
SWEEP_MAX_STAGE = 8              # sumfact_stages.h: PI slice values staged per thread
ONE_MIN_P = 5                    # run_stage0: one_type from this P (non-symmetric, q == P)
HI_P = 7                         # launch_stageA / launch_stageB / launch_final: the plain instantiations from this P
DISPATCH_P = (2, 6)              # sumfact.hip: DISPATCH_P
MAX_P = 8                        # include/igx.h: IGX_MAX_SF_DEGREE + 1
CR_WINDOW = 512                  # run_final: crmax = min(64, 512 / q - p)
TILE_LDS = 64 * 1024             # ... a row tile's basis segment
LDS_MAX = 160 * 1024             # ... the whole block
KPY_MAX = 8
BODY_RT_Q = 5                    # k_stageB: bodies of NTERM >= 5 take q at run time
FINALQ_WAVES = 4                 # sumfact.hip: FINALQ_WAVES
FINALQ_MAX_P = 6                 # sumfact_plan: k_final_q for P <= 6
TARGET_WAVES = 8192              # run_final: k_final_q
FINALQ_MIN_LPW = (16, 4)         # ... lines per block at least; in the per_super branch
FINALQ_SLOTS = 2 * 256           # ... blocks of one resident round
MFMA_NCH = (1, 6)                # sumfact_plan: k_final_mfma for NCH in this range

# axis 0 of the geometry maps the oracle has: (degree, spans) -- all of them B-spline or NURBS maps k_geoA takes
GEOS_3D = ('cylinder', 'twisted_box')
GEOS_2D = ('quarter_annulus', 'bspline_quarter_annulus')
GEO_AXIS0 = {'cylinder': (1, 1), 'twisted_box': (1, 1), 'quarter_annulus': (2, 1), 'bspline_quarter_annulus': (2, 1)}

StageA = collections.namedtuple('StageA', 'P Q SYM ONE PF')
StageB = collections.namedtuple('StageB', 'P Q')
Final = collections.namedtuple('Final', 'kernel args')
Keys = collections.namedtuple('Keys', 'stageA stageB nterm combine final shape')


class Unsupported(ValueError):
    """The stage chain refuses the patch with IGX_ERR_UNSUPPORTED."""


# ---- coefficient tables: which of the four jet blocks are present decides the terms (igx_api.hip / rtc.hip: form_terms).
# Expressions in x, y only, so that a table serves 2D and 3D; 2D reads the entries with indices below 3.
def _tab(d00=False, conv_u=False, conv_v=False, diff=False, sym=False):
    T = [[None] * 4 for _ in range(4)]
    if d00:
        T[0][0] = '2.0 + x * y'
    if conv_u:
        T[0][1], T[0][2] = 'y', '-0.5 * x'
    if conv_v:
        T[1][0], T[2][0] = ('y', '-0.5 * x') if sym else ('0.25 * x', '1.0 + y')
    if diff:
        T[1][1], T[2][2], T[3][3] = '1.5 + x', '2.0', '1.0 + 0.5 * y'
        T[1][2] = T[2][1] = '0.25 * y'
    return T


TABLES = {
    'react': _tab(d00=True),                                        # NTERM of the last-axis type 0: 1
    'conv': _tab(conv_u=True),                                      # 2
    'react_conv': _tab(d00=True, conv_u=True),                      # 3
    'diff': _tab(diff=True),                                        # 4 (symmetric table)
    'diff_react': _tab(d00=True, diff=True),                        # 5 (symmetric table)
    'diff_conv': _tab(conv_u=True, diff=True),                      # 6
    'diff_react_conv': _tab(d00=True, conv_u=True, diff=True),      # 7
    'diff_conv2': _tab(conv_u=True, conv_v=True, diff=True),        # 8
    'full': _tab(d00=True, conv_u=True, conv_v=True, diff=True),    # 9
    'full_sym': _tab(d00=True, conv_u=True, conv_v=True, diff=True, sym=True),   # 9, symmetric table
}


def table_blocks(T):
    """[test is a derivative][trial is a derivative] -> some entry of the block is present."""
    blk = [[False, False], [False, False]]
    for r in range(4):
        for s in range(4):
            if T[r][s] is not None:
                blk[r > 0][s > 0] = True
    return blk


def table_oracle(T, dim):
    """The table as the oracle takes it: constants, functions of the physical coordinates, None."""
    def entry(e):
        if e is None:
            return None
        try:
            return float(e)
        except ValueError:
            return lambda *c, e=e: eval(e, {'__builtins__': {}}, dict(x=c[0], y=c[1])) + 0.0 * c[0]
    return [[entry(e) for e in row] for row in T]


# ---- the terms of a form (sumfact_stages.h: form_terms): (field, type per axis), type = tu + 2 tv
def _sym_index(d, r, c):
    if r > c:
        r, c = c, r
    return sum(d - rr for rr in range(r)) + (c - r)


def form_terms(dim, kind, table=None):
    if kind == 'form':
        blk = table_blocks(TABLES[table] if isinstance(table, str) else table)
        out = []
        for a in range(dim + 1):
            for b in range(dim + 1):
                if blk[a > 0][b > 0]:
                    out.append((len(out), tuple((1 if b >= 1 and ax == dim - b else 0) + 2 * (1 if a >= 1 and ax == dim - a else 0)
                                                for ax in range(dim))))
        return out
    if kind == 'mass':
        return [(0, (0,) * dim)]
    out = [(_sym_index(dim, dim - 1 - a, dim - 1 - b), tuple((1 if k == a else 0) + 2 * (1 if k == b else 0) for k in range(dim)))
           for a in range(dim) for b in range(dim)]
    if kind == 'convdiff':
        out += [(dim * (dim + 1) // 2 + (dim - 1 - a), tuple(1 if k == a else 0 for k in range(dim))) for a in range(dim)]
    return out


# ---- the tables of an axis (igx_api.hip: build_axis)
Axis = collections.namedtuple('Axis', 'p P n N S simple mslo mshi jlo jhi')


def axis_tables(spec):
    knots, p = bc.axis_knots(spec), spec[0]
    mesh = np.unique(knots)
    k2m = np.searchsorted(mesh, knots)
    N = knots.size - p - 1
    assert mesh.size - 1 == spec[1], ('the knot expression of this spec makes an extra, empty span', spec[:2])
    jlo, jhi = sc.axis_ranges(types.SimpleNamespace(kv=knots, p=p))
    return Axis(p, p + 1, mesh.size - 1, N, int((jhi - jlo).sum()), not bc.repeated(spec), k2m[:N], k2m[p + 1:p + 1 + N], jlo, jhi)


def sweep_chunks(blocks_without, nspans, P, min_len=0):
    """(chunks, chunk length in spans): sumfact.hip, sweep_chunks."""
    if min_len <= 0:
        min_len = MIN_LEN * P
    if blocks_without >= WANT or nspans < TOO_SHORT * min_len:
        return 1, nspans
    n = max(min(-(-WANT // blocks_without), nspans // min_len), 1)
    length = -(-nspans // n)
    return -(-nspans // length), length


def _knobs(knobs):
    k = dict(knobs or {})
    assert set(k) <= {'IGX_PATH', 'IGX_GEOA', 'IGX_FINAL'}, k
    path = {None: 0, 'fused': 1, 'unfused': 2, 'single': 3}.get(k.get('IGX_PATH'), 0)
    geoa = k.get('IGX_GEOA', '1') != '0'
    fin = k.get('IGX_FINAL')
    final_sel = 0 if fin is None else {'q': 1, 'valu': 2, 'mfma': 3}.get(fin, 1)
    return path, geoa, final_sel


def _other_chain(ax, dim, kind, table, path, geoa, final_sel, q):
    """sumfact_plan up to the stage chain: True where a twin, the form-table chain, the single-launch 2D kernel or the fused
    stage takes the patch.  Any of IGX_PATH=unfused and IGX_FINAL switches all four off."""
    if path == 2 or final_sel:
        return False
    sym = kind in ('mass', 'stiffness')
    specs = [(a.p, a.simple) for a in ax]
    if dim == 2:
        if kind in ('mass', 'stiffness') and max(a.P for a in ax) <= 6:
            if path == 3:
                return True
            if path == 0:
                # single2d_wanted: one resident round of tiles of at most 6 x 6 rows.  Sure only past the round of the largest
                # tile; below it the LDS image decides (kern_basis.hip: single2d_plan), which is not restated
                if math.ceil(ax[0].N / 8) * math.ceil(ax[1].N / 8) <= gc.SINGLE2D_MAX_BLOCKS:
                    raise ValueError('2D patch within the reach of the single-launch kernel: not restated, set IGX_PATH')
                return False
        if path != 1:
            return False
        AM, AL = ax
        return AM.simple and AL.simple and AM.P == AL.P == q and 2 <= AL.P <= 6
    AM, AL = ax[1], ax[2]
    if not AL.simple:
        # repeated knots on the last axis only: the twin, where its chain is k_geoA -> k_bf3
        if AM.simple and geoa and kind != 'form' and bc.fused3_degrees(AL.P, AM.P, q, sym, False) and \
                2 <= ax[0].P <= 6 and (kind != 'convdiff' or ax[0].P >= 3):
            return True
        if kind == 'form':
            raise ValueError('a coefficient table on a patch with a twin: not restated, set IGX_PATH')
        return False
    if kind == 'form':
        raise ValueError('a coefficient table without IGX_PATH=unfused: the form-table chain decides, see _geoa_cases.geoa_route')
    axes3 = bc.fused3_degrees(AM.P, AL.P, q, sym, AM.simple)
    fused2 = AM.simple and AM.P == AL.P == q and 2 <= AL.P <= 6
    return axes3 or fused2


def stage_keys(axes, kind, knobs=None, table=None, geo=None):
    """What sumfact_plan, run_stage0, run_mid and run_final launch for the whole patch `axes` (specs (p, n, rep)) and the form
    `kind` ('mass', 'stiffness', 'convdiff', 'form' with `table`) under the creation-time knobs IGX_PATH, IGX_GEOA, IGX_FINAL:
    Keys(stage-A instantiation or 'geoA', stage-B instantiation or None (2D), NTERM of every last-axis type with terms,
    k_combine runs, final kernel, shape quantities).  None where the plan takes another chain."""
    dim = len(axes)
    assert dim in (2, 3) and (kind != 'convdiff' or dim == 3)
    ax = [axis_tables(a) for a in axes]
    if any(a.P < 2 or a.P > MAX_P for a in ax):
        raise Unsupported('degree')
    q = max(a.p for a in ax) + 1
    path, geoa, final_sel = _knobs(knobs)
    sym = kind in ('mass', 'stiffness')
    if _other_chain(ax, dim, kind, table, path, geoa, final_sel, q):
        return None
    A0, AL = ax[0], ax[-1]
    G = [a.n * q for a in ax]
    terms = form_terms(dim, kind, table)
    shape = {}
    # ---- stage-A arrays: unique (axis-0 type, field) in 3D, one per term in 2D
    X = []
    for f, t in terms:
        if dim == 2 or (t[0], f) not in X:
            X.append((t[0], f))
    np0 = int((np.arange(A0.N) - A0.jlo + 1).sum()) if sym else A0.S
    NPL = G[1] * (G[2] if dim == 3 else 1)
    P0 = A0.P
    geoA_ok = sym and geoa and len(X) == ((1 if kind == 'mass' else 8) if dim == 3 else (1 if kind == 'mass' else 4)) and \
        2 <= P0 <= (6 if dim == 3 else 5) and (geo is None or 2 * GEO_AXIS0[geo][1] <= G[0])
    qeq0 = q == P0
    one_type = not sym and P0 >= ONE_MIN_P and qeq0
    if geoA_ok:
        stageA = 'geoA'
        shape['chunksA'] = sweep_chunks(-(-NPL // 64), A0.n, P0, gc.CHUNK_MIN_2D * P0 if dim == 2 else 0)
    else:
        if q * 4 * P0 * P0 > SWEEP_MAX_STAGE * BS_A:
            raise Unsupported('stage A: coefficient slice too large')
        fields = collections.Counter(f for _, f in X)
        ng = sum(2 if one_type and c == 2 else 1 for c in fields.values())
        assert max(fields.values()) <= 2 and ng <= 16
        shape['groupsA'] = ng
        shape['chunksA'] = sweep_chunks(-(-NPL // BS_A) * ng, A0.n, P0, P0 if dim == 2 else 0)
        if not sym and one_type:
            stageA = StageA(P0, P0, False, True, False)
        elif P0 >= HI_P:
            stageA = StageA(P0, 0, sym, False, False)
        elif sym:
            stageA = StageA(P0, P0 if qeq0 else 0, True, False, qeq0 and dim == 2)
        else:
            stageA = StageA(P0, P0 if qeq0 else 0, False, False, False)
    # ---- stage B (3D) or k_combine (2D general forms)
    stageB = nterm = None
    combine = False
    ylast = [0 if kind == 'mass' else t[dim - 1] for _, t in terms]
    NY = 1 if max(ylast) == 0 else 4
    if dim == 3:
        A1 = ax[1]
        nterm = tuple(sorted(collections.Counter(ylast).items()))
        assert max(n for _, n in nterm) <= 9
        bs = BS_B[1] if A1.P >= HI_P else BS_B[0]
        if q * 4 * A1.P * A1.P > SWEEP_MAX_STAGE * bs:
            raise Unsupported('stage B: coefficient slice too large')
        shape['chunksB'] = sweep_chunks(-(-G[2] // bs) * np0 * NY, A1.n, A1.P)
        stageB = StageB(A1.P, A1.P if q == A1.P and A1.P < HI_P else 0)
        nlines = np0 * A1.S
        if sym:
            ndesc = 0
            for i0 in range(A0.N):
                for j0 in range(A0.jlo[i0], i0 + 1):
                    ndesc += int((np.arange(A1.N) - A1.jlo + 1).sum()) if i0 == j0 else A1.S
        else:
            ndesc = nlines
    else:
        if kind != 'mass' and kind != 'form':
            NY = 4
        combine = kind == 'form'
        ndesc = np0
    # ---- the final stage
    PL, W = AL.P, 2 * AL.P - 1
    final = None
    if final_sel == 3 and sym and G[-1] >= 2:
        wmax = 0
        for t in range((AL.N * W + 15) // 16):
            i_first, i_last = min(AL.N - 1, (t * 16) // W), min(AL.N - 1, (t * 16 + 15) // W)
            wmax = max(wmax, int(AL.mshi[i_last] - AL.mslo[i_first]) * q)
        shape['mfma_nch'] = (wmax + 7) // 8
        if MFMA_NCH[0] <= shape['mfma_nch'] <= MFMA_NCH[1]:
            final = Final('k_final_mfma', (NY, shape['mfma_nch']))
    if final is None and final_sel != 2 and q == PL and AL.simple and PL <= FINALQ_MAX_P:
        R = 64 // PL
        nchunks = -(-AL.N // R)
        nsuper = -(-nchunks // FINALQ_WAVES)
        lpw = max(FINALQ_MIN_LPW[0], -(-ndesc * nsuper * FINALQ_WAVES // TARGET_WAVES))
        per_super = FINALQ_SLOTS // nsuper
        branch = per_super > 0 and -(-ndesc // 16) * nsuper <= FINALQ_SLOTS
        if branch:
            lpw = max(FINALQ_MIN_LPW[1], -(-ndesc // per_super))
        shape.update(q_nchunks=nchunks, q_nsuper=nsuper, q_lpw=lpw, q_per_super=branch, q_ndesc=ndesc,
                     q_last_rows=AL.N - (nchunks - 1) * R)
        final = Final('k_final_q', (PL, NY))
    if final is None:
        SSTR, KSTR = (q * PL * 2) | 1, q | 1
        crmax = max(1, min(64, CR_WINDOW // q - AL.p))
        ntiles = 1
        while True:
            rows_per_tile = -(-AL.N // ntiles)
            nch = -(-rows_per_tile // crmax)
            CR = -(-rows_per_tile // nch)
            tile_rows = CR * nch
            tsp_max = trow_max = nsp_max = 0
            for lo in range(0, AL.N, tile_rows):
                hi = min(lo + tile_rows, AL.N)
                tsp_max = max(tsp_max, int(AL.mshi[hi - 1] - AL.mslo[lo]))
                trow_max = max(trow_max, int(AL.jhi[hi - 1] - AL.jlo[lo]))
                for cl in range(lo, hi, CR):
                    nsp_max = max(nsp_max, int(AL.mshi[min(cl + CR, hi) - 1] - AL.mslo[cl]))
            if tsp_max * SSTR * 8 <= TILE_LDS or tile_rows <= crmax:
                break
            ntiles += 1
        ntiles = -(-AL.N // tile_rows)
        kpy = -(-nsp_max * q // 64)
        if kpy > KPY_MAX:
            raise Unsupported('final stage: K window does not fit the prefetch registers')
        vbytes = tsp_max * SSTR * 8
        kslot = max(NY * nsp_max * KSTR, CR * W) * 8
        tbytes = (5 * trow_max + tsp_max) * 4
        if vbytes + kslot + tbytes > LDS_MAX:
            raise Unsupported('final stage: basis table segment does not fit LDS')
        fast = q == PL and AL.simple and PL < HI_P
        shape.update(crmax=crmax, CR=CR, tile_rows=tile_rows, ntiles=ntiles, nsp_max=nsp_max, kpy=kpy, chunks_per_tile=tile_rows // CR,
                     last_chunk_rows=(min(tile_rows, AL.N - (ntiles - 1) * tile_rows) - 1) % CR + 1)
        if PL >= HI_P:
            final = Final('k_final', (PL, NY, 0, 8, False))
        else:
            final = Final('k_final', (PL, NY, PL if fast else 0, 4 if kpy <= 4 else 8, fast))
    shape.update(NY=NY, np0=np0, q=q)
    return Keys(stageA, stageB, nterm, combine, final, shape)


def body_keys(keys):
    """{(NTERM, the kernel has a compile-time q)} of the stage-B bodies a patch runs."""
    if keys is None or keys.stageB is None:
        return set()
    return {(n, keys.stageB.Q != 0) for _, n in keys.nterm}


# ---- the dispatch lines, read from the sources
def read_sources():
    out = []
    for path in (SUMFACT_HIP, STAGES_H, SUMFACT_HI_HIP, IGX_H):
        with open(path) as f:
            out.append(f.read())
    return tuple(out)


def _func(src, start, end='\n}\n'):
    s = src[src.index(start):]
    return s[:s.index(end)]


def _split_hi(body):
    """(the `if constexpr (P >= HI_P)` block, the rest, HI_P) of a launcher."""
    m = re.search(r'if constexpr \(P >= (\d+)\) \{', body)
    rest = body[m.end():]
    depth, i = 1, 0
    while depth:
        depth += {'{': 1, '}': -1}.get(rest[i], 0)
        i += 1
    return rest[:i], body[:m.start()] + rest[i:], int(m.group(1))


def _targs(text, P):
    out = []
    for a in text.split(','):
        a = a.strip()
        out.append(P if a == 'P' else True if a == 'true' else False if a == 'false' else int(a))
    return tuple(out)


def parse_dispatch(srcs=None):
    """Everything the launchers of the stage chain can instantiate, and the constants the restatement depends on."""
    sumfact, stages, hi, igxh = srcs or read_sources()
    d = {}
    macro = gc._macro_def(sumfact, 'DISPATCH_P')
    pairs = re.findall(r'case (\d+): \{ constexpr int PP = (\d+);', macro)
    cases = [int(a) for a, _ in pairs]
    assert cases == [int(b) for _, b in pairs]
    d['DISPATCH_P'] = cases
    hiP = {name: sorted(int(v) for v in re.findall(r'%s<(\d+)>' % name, hi)) for name in ('launch_stageA', 'launch_stageB', 'launch_final')}
    d['hi_P'] = hiP
    # k_stageA
    body = _func(stages, 'static void launch_stageA(')
    hi_part, lo_part, thr = _split_hi(body)
    d['hi_threshold'] = {thr}
    sa = set()
    for part, Ps in ((hi_part, hiP['launch_stageA']), (lo_part, cases)):
        for m in re.findall(r'k_stageA<([^<>]*)><<<', part):
            for P in Ps:
                t = _targs(m, P)
                sa.add(StageA(*(t + (False,) * (5 - len(t)))))
    d['stageA'] = sa
    # k_stageB
    body = _func(stages, 'static void launch_stageB(')
    m = re.search(r'if \(qeq && P < (\d+)\) k_stageB<P, \(P < (\d+) \? P : 0\)><<<', body)
    assert m and 'else k_stageB<P, 0><<<' in body
    d['hi_threshold'] |= {int(m.group(1)), int(m.group(2))}
    allP = cases + hiP['launch_stageB']
    d['stageB'] = {StageB(P, P) for P in allP if P < int(m.group(1))} | {StageB(P, 0) for P in allP}
    kb = _func(stages, '__global__ void __launch_bounds__(256) k_stageB(')
    d['stageB_body'] = sorted((9 if lab == 'default' else int(lab.split()[1]), int(n), qq == 'Q')
                              for lab, n, qq in re.findall(r'(case \d+|default): stageB_body<P, (\d+), (Q|0)>', kb))
    # k_final
    body = _func(stages, 'static int launch_final(')
    hi_part, lo_part, thr = _split_hi(body)
    d['hi_threshold'].add(thr)
    fin = set()
    for part, Ps in ((hi_part, hiP['launch_final']), (lo_part, cases)):
        for m in re.findall(r'launch_final_k<([^<>]*)>\(', part):
            for P in Ps:
                fin.add(Final('k_final', _targs(m, P)))
    d['kpy_split'] = sorted(set(int(v) for v in re.findall(r'kpy <= (\d+) \?', lo_part)))
    rf = _func(sumfact, 'static int run_final(')
    lq = rf[rf.index('#define LAUNCH_Q'):rf.index('#undef LAUNCH_Q')]
    d['LAUNCH_Q'] = [(lab, int(v)) for lab, v in re.findall(r'(case \d+|default): LAUNCH_Q\((\d+)\)', lq)]
    d['LAUNCH_Q_NY'] = sorted(int(v) for v in re.findall(r'k_final_q<PV, (\d+)>', lq))
    for _, P in d['LAUNCH_Q']:
        for NY in d['LAUNCH_Q_NY']:
            fin.add(Final('k_final_q', (P, NY)))
    lm = rf[rf.index('#define LAUNCH_M'):rf.index('#undef LAUNCH_M')]
    d['LAUNCH_M'] = [(lab, int(a), int(b)) for lab, a, b in re.findall(r'(case \d+|default): LAUNCH_M\((\d+), (\d+)\)', lm)]
    for _, NY, NCH in d['LAUNCH_M']:
        fin.add(Final('k_final_mfma', (NY, NCH)))
    d['final'] = fin
    # constants
    sw = _func(sumfact, 'static SweepChunks sweep_chunks(')
    r0 = _func(sumfact, 'static int run_stage0(')
    rm = _func(sumfact, 'static int run_mid(')
    pl = _func(sumfact, 'void sumfact_plan(')
    num = lambda pat, s: int(re.search(pat, s).group(1))
    d['const'] = {
        'WANT': num(r'const long long want = (\d+);', sw),
        'MIN_LEN': num(r'if \(min_len <= 0\) min_len = (\d+) \* P;', sw),
        'TOO_SHORT': num(r'nspans < (\d+) \* min_len', sw),
        'BS_A': num(r'const int bsA = (\d+);', r0),
        'BS_B': tuple(int(v) for v in re.search(r'const int bs = A1\.P >= \d+ \? (\d+) : (\d+);', rm).groups())[::-1],
        'BS_B_P': num(r'const int bs = A1\.P >= (\d+) \?', rm),
        'SWEEP_MAX_STAGE': num(r'constexpr int SWEEP_MAX_STAGE = (\d+);', stages),
        'ONE_MIN_P': num(r'const bool one_type = !sym && A0\.P >= (\d+) && A0\.q == A0\.P;', r0),
        'stageA_2d_min': bool(re.search(r'sweep_chunks\(bx \* ng, pt->s0_hi - pt->s0_lo, A0\.P, dim == 2 \? A0\.P : 0\)', r0)),
        'stageA_hi_P': num(r'if \(A0\.P >= (\d+)\) stageA_hi\(', r0),
        'stageB_hi_P': num(r'if \(A1\.P >= (\d+)\) stageB_hi\(', rm),
        'final_hi_P': num(r'if \(AL\.P >= (\d+)\) rc = final_hi\(', rf),
        'fast_P': num(r'const bool fast = AL\.q == AL\.P && AL\.simple && AL\.P < (\d+);', rf),
        'MAX_P': num(r'#define IGX_MAX_SF_DEGREE (\d+)', igxh) + 1,
        'CR_WINDOW': num(r'std::min\(64, (\d+) / std::max\(AL\.q, 1\) - AL\.p\)', rf),
        'TILE_LDS': eval(re.search(r'sizeof\(double\) <= ([\d* ]+) \|\| tile_rows <= crmax', rf).group(1)),
        'LDS_MAX': eval(re.search(r'vbytes \+ kslot \+ tbytes > ([\d* ]+)\)', rf).group(1)),
        'KPY_MAX': num(r'if \(kpy > (\d+)\)', rf),
        'kpy': bool(re.search(r'const int kpy = \(nsp_max \* AL\.q \+ 63\) / 64;', rf)),
        'BODY_RT_Q': min(n for _, n, ct in d['stageB_body'] if not ct),
        'FINALQ_WAVES': num(r'#define IGX_Q_WAVES (\d+)', sumfact),
        'FINALQ_MAX_P': num(r'AL\.q == AL\.P && AL\.simple && AL\.P <= (\d+)\) pl\.fin = Plan::FINAL_Q;', pl),
        'TARGET_WAVES': num(r'long long target_waves = (\d+);', rf),
        'FINALQ_MIN_LPW': (num(r'Q\.lpw = \(int\)std::max<long long>\((\d+), \(Q\.ndesc \* Q\.nsuper', rf),
                           num(r'Q\.lpw = \(int\)std::max<long long>\((\d+), \(Q\.ndesc \+ per_super', rf)),
        'FINALQ_SLOTS': eval(re.search(r'const long long slots = ([\d* ]+),', rf).group(1)),
        'FINALQ_R': bool(re.search(r'const int R = 64 / AL\.P;', rf)),
        'MFMA_NCH': tuple(int(v) for v in re.search(r'pl\.mfma_nch >= (\d+) && pl\.mfma_nch <= (\d+)\) pl\.fin = Plan::FINAL_MFMA;', pl).groups()),
        'mfma_nch': bool(re.search(r'pl\.mfma_nch = \(wmax \+ 7\) / 8;', pl)),
    }
    return d


MODULE_CONSTANTS = dict(WANT=WANT, MIN_LEN=MIN_LEN, TOO_SHORT=TOO_SHORT, BS_A=BS_A, BS_B=BS_B, BS_B_P=HI_P, SWEEP_MAX_STAGE=SWEEP_MAX_STAGE,
                        ONE_MIN_P=ONE_MIN_P, stageA_2d_min=True, stageA_hi_P=HI_P, stageB_hi_P=HI_P, final_hi_P=HI_P, fast_P=HI_P,
                        MAX_P=MAX_P, CR_WINDOW=CR_WINDOW, TILE_LDS=TILE_LDS, LDS_MAX=LDS_MAX, KPY_MAX=KPY_MAX, kpy=True,
                        BODY_RT_Q=BODY_RT_Q, FINALQ_WAVES=FINALQ_WAVES, FINALQ_MAX_P=FINALQ_MAX_P, TARGET_WAVES=TARGET_WAVES,
                        FINALQ_MIN_LPW=FINALQ_MIN_LPW, FINALQ_SLOTS=FINALQ_SLOTS, FINALQ_R=True, MFMA_NCH=MFMA_NCH, mfma_nch=True)


# ---- compiled, but no patch gets there: (instantiation, one-line derivation, check).  The check evaluates the restatement at
# its extremes and returns True if the derivation holds (test_stage_coverage_cpu.py).
def _fast_kpy8_impossible(P):
    """Fast k_final (q == P, single knots): a wave task has CR <= crmax = min(64, 512 / P - p) rows, so nsp_max <= crmax + p spans
    and KPY = 8 needs (crmax + p) * P > 256."""
    crmax = max(1, min(64, CR_WINDOW // P - (P - 1)))
    if (crmax + P - 1) * P > 4 * 64:
        return False
    worst = 0
    for n in range(1, 3 * 64):                               # ... and the restatement agrees at every length up to three tasks
        k = stage_keys(((P - 1, 2, 1), (P - 1, n, (1,) * (n - 1)) if n > 1 else (P - 1, 1, 1)), 'mass', {'IGX_FINAL': 'valu'})
        worst = max(worst, k.shape['kpy'])
    return worst <= 4


def _one_needs_p5(P):
    """ONE is chosen by one_type = !sym && P >= 5 && q == P alone."""
    return P < ONE_MIN_P and all(stage_keys(((P - 1, 2, 1), (P - 1, 2, 1)), 'form', {'IGX_PATH': 'unfused'}, table=t).stageA.ONE is False
                                 for t in ('conv', 'full'))


def _two_types_nonsym_p5(P):
    """Non-symmetric with q == P: from P = 5 on one_type holds, so the ONE instantiation runs instead."""
    return P >= ONE_MIN_P and all(stage_keys(((P - 1, 2, 1),) * 3, kind, {'IGX_PATH': 'unfused'}, table=t).stageA == StageA(P, P, False, True, False)
                                  for kind, t in (('convdiff', None), ('form', 'full')))


def _q0_nonsym_p8(P):
    """P = 8 is the highest degree the chain takes, so q == P on every patch and a non-symmetric form runs ONE."""
    return P == MAX_P and stage_keys(((P - 1, 1, 1), (1, 2, 1), (1, 2, 1)), 'convdiff', {'IGX_PATH': 'unfused'}).stageA == StageA(P, P, False, True, False)


UNREACHABLE = []
for _P in (2, 3):
    for _NY in (1, 4):
        UNREACHABLE.append((Final('k_final', (_P, _NY, _P, 8, True)),
                            'fast k_final: nsp_max <= 64 + p spans of P points: %d <= 256, KPY = 4' % ((64 + _P - 1) * _P),
                            lambda P=_P: _fast_kpy8_impossible(P)))
for _P in (2, 3, 4):
    UNREACHABLE.append((StageA(_P, _P, False, True, False), 'ONE needs one_type, which needs P >= 5', lambda P=_P: _one_needs_p5(P)))
for _P in (5, 6):
    UNREACHABLE.append((StageA(_P, _P, False, False, False), 'non-symmetric, q == P, P >= 5: one_type, the ONE instantiation runs',
                        lambda P=_P: _two_types_nonsym_p5(P)))
UNREACHABLE.append((StageA(8, 0, False, False, False), 'P = 8 is the highest degree: q == P, so a non-symmetric form has one_type',
                    lambda: _q0_nonsym_p8(8)))
UNREACHABLE_KEYS = {u[0] for u in UNREACHABLE}


# ---- the ledger
Case = collections.namedtuple('Case', 'id axes geo kind table knobs stageA stageB final slabs')
UNF = {'IGX_PATH': 'unfused'}


def _kn(**kw):
    k = dict(UNF)
    k.update({'IGX_' + a.upper(): v for a, v in kw.items()})
    return k


def _ax_tag(axes):
    return '-'.join('p%dn%d%s' % (p, n, '' if rep == 1 else 'm' + ''.join(map(str, np.atleast_1d(rep)))) for p, n, rep in axes)


_geo_turn = [0]


def _mk(axes, kind, knobs, table=None, geo=None, stageA=None, stageB=None, final=None):
    """A case with the instantiations it is in the ledger for (None: whatever the patch runs); the geometry maps take turns."""
    dim = len(axes)
    if geo is None:
        _geo_turn[0] += 1
        geo = (GEOS_3D if dim == 3 else GEOS_2D)[_geo_turn[0] % 2]
    k = '-'.join('%s=%s' % (a[4:].lower(), v) for a, v in sorted(knobs.items()))
    cid = '-'.join(x for x in (kind, table, _ax_tag(axes), geo, k) if x)
    return Case(cid, tuple(axes), geo, kind, table, knobs, stageA, stageB, final, False)


# KPY = 8 needs a wave task whose K window passes 256 points: (P, generic) -> (degree of axis 0, spans of the last axis), the
# shortest last axis that gets there (fast: q == P; generic: axis 0 one degree up, or as far up as a task of at most 64 rows needs)
_KPY8 = {(4, False): (3, 181), (5, False): (4, 52), (6, False): (5, 43),
         (2, True): (3, 189), (3, True): (3, 185), (4, True): (4, 52), (5, True): (5, 43), (6, True): (6, 37)}


def _build_cases():
    cases = []
    # ---- k_final, every reachable (P, NY, Q, KPY, SIMPLE)
    for P in range(2, 7):
        p = P - 1
        for NY, kind in ((1, 'mass'), (4, 'stiffness')):
            # fast, KPY = 4: 3D, equal degrees, IGX_FINAL=valu; stage A with and without the geometry inside
            cases.append(_mk(((p, 2, 1), (p, 3, 1), (p, 4, 1)), kind, _kn(final='valu', geoa='0' if NY == 4 else '1'),
                             stageA=StageA(P, P, True, False, False) if NY == 4 else 'geoA', stageB=StageB(P, P),
                             final=Final('k_final', (P, NY, P, 4, True))))
            # fast, KPY = 8: 2D with a long last axis (P >= 4: UNREACHABLE below)
            if P >= 4:
                p0, n1 = _KPY8[(P, False)]
                cases.append(_mk(((p0, 3, 1), (p, n1, 1)), kind, _kn(final='valu', geoa='0'),
                                 stageA=StageA(P, P, True, False, True), final=Final('k_final', (P, NY, P, 8, True))))
            # generic, KPY = 4: 3D; repeated knots on the mid and the last axis, or a last axis below the others (P = 2 and NY = 1)
            if P == 2 or NY == 1:
                axes = ((p + 1, 2, 1), (p + 1, 2, 2 if p >= 1 else 1), (p, 4, 1))
                sA, sB = ('geoA', StageB(P + 1, P + 1)) if P < 6 else (StageA(7, 0, True, False, False), StageB(7, 0))
            else:
                axes = ((p, 3, 2), (p, 3, (1, p)), (p, 4, (2, 1, p)))
                sA, sB = 'geoA', StageB(P, P)
            cases.append(_mk(axes, kind, _kn(), stageA=sA, stageB=sB, final=Final('k_final', (P, NY, 0, 4, False))))
            # generic, KPY = 8: 2D with a long last axis below the degree of axis 0
            p0, n1 = _KPY8[(P, True)]
            sA = StageA(p0 + 1, p0 + 1, True, False, True) if p0 + 1 < HI_P else StageA(p0 + 1, 0, True, False, False)
            cases.append(_mk(((p0, 3, 1), (p, n1, 1)), kind, _kn(geoa='0'), stageA=sA, final=Final('k_final', (P, NY, 0, 8, False))))
    for P in (7, 8):
        p = P - 1
        cases.append(_mk(((p, 2, 1), (p, 3, 1)), 'mass', _kn(), stageA=StageA(P, 0, True, False, False), final=Final('k_final', (P, 1, 0, 8, False))))
        cases.append(_mk(((p, 2, 2), (p, 2, 3)), 'stiffness', _kn(), stageA=StageA(P, 0, True, False, False), final=Final('k_final', (P, 4, 0, 8, False))))
    # ---- k_final_q, every (P, NY): 3D and 2D, the default final kernel of these patches once the chain is unfused
    for P in range(2, 7):
        p = P - 1
        cases.append(_mk(((p, 2, 1), (p, 2, 1), (p, 5, 1)), 'mass', _kn(geoa='0'), stageA=StageA(P, P, True, False, False), stageB=StageB(P, P),
                         final=Final('k_final_q', (P, 1))))
        cases.append(_mk(((max(p - 1, 1), 3, 1), (p, 64 // P + 3, 1)), 'stiffness', _kn(geoa='0'),
                         stageA=StageA(max(P - 1, 2), 0 if P > 2 else 2, True, False, P == 2), final=Final('k_final_q', (P, 4))))
    # ---- k_final_mfma, every (NY, NCH): the window of a 16-slot tile is (rows + p) spans of q points
    # (last axis, the degree the other axes have): NCH = ceil(window / 8)
    mf = {1: ((1, 1, 1), 1), 2: ((2, 3, 1), 1), 3: ((2, 7, 1), 2), 4: ((3, 10, 1), 2), 5: ((4, 8, 1), 3), 6: ((5, 7, 1), 1)}
    for NCH, (last, po) in mf.items():
        cases.append(_mk(((po, 2, 1), (po, 2, 1), last), 'mass', _kn(final='mfma'), final=Final('k_final_mfma', (1, NCH))))
        cases.append(_mk(((po, 3, 1), last), 'stiffness', _kn(final='mfma'), final=Final('k_final_mfma', (4, NCH))))
    # NCH = 7 (q above P only): the plan takes another kernel, the generic k_final
    cases.append(_mk(((6, 1, 1), (5, 7, 1)), 'mass', _kn(final='mfma'), final=Final('k_final', (6, 1, 0, 4, False))))
    cases.append(_mk(((6, 1, 1), (2, 2, 1), (4, 8, 1)), 'stiffness', _kn(final='mfma'), final=Final('k_final', (5, 4, 0, 4, False))))
    # ---- k_stageA: what the cases above leave.  Non-symmetric forms, q above P, the high degrees
    for P in range(2, 7):
        p = P - 1
        # 3D non-symmetric, q == P: two types per group (P <= 4) or ONE (P >= 5): convection-diffusion
        cases.append(_mk(((p, 3, (1, min(2, p))), (max(p - 1, 1), 2, 1), (p, 2, 1)), 'convdiff', _kn(),
                         stageA=StageA(P, P, False, P >= 5, False), stageB=StageB(max(P - 1, 2), 0 if P > 2 else 2)))
        # 2D non-symmetric, q above P: a table; k_combine
        cases.append(_mk(((p, 4, 1), (p + 1, 3, 1)), 'form', _kn(), table='diff_conv', stageA=StageA(P, 0, False, False, False)))
        # 3D symmetric, q above P, field kernels
        cases.append(_mk(((p, 3, 1), (p + 1, 2, 1), (p, 3, 1)), 'stiffness', _kn(geoa='0'), stageA=StageA(P, 0, True, False, False), stageB=StageB(P + 1, P + 1 if P < 6 else 0)))
    # 2D symmetric with the next span's field values prefetched (PF), double knots on axis 0
    cases.append(_mk(((2, 9, 2), (2, 5, 1)), 'stiffness', _kn(geoa='0'), stageA=StageA(3, 3, True, False, True)))
    cases.append(_mk(((6, 2, 1), (1, 2, 1), (2, 2, 1)), 'stiffness', _kn(), stageA=StageA(7, 0, True, False, False), stageB=StageB(2, 0)))
    cases.append(_mk(((6, 2, 2), (1, 2, 1), (1, 3, 1)), 'convdiff', _kn(), stageA=StageA(7, 7, False, True, False), stageB=StageB(2, 0)))
    cases.append(_mk(((6, 2, 1), (7, 1, 1)), 'form', _kn(), table='conv', stageA=StageA(7, 0, False, False, False)))
    cases.append(_mk(((7, 1, 1), (2, 2, 2), (1, 3, 1)), 'mass', _kn(), stageA=StageA(8, 0, True, False, False), stageB=StageB(3, 0)))
    cases.append(_mk(((7, 2, 3), (1, 2, 1), (1, 2, 1)), 'convdiff', _kn(), stageA=StageA(8, 8, False, True, False), stageB=StageB(2, 0)))
    # ---- k_stageB: the remaining (P, Q), and every NTERM at a compile-time and at a run-time q
    for P in range(3, 7):                                    # (P, 0): axis 1 below the others
        p = P - 1
        cases.append(_mk(((p + 1, 2, 1), (p, 3, 2 if P % 2 else 1), (p, 2, 1)), 'stiffness' if P % 2 else 'mass', _kn(), stageB=StageB(P, 0)))
    cases.append(_mk(((1, 2, 1), (6, 2, 1), (1, 2, 1)), 'stiffness', _kn(), stageB=StageB(7, 0)))     # the 256-thread block
    cases.append(_mk(((1, 2, 1), (7, 1, 1), (2, 2, 1)), 'mass', _kn(), stageB=StageB(8, 0)))
    for i, table in enumerate(('react', 'conv', 'react_conv', 'diff', 'diff_react', 'diff_conv', 'diff_react_conv', 'diff_conv2', 'full', 'full_sym')):
        rep = (2,) if i % 2 else 1
        cases.append(_mk(((2, 2, 1), (2, 3 if rep == 1 else 2, rep), (2, 3, 1)), 'form', _kn(), table=table, stageB=StageB(3, 3)))
        cases.append(_mk(((2, 2, 1), (1, 3, 1), (2, 2, 2)), 'form', _kn(), table=table, stageB=StageB(2, 0)))
    for table in ('diff_react', 'diff_react_conv', 'diff_conv2', 'full'):
        cases.append(_mk(((1, 2, 1), (6, 2, (3,)), (1, 2, 1)), 'form', _kn(), table=table, stageB=StageB(7, 0)))
    return cases


def _with_slabs(cases):
    """Row slabs: the first case of every final-kernel family (k_final fast / generic per NY, k_final_q, k_final_mfma) and of
    every stage-A variant (Q, SYM, ONE, PF), 2D and 3D apart."""
    seen, out = set(), []
    for c in cases:
        k = stage_keys(c.axes, c.kind, c.knobs, c.table, c.geo)
        fam = (k.final.kernel, k.final.args[-1] if k.final.kernel == 'k_final' else None, k.shape['NY'], len(c.axes))
        var = k.stageA if k.stageA == 'geoA' else (k.stageA.Q != 0, k.stageA.SYM, k.stageA.ONE, k.stageA.PF, len(c.axes))
        new = {('f',) + fam, ('a', var)} - seen
        out.append(c._replace(slabs=bool(new)))
        seen |= new
    return out


STAGE_CASES = _with_slabs(_build_cases())


# ---- the largest case: rows and nonzeros of a ledger or sweep patch stay below these.  The oracle with 8 threads takes 0.30 s
# for the largest ledger case, 3.5 s for the whole ledger and 7.0 s for the 267 sizes of the edge sweeps on the development
# machine's 8-core CPU (tools/stage_cases.py --time).
MAX_ROWS = 6000
MAX_NNZ = 1200000


def patch_size(axes):
    """(rows, nonzeros) of the patch's matrix."""
    ax = [axis_tables(a) for a in axes]
    return int(np.prod([a.N for a in ax])), int(np.prod([a.S for a in ax]))


# ---- edge sweeps: every entry is (name, function of the size -> (axes, kind, knobs, table), sizes); each size is checked
# against the oracle by test_stage_kernels_gpu.py, and test_stage_coverage_cpu.py checks that the sizes visit what is claimed
def mult_axis(p, N, m=2):
    """An axis of degree p with N dofs whose interior knots are m-fold, the last one of lower multiplicity where N asks for it."""
    inner = N - p - 1
    assert inner >= 1
    mults = (m,) * (inner // m) + ((inner % m,) if inner % m else ())
    return (p, len(mults) + 1, mults)


def exact_axis(p, n):
    """n spans with single knots at k / n (make_knots' np.arange expression gives an extra, nearly empty span for some n)."""
    return (p, n, (1,) * (n - 1)) if n > 1 else (p, 1, 1)


def _crmax(P, q):
    return max(1, min(64, CR_WINDOW // q - (P - 1)))


# k_final, rows per wave task: the last axis has crmax - 1 .. 2 crmax + 2 dofs: one chunk, two chunks, three chunks, every
# position of the last chunk's edge
FINAL_ROW_SWEEPS = [
    ('fast-p2-2d', lambda N: (((2, 2, 1), exact_axis(2, N - 2)), 'stiffness', _kn(final='valu'), None), _crmax(3, 3)),
    ('generic-p2-3d', lambda N: (((2, 1, 1), (2, 2, 2), mult_axis(2, N)), 'stiffness', _kn(final='valu'), None), _crmax(3, 3)),
]


def final_row_sizes(crmax, half=None):
    sizes = list(range(crmax - 1, 2 * crmax + 3))
    if half is None:
        return sizes
    return sizes[:len(sizes) // 2] if half == 0 else sizes[len(sizes) // 2:]


# k_final, row tiles: a tile's basis segment is tsp_max * SSTR doubles and must stay within 64 KiB
def _tile_axes(n1):
    return ((3, 4, 1), exact_axis(3, n1)), 'mass', _kn(final='valu'), None


def final_tile_sizes():
    """Spans of the last axis: the first with two and with three tiles, one span either side of each, and a short one; then the
    sizes that put the last tile's edge one row either side of a full tile."""
    first = {}
    n1 = 200
    while 3 not in first:
        nt = stage_keys(_tile_axes(n1)[0], 'mass', _kn(final='valu')).shape['ntiles']
        first.setdefault(nt, n1)
        n1 += 1
    return [first[1]] + [first[k] + d for k in (2, 3) for d in (-1, 0, 1)]


FINAL_TILE_SWEEP = ('tiles-p3-2d', _tile_axes)

# k_final_q: a wave owns R = 64 / P rows; the last axis has R - 1 .. 2 R + 1 dofs
FINALQ_SWEEPS = [
    ('p1-2d', 2, lambda N: (((1, 3, 1), exact_axis(1, N - 1)), 'stiffness', _kn(), None)),
    ('p2-3d', 3, lambda N: (((2, 1, 1), (2, 2, 2), exact_axis(2, N - 2)), 'stiffness', _kn(), None)),
    ('p5-2d', 6, lambda N: (((5, 2, 1), exact_axis(5, N - 5)), 'mass', _kn(), None)),
]


def finalq_sizes(P):
    R = 64 // P
    return list(range(R - 1, 2 * R + 2))


# ... lines per block: a launch of less than one resident round takes the per_super branch (2D), a larger one does not (3D)
FINALQ_LPW_CASES = [
    ('per_super-2d', ((3, 9, 1), (3, 70, 1)), 'stiffness', _kn(), True),
    ('rounds-3d', ((2, 18, 1), (2, 18, 1), (2, 3, 1)), 'convdiff', _kn(), False),
]

# chunked sweeps: axis 0 (stage A) or axis 1 (stage B) over 8 P - 1 .. 8 P + 2 spans and 12 P (three chunks); in 2D stage A
# chunks from 2 P spans on.  (name, which sweep, function of the spans -> (axes, kind, knobs, table), P, least chunk length / P)
def _rep_axis(p, n, double):
    return (p, n, (2 if double else 1,) * (n - 1))


CHUNK_SWEEPS = [
    ('A-stiffness-single', 'chunksA', lambda n: ((_rep_axis(2, n, False), (2, 1, 1), (2, 2, 1)), 'stiffness', _kn(geoa='0'), None), 3, 4),
    ('A-mass-double', 'chunksA', lambda n: ((_rep_axis(3, n, True), (3, 1, 1), (2, 2, 1)), 'mass', _kn(geoa='0'), None), 4, 4),
    ('A-convdiff-single', 'chunksA', lambda n: ((_rep_axis(2, n, False), (1, 2, 1), (2, 1, 1)), 'convdiff', _kn(), None), 3, 4),
    ('A-table-double', 'chunksA', lambda n: ((_rep_axis(2, n, True), (2, 1, 1), (1, 2, 1)), 'form', _kn(), 'full'), 3, 4),
    ('B-stiffness-single', 'chunksB', lambda n: (((2, 1, 1), _rep_axis(2, n, False), (2, 2, 1)), 'stiffness', _kn(), None), 3, 4),
    ('B-mass-double', 'chunksB', lambda n: (((1, 2, 1), _rep_axis(3, n, True), (3, 1, 1)), 'mass', _kn(final='valu'), None), 4, 4),
    ('B-convdiff-double', 'chunksB', lambda n: (((2, 1, 1), _rep_axis(2, n, True), (2, 1, 2)), 'convdiff', _kn(), None), 3, 4),
    ('B-table-single', 'chunksB', lambda n: (((1, 2, 1), _rep_axis(2, n, False), (2, 1, 1)), 'form', _kn(), 'diff_react_conv'), 3, 4),
    ('A2d-stiffness-PF', 'chunksA', lambda n: ((_rep_axis(2, n, False), (2, 3, 1)), 'stiffness', _kn(geoa='0'), None), 3, 1),
    ('A2d-mass-PF-double', 'chunksA', lambda n: ((_rep_axis(3, n, True), (3, 2, 1)), 'mass', _kn(geoa='0'), None), 4, 1),
]


def chunk_sweep_sizes(P, factor):
    m = 2 * factor * P
    return [m - 1, m, m + 1, m + 2, 3 * factor * P]


def sweep_patches():
    """Every (tag, axes, kind, knobs, table) of the edge sweeps."""
    out = []
    for name, fn, crmax in FINAL_ROW_SWEEPS:
        out += [(('rows', name, N),) + fn(N) for N in final_row_sizes(crmax)]
    out += [(('tiles', n1),) + FINAL_TILE_SWEEP[1](n1) for n1 in final_tile_sizes()]
    for name, P, fn in FINALQ_SWEEPS:
        out += [(('finalq', name, N),) + fn(N) for N in finalq_sizes(P)]
    out += [(('lpw', name), axes, kind, knobs, None) for name, axes, kind, knobs, _ in FINALQ_LPW_CASES]
    for name, _, fn, P, factor in CHUNK_SWEEPS:
        out += [(('chunks', name, n),) + fn(n) for n in chunk_sweep_sizes(P, factor)]
    return out

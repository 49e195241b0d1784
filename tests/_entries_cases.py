"""The cases that run every instantiation and launch edge of the entry-wise and pattern kernels
(pyiga_amd/csrc/kern_entries.hip), and the dispatch that decides which kernel a request reaches, restated.

A plain helper module (no GPU, no library load).  tests/test_entries_coverage_cpu.py ties the tables below to the source and
checks on the host that the cases reach what they claim; tests/test_entries_kernels_gpu.py runs them against the long-double
model of tests/_entries_model.py.

A case: knot vectors as (degree, spans, interior multiplicity) per axis, geometry, kinds ('mass', 'stiffness', 'convdiff',
'form_phys': IGX_FORM with a physical table that has all four blocks, 'form_par': IGX_FORM with a set_pform form), an optional
row slab `row0` or span box `bbox`, an optional `nqp`, and how its index pairs are drawn (``picks``, seeded by the case id):

- `nrand` pattern pairs (a random row, a random column of that row; for a slab or a box every other row is one whose support lies
  inside the resident window, so that enough picks have a value); with `top1` both axis-1 indices are taken from the last
  `top1` dofs of axis 1 (at degree 15 the product of two functions at the last Gauss point of the overlap is below rounding
  unless both are among the last: the mutation test needs picks that can see that point),
- axis sweeps: for every axis the coupled index pairs of that axis (at most SWEEP_CAP of them, drawn), the other axes at the
  centre dof: every overlap length, every face of a slab or box,
- the first and the last dof with themselves,
- pairs outside the pattern, and indices at and past prod(N),
- more pattern pairs until M % 4 == 1 (so M % 128 != 0): with ``request_lengths`` every case asks for M, M - 3, M - 2 and 1
  entries: M % 4 = 1, 2, 3 on the wave kernel, ragged last blocks of 128 on the thread kernel, and a single entry.
"""
import os
import re
import zlib
from typing import NamedTuple, Optional

import numpy as np

import _entries_model as em

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERN_ENTRIES_HIP = os.path.join(ROOT, 'pyiga_amd', 'csrc', 'kern_entries.hip')
CSRC = os.path.join(ROOT, 'pyiga_amd', 'csrc')
IGX_H = os.path.join(ROOT, 'include', 'igx.h')

# ---------------------------------------------------------------------------------------------
# kern_entries.hip, restated (test_entries_coverage_cpu.py reads the source and compares)
IGX_MAX_DEGREE = 15
DISPATCH_RULE = 'kind != IGX_FORM && pmax >= 2 && !pt->knobs.entries_thread && M < (1ull << 25)'
WAVE_M_LIMIT = 1 << 25
LIST_BLOCK = 128
WAVE_BLOCK = 256
WAVE_ENTRIES_PER_BLOCK = 4           # 256 threads / 64 lanes
WAVE_LANES = 64
CSR_BLOCK = 128
PATTERN_BLOCK = 256
LIST_INSTANCES = {(2, 'MASS'), (2, 'FORM'), (2, 'STIFFNESS'), (3, 'MASS'), (3, 'CONVDIFF'), (3, 'FORM'), (3, 'STIFFNESS')}
WAVE_INSTANCES = {(2, 'MASS'), (2, 'STIFFNESS'), (3, 'MASS'), (3, 'CONVDIFF'), (3, 'STIFFNESS')}
CSR_INSTANCES = set(LIST_INSTANCES)
PATTERN_INSTANCES = {2, 3}
KIND_ENUM = {'mass': 'MASS', 'stiffness': 'STIFFNESS', 'convdiff': 'CONVDIFF', 'form_phys': 'FORM', 'form_par': 'FORM'}
SYMMETRIC = {'mass', 'stiffness'}    # launch_entries_csr: lower triangle + mirror; every other kind: each entry of the owned rows


def wave_runs(kind, degrees, thread, M):
    """launch_entries_list's condition."""
    return KIND_ENUM[kind] != 'FORM' and max(degrees) >= 2 and not thread and M < WAVE_M_LIMIT


def entries_kernel(case, kind, thread, M):
    dim, k = len(case.axes), KIND_ENUM[kind]
    fam = 'wave' if wave_runs(kind, [a[0] for a in case.axes], thread, M) else 'list'
    inst = (dim, k)
    assert inst in (WAVE_INSTANCES if fam == 'wave' else LIST_INSTANCES), (case.id, kind, fam)
    return fam, inst


def kernel_name(fam, inst):
    return 'k_entries_%s<%d, IGX_%s>' % (fam, inst[0], inst[1])


def request_lengths(M):
    return (M, M - 3, M - 2, 1)


SWEEP_CAP = 40
N_OUTSIDE = 12


class Case(NamedTuple):
    id: str
    axes: tuple                      # (degree, spans, interior multiplicity) per axis
    geo: str                         # 'annulus' (2D), 'cylinder' | 'twisted' (3D)
    kinds: tuple
    nrand: int
    row0: Optional[tuple] = None
    bbox: Optional[tuple] = None
    nqp: Optional[int] = None
    top1: Optional[int] = None
    assemble: bool = True            # also through assemble(kind, algo='entrywise') and pattern()

    @property
    def dim(self):
        return len(self.axes)

    def q(self):
        return self.nqp or max(a[0] for a in self.axes) + 1

    def kvs(self):
        from pyiga_amd import bspline
        return tuple(bspline.make_knots(p, 0.0, 1.0, n, mult=m) for p, n, m in self.axes)

    def tables(self):
        """Integer bookkeeping of every axis (no basis values)."""
        return [em.axis_table(kv, self.q()) for kv in self.kvs()]

    def window(self):
        ax = self.tables()
        if self.row0 is not None:
            return em.slab_window(ax, self.row0)
        if self.bbox is not None:
            return em.box_window(ax, self.bbox)
        return em.whole_window(ax)


ALL2 = ('mass', 'stiffness', 'form_phys', 'form_par')
ALL3 = ('mass', 'stiffness', 'convdiff', 'form_phys', 'form_par')
FIX2 = ('mass', 'stiffness')
FIX3 = ('mass', 'stiffness', 'convdiff')

CASES = (
    # all p = 1: the rule sends every kind to k_entries_list
    Case('p1_2d', ((1, 5, 1), (1, 4, 1)), 'annulus', ALL2, 60),
    Case('p1_3d', ((1, 3, 1), (1, 4, 1), (1, 3, 1)), 'cylinder', ALL3, 60),
    # p >= 2: the five wave instantiations; with IGX_ENTRIES=thread the list ones; FORM stays on the list kernel
    Case('p3_2d_nqp17', ((3, 5, 1), (3, 6, 1)), 'annulus', ALL2, 80, nqp=17),          # boxes of 17, 34, 51, 68 points
    Case('p3_3d', ((3, 5, 1), (3, 5, 1), (3, 5, 1)), 'cylinder', ALL3, 80),            # boxes of 16 .. 256 points, 64 among them
    Case('p4_3d', ((4, 6, 1), (4, 6, 1), (4, 6, 1)), 'twisted', FIX2, 40),             # 2p + 2 dofs per axis: full interior rows
    # degrees 8 .. 15
    Case('p15_2d', ((15, 2, 1), (15, 2, 1)), 'annulus', FIX2, 60, top1=3),
    Case('p8_3_2d', ((8, 3, 1), (3, 5, 1)), 'annulus', FIX2 + ('form_phys',), 60),
    Case('p15_2_1_3d', ((15, 1, 1), (2, 3, 1), (1, 4, 1)), 'cylinder', FIX3, 30),      # and a two-function axis under the wave kernel
    Case('mixed_3d', ((2, 4, 1), (1, 3, 1), (3, 5, 1)), 'twisted', FIX3 + ('form_par',), 60),
    # repeated interior knots: axis 0, the last axis, multiplicity p (C^0)
    Case('rep_ax0_2d', ((3, 5, 2), (2, 4, 1)), 'annulus', FIX2 + ('form_phys',), 60),
    Case('rep_last_3d', ((2, 3, 1), (2, 3, 1), (2, 4, 2)), 'cylinder', FIX3, 60),
    Case('c0_2d', ((2, 4, 1), (3, 4, 3)), 'annulus', FIX2, 60),
    # row slabs, row0 strictly inside; a slab of one plane
    Case('slab_2d', ((3, 10, 1), (2, 5, 1)), 'annulus', ALL2, 60, row0=(5, 8)),
    Case('slab_3d', ((2, 7, 1), (2, 3, 1), (1, 3, 1)), 'cylinder', ALL3, 60, row0=(3, 5)),
    Case('slab1_2d', ((2, 6, 1), (2, 4, 2)), 'annulus', FIX2, 40, row0=(4, 5)),
    # span boxes (batched entries only; set_pform refuses them)
    Case('box_2d', ((2, 7, 1), (3, 8, 1)), 'annulus', FIX2 + ('form_phys',), 80, bbox=((2, 5), (2, 6)), assemble=False),
    Case('box_3d', ((2, 6, 1), (2, 6, 1), (2, 6, 1)), 'cylinder', FIX3 + ('form_phys',), 80, bbox=((1, 4), (2, 5), (2, 5)), assemble=False),
    # degree 0 on one axis
    Case('p0_2d', ((0, 4, 1), (2, 4, 1)), 'annulus', ('mass',), 40),
)
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

# fast_assemble(kind, batch >= S0 * S1): k_box_pairs feeding the entries kernel (2D mixed degrees / repeated knots)
BOX_PAIR_CASES = ('p8_3_2d', 'rep_ax0_2d', 'c0_2d')
# the axes whose basis tables are compared with the long-double recursion
HIGH_DEGREE_AXES = ((8, 3, 1), (15, 2, 1), (15, 1, 1), (11, 2, 2), (13, 3, 1))
# how far the oracle's double-precision active_deriv lies from the long-double run of the same recursion at the p + 1 Gauss nodes
# per span of these axes: max |double - long double| / max |long double| per derivative order 0, 1, 2, in units of 2**-53,
# measured on the host and rounded up (test_entries_coverage_cpu.py measures again).  The device gets 4 times that.
ORACLE_TABLE_DEVIATION = {
    (8, 3, 1): (8.2, 8.6, 8.9), (15, 2, 1): (3.5, 3.4, 3.4), (15, 1, 1): (3.4, 3.4, 2.3), (11, 2, 2): (7.2, 6.8, 5.8),
    (13, 3, 1): (8.7, 10.0, 8.6),
}
TABLE_FACTOR = 4


# ---------------------------------------------------------------------------------------------
def picks(case):
    """(M, 2) int64 index pairs; deterministic."""
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    ax = case.tables()
    Ns = [a.N for a in ax]
    Ntot = int(np.prod(Ns))

    def ravel(i):
        return int(np.ravel_multi_index(i, Ns))

    w = case.window()
    wspans = [(b // a.q, (b + L) // a.q) for a, (b, L) in zip(ax, ((w.g0, w.G0), (w.b1, w.L1), (w.b2, w.L2)))]
    inside = [np.flatnonzero((a.mslo >= lo) & (a.mshi <= hi)) for a, (lo, hi) in zip(ax, wspans)]

    def random_pattern_pair():
        i = [int(rng.integers(0, N)) for N in Ns]
        if (case.row0 or case.bbox) and rng.random() < 0.5:          # a row whose support lies inside the resident window
            i = [int(rng.choice(ins)) for ins in inside]
        if case.top1:
            i[1] = int(rng.integers(Ns[1] - case.top1, Ns[1]))
        j = [int(rng.integers(a.jlo[ik], a.jhi[ik])) for a, ik in zip(ax, i)]
        if case.top1:
            j[1] = int(rng.integers(Ns[1] - case.top1, Ns[1]))
        return ravel(i), ravel(j)

    out = [random_pattern_pair() for _ in range(case.nrand)]
    centre = [N // 2 for N in Ns]
    for k, a in enumerate(ax):
        pairs = [(ik, jk) for ik in range(a.N) for jk in range(a.jlo[ik], a.jhi[ik])]
        if len(pairs) > SWEEP_CAP:
            pairs = [pairs[t] for t in sorted(rng.choice(len(pairs), SWEEP_CAP, replace=False))]
        for ik, jk in pairs:
            i, j = list(centre), list(centre)
            i[k], j[k] = ik, jk
            out.append((ravel(i), ravel(j)))
    out += [(0, 0), (Ntot - 1, Ntot - 1)]
    n_out = 0
    while n_out < N_OUTSIDE:
        I, J = int(rng.integers(0, Ntot)), int(rng.integers(0, Ntot))
        if em.overlap(ax, I, J) is None:
            out.append((I, J))
            n_out += 1
    out += [(Ntot, 0), (0, Ntot), (Ntot + 5, Ntot + 7), (1 << 40, 1)]
    while len(out) % 4 != 1:
        out.append(random_pattern_pair())
    return np.array(out, dtype=np.int64)


# ---------------------------------------------------------------------------------------------
# coefficients of the forms: smooth arrays over the Gauss nodes, nothing special about them
def coef_array(r, s, nodes):
    """Coefficient (r, s) on the tensor grid of `nodes` (one array per axis)."""
    X = np.meshgrid(*nodes, indexing='ij')
    ph = sum((k + 1) * x for k, x in enumerate(X))
    return (1.0 if r == s else 0.0) + 0.3 * r - 0.2 * s + 0.5 * np.sin(1.0 + r + 2 * s + 3.0 * ph)


def phys_present(dim):
    """A table with all four blocks (value/value, value/derivative, derivative/value, derivative/derivative), not full."""
    pres = {(0, 0), (0, 1), (dim, 0)} | {(r, r) for r in range(1, dim + 1)} | {(1, dim)}
    return sorted(pres)


def phys_table(dim, nodes):
    t = [[None] * 4 for _ in range(4)]
    for r, s in phys_present(dim):
        t[r][s] = coef_array(r, s, nodes)
    return t


def par_masks(dim):
    """(mask of v, mask of u) over the grid axes: value/value, every single axis, mixed and repeated masks."""
    full = (1 << dim) - 1
    return [(0, 0), (1, 1), (full, 0), (2, 1), (1 << (dim - 1), 1 << (dim - 1)), (full, full), (0, 2)]


def par_terms(dim, nodes):
    return [(mv, mu, coef_array(mv, mu, nodes)) for mv, mu in par_masks(dim)]


def form_of(case, kind):
    """The `form` argument of the model's terms_of / c_kind."""
    if kind == 'form_phys':
        return ('phys', em.physical_form_ab(case.dim, phys_present(case.dim)))
    if kind == 'form_par':
        return ('par', par_masks(case.dim))
    return None


def model_kind(kind):
    return 'form' if kind.startswith('form') else kind


# ---------------------------------------------------------------------------------------------
# the source
def read_source(path=KERN_ENTRIES_HIP):
    with open(path) as f:
        return f.read()


def function_body(src, name):
    """Text of the top-level function `name` (from its header to the closing brace at column 0)."""
    m = re.search(r'^int %s\(.*?^\}' % re.escape(name), src, re.S | re.M)
    assert m, name
    return m.group(0)


_INST = re.compile(r'\b(k_entries_list|k_entries_wave|k_entries_csr)<\s*(\d)\s*,\s*IGX_(\w+)\s*><<<')
_PAT = re.compile(r'\bk_pattern<\s*(\d)\s*><<<')


def parse_instances(src):
    """{'list' | 'wave' | 'csr': set of (dim, kind), 'pattern': set of dim} named in the three launch functions."""
    out = {'list': set(), 'wave': set(), 'csr': set(), 'pattern': set()}
    for fn, fams in (('launch_entries_list', ('list', 'wave')), ('launch_entries_csr', ('csr',))):
        for name, dim, kind in _INST.findall(function_body(src, fn)):
            fam = name[len('k_entries_'):]
            assert fam in fams, (fn, name)
            out[fam].add((int(dim), kind))
    out['pattern'] = {int(d) for d in _PAT.findall(function_body(src, 'launch_pattern'))}
    return out


def instances_outside_launchers():
    """Instantiations of the entry and pattern kernels named anywhere in csrc/ outside the three launch functions."""
    found = []
    name = re.compile(r'\b(k_entries_list|k_entries_wave|k_entries_csr|k_pattern)\s*<[^<>;(){}]*>\s*(<<<|\)|,|;)')
    for fn in sorted(os.listdir(CSRC)):
        if not fn.endswith(('.hip', '.h', '.cpp', '.hpp')):
            continue
        text = read_source(os.path.join(CSRC, fn))
        if fn == 'kern_entries.hip':
            for f in ('launch_entries_list', 'launch_entries_csr', 'launch_pattern'):
                text = text.replace(function_body(text, f), '')
        found += [(fn, m.group(0)) for m in name.finditer(text)]
    return found


def parse_dispatch_rule(src):
    """The condition of the first `if` after pmax is computed in launch_entries_list, whitespace-normalised."""
    body = function_body(src, 'launch_entries_list')
    at = body.index('pmax = std::max')
    at = body.index('if (', at)
    depth, k = 0, at + 3
    while True:
        depth += body[k] == '('
        depth -= body[k] == ')'
        if depth == 0:
            break
        k += 1
    return ' '.join(body[at + 4:k].split())


def parse_constants(src):
    lst = function_body(src, 'launch_entries_list')
    csr = function_body(src, 'launch_entries_csr')
    pat = function_body(src, 'launch_pattern')
    wave = src[src.index('k_entries_wave(PatchDev'):src.index('k_box_pairs(PatchDev')]
    header = read_source(IGX_H)
    return {
        'LIST_BLOCK': int(re.search(r'\(M \+ 127\) / 128\)\), block\((\d+)\)', lst).group(1)),
        'WAVE_BLOCK': int(re.search(r'blockw\((\d+)\)', lst).group(1)),
        'WAVE_ENTRIES_PER_BLOCK': int(re.search(r'gridw\(\(unsigned\)\(\(M \+ 3\) / (\d+)\)\)', lst).group(1)),
        'WAVE_LANES': 1 << int(re.search(r'threadIdx\.x\) >> (\d+);', wave).group(1)),
        'WAVE_LANE_STRIDE': int(re.search(r'idx < nbox; idx \+= (\d+)\)', wave).group(1)),
        'WAVE_LAUNCH_BOUNDS': int(re.search(r'__launch_bounds__\((\d+)\) k_entries_wave', src).group(1)),
        'CSR_BLOCK': int(re.search(r'\(total \+ 127\) / 128\)\), block\((\d+)\)', csr).group(1)),
        'PATTERN_BLOCK': int(re.search(r'\(total \+ 255\) / 256\)\), block\((\d+)\)', pat).group(1)),
        'IGX_MAX_DEGREE': int(re.search(r'#define IGX_MAX_DEGREE (\d+)', header).group(1)),
    }


EXPECTED_CONSTANTS = {
    'LIST_BLOCK': LIST_BLOCK, 'WAVE_BLOCK': WAVE_BLOCK, 'WAVE_ENTRIES_PER_BLOCK': WAVE_ENTRIES_PER_BLOCK, 'WAVE_LANES': WAVE_LANES,
    'WAVE_LANE_STRIDE': WAVE_LANES, 'WAVE_LAUNCH_BOUNDS': WAVE_BLOCK, 'CSR_BLOCK': CSR_BLOCK, 'PATTERN_BLOCK': PATTERN_BLOCK,
    'IGX_MAX_DEGREE': IGX_MAX_DEGREE,
}

"""The cases that drive every kernel of pyiga_amd/csrc/multipatch.hip, and the constants that decide them.

A plain helper module (no GPU needed to import it).  igx_multipatch_create takes arbitrary int32 maps, so every situation of
the pattern build and of the scatter is put on the device with tiny patches and hand-made maps; tests/_multipatch_model.py
gives the exact answer.  tests/test_multipatch_coverage_cpu.py checks on the host that the table reaches what it is meant to
reach, tests/test_multipatch_kernels_gpu.py runs it.

A case is a list of patches ((degree, spans, multiplicity) per axis), one map per patch and ``nglobal``.  Every map is built
deterministically from a seed derived from the case id.
"""
import os
import re
import zlib
from typing import NamedTuple

import numpy as np

import _solver_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, 'pyiga_amd', 'csrc', 'multipatch.hip')

# constants of multipatch.hip (test_multipatch_coverage_cpu.py reads them from the source and compares)
WAVE = 64
SORT_TILE = 1024
SCAN_BLOCK = 256
SCAN_ITEMS = 4
SCAN_TILE = SCAN_BLOCK * SCAN_ITEMS
SCAN_CHUNK = SCAN_BLOCK * SCAN_TILE            # inputs one trip of k_scan_sums covers
CONSTS = dict(WAVE=WAVE, SORT_TILE=SORT_TILE, SCAN_BLOCK=SCAN_BLOCK, SCAN_ITEMS=SCAN_ITEMS)

KERNELS = ('k_scan_tiles', 'k_scan_sums', 'k_scan_add', 'k_count', 'k_fill', 'k_sort_rows', 'k_sort_long',
           'k_compact', 'k_positions', 'k_compact_pos', 'k_scatter', 'k_scatter_vec')

# the raw row lengths of the ladder: 2^k - 1, 2^k, 2^k + 1 up to the switch to k_sort_long, and one row past twice the tile
LADDER_LENGTHS = (4,) + tuple(2 ** k + d for k in range(6, 11) for d in (-1, 0, 1)) + (2 * SORT_TILE + 4,)


def read_source():
    with open(SOURCE) as f:
        return f.read()


def parse_constants(src):
    out = {}
    for name in ('WAVE', 'SORT_TILE', 'SCAN_BLOCK', 'SCAN_ITEMS'):
        m = re.search(r'constexpr int (?:[A-Z_]+ = \d+, )*%s = (\d+)[;,]' % name, src)
        out[name] = int(m.group(1)) if m else None
    return out


def parse_scan_tile(src):
    """The right-hand side of SCAN_TILE."""
    m = re.search(r'\bSCAN_TILE = ([A-Z_ *]+);', src)
    return m.group(1).strip() if m else None


def parse_kernels(src):
    return tuple(re.findall(r'__global__ void (?:__launch_bounds__\(\w+\) )?(k_\w+)\(', src))


def seed_of(case_id):
    return zlib.crc32(case_id.encode())


class Case(NamedTuple):
    id: str
    patches: tuple        # per patch: ((p, n, mult) per axis)
    l2g: tuple            # per patch: int32 array
    nglobal: int
    rows: bool = True     # small enough for the row-by-row staged build of the model

    def kvs(self, p):
        from pyiga_amd import bspline
        return tuple(bspline.make_knots(d, 0.0, 1.0, n, mult=m) for d, n, m in self.patches[p])

    def patterns(self):
        return [sc.patch_pattern(self.kvs(p)) for p in range(len(self.patches))]

    def ndofs(self, p):
        return int(np.prod([n * m + d + 1 - m for d, n, m in self.patches[p]]))


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _row_lengths(axes):
    from pyiga_amd import bspline
    kvs = tuple(bspline.make_knots(d, 0.0, 1.0, n, mult=m) for d, n, m in axes)
    return np.diff(sc.patch_pattern(kvs).indptr)


# ---------------------------------------------------------------------------------------------
def ladder():
    """One 40 x 40-dof degree-1 patch (rows of 4, 6 and 9 entries) and three 2 x 2-dof patches (rows of 4): for every target
    length, local rows whose lengths add up to it go to one global row.  All other dofs go through a random permutation; global
    rows 0, G - 1 and a few in the middle stay unreached.  Not injective."""
    rng = np.random.default_rng(seed_of('ladder'))
    patches = (((1, 39, 1), (1, 39, 1)),) + 3 * (((1, 1, 1), (1, 1, 1)),)
    lens = [_row_lengths(ax) for ax in patches]
    pool = {4: [], 6: [], 9: []}                   # (patch, local row) by row length, in random order
    for p, ln in enumerate(lens):
        for i in rng.permutation(ln.size):
            pool[int(ln[i])].append((p, int(i)))
    chosen = []                                    # per target: its (patch, row) list
    for L in LADDER_LENGTHS:
        a = {0: 0, 1: 1, 2: 2}[L % 3]              # rows of 4: L = 4 a mod 3
        rest = L - 4 * a
        b = 0 if rest % 9 == 0 else next(b for b in range(1, 4) if (rest - 6 * b) % 9 == 0 and rest >= 6 * b)
        c = (rest - 6 * b) // 9
        assert 4 * a + 6 * b + 9 * c == L
        chosen.append([pool[4].pop() for _ in range(a)] + [pool[6].pop() for _ in range(b)] + [pool[9].pop() for _ in range(c)])
    nfree = sum(ln.size for ln in lens) - sum(len(c) for c in chosen)
    n_unreached_mid = 5
    G = len(chosen) + nfree + 2 + n_unreached_mid
    ids = rng.permutation(np.arange(1, G - 1))     # rows 0 and G - 1 stay unreached, and the last n_unreached_mid of `ids`
    maps = [np.full(ln.size, -1, dtype=np.int64) for ln in lens]
    k = 0
    for rows in chosen:
        for p, i in rows:
            maps[p][i] = ids[k]
        k += 1
    for m in maps:
        free = np.flatnonzero(m < 0)
        m[free] = ids[k:k + free.size]
        k += free.size
    assert k == ids.size - n_unreached_mid
    return Case('ladder', patches, tuple(_i32(m) for m in maps), G)


def all_dup():
    """A 2 x 2-dof patch with every dof on global dof 0: one row of 16 raw entries, one unique column, G = 1."""
    return Case('all_dup', (((1, 1, 1), (1, 1, 1)),), (_i32(np.zeros(4)),), 1)


def dup_free_multi():
    """A row with contrib > 1 whose raw entries are as distinct as a patch pattern allows.  Every local row holds its own
    diagonal, so two local rows on one global row always share that one column; the rows chosen here (far apart in an 8 x 8
    degree-1 patch) share nothing else: 18 raw entries, 17 unique."""
    n = 64
    rng = np.random.default_rng(seed_of('dup_free_multi'))
    a, b = 1 * 8 + 1, 5 * 8 + 5
    m = np.empty(n, dtype=np.int64)
    others = np.setdiff1d(np.arange(n), [a, b])
    m[others] = rng.permutation(n - 2) + 1
    m[a] = m[b] = 0
    return Case('dup_free_multi', (((1, 7, 1), (1, 7, 1)),), (_i32(m),), n - 1)


def _rotated_partly_permuted(n, G, rng):
    """An injective map of n dofs into G > n: a monotone embedding with gaps of the rotated numbering (rows away from the cut
    keep increasing columns and move by a non-zero delta), then the images of the first eighth of the dofs permuted among
    themselves (the rows that see one of them, or both sides of the cut, have their columns out of order)."""
    img = np.sort(rng.choice(G, size=n, replace=False))
    shift = n // 3 + 1
    m = img[(np.arange(n) + shift) % n]
    m[:n // 8] = rng.permutation(m[:n // 8])
    return m


def permuted_2d(deg):
    cid = 'permuted_2d_p%d' % deg
    rng = np.random.default_rng(seed_of(cid))
    axes = ((deg, 20, 1), (deg, 7, 1))
    n = (20 + deg) * (7 + deg)
    G = n + n // 4
    return Case(cid, (axes,), (_i32(_rotated_partly_permuted(n, G, rng)),), G)


P5 = ((5, 6, 1),) * 3                              # 11^3 = 1331 dofs, 753 571 nonzeros, 25 rows of 1331 > SORT_TILE entries


def p5_3d_identity():
    return Case('p5_3d_identity', (P5,), (_i32(np.arange(1331)),), 1331)


def p5_3d_permuted():
    rng = np.random.default_rng(seed_of('p5_3d_permuted'))
    return Case('p5_3d_permuted', (P5,), (_i32(rng.permutation(1331)),), 1331)


def p5_3d_two_cubes():
    """Two degree-5 cubes glued on a face with the reference's numbering: interface rows of 2 x 726 raw entries (1331 unique,
    RMW), long STORE rows next to the interface and long DIRECT rows inside."""
    MP = sc.two_cubes(5, 6)
    maps = tuple(_i32(MP.patch_to_global_idx(p)) for p in range(2))
    return Case('p5_3d_two_cubes', (P5, P5), maps, int(MP.numdofs))


def many_patches(where):
    """Nine 3 x 3-dof patches (degree 1 on 2 spans and degree 2 on 1 span, alternating) with injective maps: local dof 0 of
    every patch is one global dof (contrib 9), local dof 4 of patches 0-2 another (contrib 3), local dof 8 of patches 3-4 a
    third (contrib 2); all other dofs are private.  `where`: the three shared dofs are numbered in the 'middle' of the range
    (no tail: zero_from == 0) or 'last' (zero_from > 0)."""
    cid = 'many_patches_' + where
    rng = np.random.default_rng(seed_of(cid))
    npatch = 9
    patches = tuple((((1, 2, 1),) * 2 if p % 2 == 0 else ((2, 1, 1),) * 2) for p in range(npatch))
    nprivate = 9 * npatch - (9 + 3 + 2)
    G = nprivate + 3
    shared = np.arange(G - 3, G) if where == 'last' else np.array([G // 2 - 4, G // 2, G // 2 + 5])
    private = rng.permutation(np.setdiff1d(np.arange(G), shared))
    maps, k = [], 0
    for p in range(npatch):
        m = np.full(9, -1, dtype=np.int64)
        m[0] = shared[0]
        if p < 3:
            m[4] = shared[1]
        if p in (3, 4):
            m[8] = shared[2]
        free = np.flatnonzero(m < 0)
        m[free] = private[k:k + free.size]
        k += free.size
        maps.append(_i32(m))
    assert k == nprivate
    return Case(cid, patches, tuple(maps), G)


def scan_nglobal(G):
    """One 5 x 7-dof patch spread over [0, G), first and last row included, in random order."""
    cid = 'scan_nglobal_%d' % G
    rng = np.random.default_rng(seed_of(cid))
    axes = ((1, 4, 1), (2, 5, 1))
    n = 35
    img = np.concatenate(([0, G - 1], rng.choice(np.arange(1, G - 1), size=n - 2, replace=False)))
    return Case(cid, (axes,), (_i32(rng.permutation(img)),), G)


def scan_big():
    """One degree-1 patch of 513 x 513 = 263 169 > SCAN_CHUNK dofs under an injective random map into a slightly larger range:
    the scans of the raw and unique row lengths (G inputs) and of the position-array lengths (n inputs) take the second trip
    of k_scan_sums with non-zero inputs in every tile."""
    rng = np.random.default_rng(seed_of('scan_big'))
    n = 513 * 513
    G = n + 41
    m = rng.permutation(G)[:n]
    return Case('scan_big', (((1, 512, 1), (1, 512, 1)),), (_i32(m),), G, rows=False)


def non_injective_mix():
    """Patch 0 (degree 1, 5 x 5 dofs) injective; patch 1 (degree 4, 9 x 9 dofs, rows of up to 81 entries) shares the first five
    dofs of its first column with patch 0's last column and is otherwise numbered in its own order, except that dof (2, 3)
    goes where dof (2, 2) goes (two neighbouring columns of one local row on one global column: row (6, 6), reached once,
    keeps non-decreasing but not increasing columns) and dof (8, 1) where dof (0, 2) goes.  The images of (2, 3) and (8, 1)
    stay unreached."""
    n0, n1 = 25, 81
    m0 = np.arange(n0)
    m1 = n0 + np.arange(n1)
    for i in range(5):
        m1[i * 9] = m0[i * 5 + 4]
    m1[2 * 9 + 3] = m1[2 * 9 + 2]
    m1[8 * 9 + 1] = m1[0 * 9 + 2]
    return Case('non_injective_mix', (((1, 4, 1), (1, 4, 1)), ((4, 5, 1), (4, 5, 1))), (_i32(m0), _i32(m1)), n0 + n1)


BUILDERS = {
    'ladder': ladder,
    'all_dup': all_dup,
    'dup_free_multi': dup_free_multi,
    'permuted_2d_p4': lambda: permuted_2d(4),
    'permuted_2d_p1': lambda: permuted_2d(1),
    'p5_3d_identity': p5_3d_identity,
    'p5_3d_permuted': p5_3d_permuted,
    'p5_3d_two_cubes': p5_3d_two_cubes,
    'many_patches_middle': lambda: many_patches('middle'),
    'many_patches_last': lambda: many_patches('last'),
    'scan_nglobal_%d' % (SCAN_TILE - 1): lambda: scan_nglobal(SCAN_TILE - 1),
    'scan_nglobal_%d' % SCAN_TILE: lambda: scan_nglobal(SCAN_TILE),
    'scan_nglobal_%d' % (SCAN_TILE + 1): lambda: scan_nglobal(SCAN_TILE + 1),
    'scan_big': scan_big,
    'non_injective_mix': non_injective_mix,
}
CASE_IDS = tuple(BUILDERS)

_cache = {}


def case(cid):
    if cid not in _cache:
        c = BUILDERS[cid]()
        assert c.id == cid
        _cache[cid] = c
    return _cache[cid]


_models = {}


def model(cid):
    """The host model of a case, computed once and shared (read-only) by the tests."""
    import _multipatch_model as mm
    if cid not in _models:
        c = case(cid)
        _models[cid] = mm.Model(c.patterns(), c.l2g, c.nglobal)
    return _models[cid]


def values(cid, what, integer=False, scale=1.0):
    """Deterministic values per patch: 'mat' (one per local nonzero) or 'vec' (one per local dof).  Real values have mixed signs
    and magnitudes over six decades; integer ones are small signed integers (their sums are exact in any order)."""
    c = case(cid)
    M = model(cid)
    rng = np.random.default_rng(seed_of('%s/%s/%d/%r' % (cid, what, integer, scale)))
    out = []
    for p in range(len(c.patches)):
        n = M.lindices[p].size if what == 'mat' else M.l2g[p].size
        if integer:
            v = rng.integers(-1000, 1001, size=n).astype(np.float64)
        else:
            v = rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, size=n)
        out.append(np.ascontiguousarray(v * scale))
    return out

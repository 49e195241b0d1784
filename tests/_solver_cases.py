"""The cases that run every SpMV instantiation of the device solvers (pyiga_amd/csrc/solve.hip), and what decides them.

A plain helper module (no GPU needed to import it): tests/test_solver_coverage_cpu.py checks on the host that the table reaches
every group width of k_spmv and k_csr_spmv and wraps every grid-stride loop, tests/test_solver_kernels_gpu.py runs the cases.

- ``spmv_gw(maxlen)``: the restatement of solve.hip's group width (lanes per row) from the longest row.
- ``patch_maxlen(kvs)``: the longest row of a patch's structured layout, the product over axes of ``max_i (jhi - jlo)``, as
  igx_solver_create computes it (jlo / jhi: the first and one past the last basis function whose support overlaps that of
  basis function i; igx_api.hip).
- ``multipatch_pattern(MP)``: the global pattern ``sum_p X_p A_p X_p^T`` of a finalized Multipatch, built on the host from the
  per-axis patterns; its longest row is what igx_solver_create_multipatch passes to spmv_gw.
- ``spmv_pass_rows(gw)`` / ``vec_pass_rows()``: a case wraps the SpMV loop only with more rows than NB_SPMV_MAX blocks of
  BLOCK / GW rows hold, the vector kernels only with more than NB_VEC blocks of BLOCK threads.  These bounds hold at any
  occupancy (the solver's grid is min(NB_SPMV_MAX, per_cu x ncu) blocks): past them the loops take two passes or more.
"""
import os
import re
from typing import NamedTuple

import numpy as np
import scipy.sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the solver source: the internal header, then the units of the linear solvers, the time stepping and the eigen-solver
SOLVE_SOURCES = tuple(os.path.join(ROOT, 'pyiga_amd', 'csrc', fn)
                      for fn in ('solve_internal.h', 'solve.hip', 'solve_step.hip', 'solve_eig.hip'))

# constants of solve_internal.h (test_solver_coverage_cpu.py reads them from the source and compares)
BLOCK = 256
NB_VEC = 1024
NB_SPMV_MAX = 8192
GW_THRESHOLDS = ((192, 64), (96, 32), (48, 16), (24, 8))      # maxlen >= t -> gw, else 4
GWS = (4, 8, 16, 32, 64)
# the (GW, U) instantiations of k_spmv and k_csr_spmv
SPMV_INSTANCES = {(64, 12), (32, 4), (16, 4), (8, 4), (4, 4)}
CSR_SPMV_INSTANCES = {(64, 8), (32, 4), (16, 4), (8, 4), (4, 4)}


def spmv_gw(maxlen):
    for t, gw in GW_THRESHOLDS:
        if maxlen >= t:
            return gw
    return 4


def spmv_pass_rows(gw):
    """Rows one grid-stride pass of the SpMV covers at the largest grid: more rows than this always take a second pass."""
    return NB_SPMV_MAX * (BLOCK // gw)


def vec_pass_rows():
    return NB_VEC * BLOCK


# ---------------------------------------------------------------------------------------------
# parsing the solver source
def read_source():
    """The text of solve_internal.h and of the three units, joined in this order."""
    parts = []
    for path in SOLVE_SOURCES:
        with open(path) as f:
            parts.append(f.read())
    return '\n'.join(parts)


def _function_body(src, signature):
    """Text of the function whose definition starts with `signature` (up to its closing brace at column 0)."""
    i = src.index(signature)
    j = src.index('\n}\n', i)
    return src[i:j]


def parse_constants(src):
    out = {}
    for name in ('BLOCK', 'NB_VEC', 'NB_SPMV_MAX'):
        m = re.search(r'constexpr int %s = (\d+);' % name, src)
        out[name] = int(m.group(1)) if m else None
    return out


def parse_gw_thresholds(src):
    """((threshold, gw), ...) and the default gw of `int spmv_gw(long long maxlen)`."""
    body = _function_body(src, 'int spmv_gw(')
    pairs = tuple((int(t), int(g)) for t, g in re.findall(r'maxlen >= (\d+) \? (\d+)', body))
    m = re.search(r': (\d+);', body)
    return pairs, int(m.group(1)) if m else None


def _cases(body, kernel):
    """{(label, GW, U)} of the `case N:` / `default:` lines of a switch that name `kernel<GW, U>`."""
    out = set()
    for label, gw, u in re.findall(r'(case \d+|default):[^\n]*?\b%s<(\d+), (\d+)>' % kernel, body):
        out.add((None if label == 'default' else int(label.split()[1]), int(gw), int(u)))
    return out


# the dispatch table of each SpMV kernel family: the function that maps a group width to its instantiation
TABLES = {'k_spmv': 'decltype(auto) with_spmv_kernel(', 'k_csr_spmv': 'decltype(auto) with_csr_spmv_kernel('}


def parse_dispatch(src):
    """The case lines of the dispatch tables, per kernel family."""
    return {kernel: _cases(_function_body(src, sig), kernel) for kernel, sig in TABLES.items()}


def instances_outside_tables(src):
    """The template argument lists of k_spmv / k_csr_spmv written anywhere but in the dispatch tables."""
    for sig in TABLES.values():
        body = _function_body(src, sig)
        src = src.replace(body, '')
    return re.findall(r'\bk_(?:csr_)?spmv\s*<[^>]*>', src)


# ---------------------------------------------------------------------------------------------
# row lengths
def axis_ranges(kv):
    """(jlo, jhi) of every basis function of the knot vector `kv`: the contiguous range of basis functions whose supports
    overlap its own in a span of positive length."""
    knots = np.asarray(kv.kv, dtype=np.float64)
    p = int(kv.p)
    mesh = np.unique(knots)
    k2m = np.searchsorted(mesh, knots)
    N = knots.size - p - 1
    lo_m, hi_m = k2m[:N], k2m[p + 1:p + 1 + N]
    jlo = np.empty(N, dtype=np.int64)
    jhi = np.empty(N, dtype=np.int64)
    for i in range(N):
        ov = (np.minimum(hi_m, hi_m[i]) > np.maximum(lo_m, lo_m[i]))
        idx = np.flatnonzero(ov)
        jlo[i], jhi[i] = idx[0], idx[-1] + 1
        assert ov[jlo[i]:jhi[i]].all()
    return jlo, jhi


def axis_pattern(kv):
    jlo, jhi = axis_ranges(kv)
    N = jlo.size
    indptr = np.concatenate(([0], np.cumsum(jhi - jlo)))
    indices = np.concatenate([np.arange(a, b) for a, b in zip(jlo, jhi)])
    return scipy.sparse.csr_matrix((np.ones(indices.size, dtype=np.int8), indices, indptr), shape=(N, N))


def patch_maxlen(kvs):
    """Product over axes of max_i (jhi - jlo): the longest row of the patch, as igx_solver_create computes it."""
    out = 1
    for kv in kvs:
        jlo, jhi = axis_ranges(kv)
        out *= int((jhi - jlo).max())
    return out


def patch_pattern(kvs):
    S = axis_pattern(kvs[0])
    for kv in kvs[1:]:
        S = scipy.sparse.kron(S, axis_pattern(kv), format='csr')
    return S


def multipatch_pattern(MP):
    """The global pattern sum_p X_p A_p X_p^T (0/1 CSR with sorted indices) of the finalized multipatch `MP`."""
    n = MP.numdofs
    rows, cols = [], []
    for p, (kvs, _) in enumerate(MP.patches):
        Sp = patch_pattern(tuple(kvs)).tocoo()
        l2g = np.asarray(MP.patch_to_global_idx(p), dtype=np.int64)
        rows.append(l2g[Sp.row])
        cols.append(l2g[Sp.col])
    r, c = np.concatenate(rows), np.concatenate(cols)
    S = scipy.sparse.csr_matrix((np.ones(r.size, dtype=np.int8), (r, c)), shape=(n, n))
    S.sum_duplicates()
    S.sort_indices()
    S.data[:] = 1
    return S


def max_row(S):
    return int(np.diff(S.indptr).max())


# ---------------------------------------------------------------------------------------------
# the cases
class PatchCase(NamedTuple):
    id: str
    axes: tuple        # (p, n, mult) per axis
    gw: int            # spmv_gw of its longest row (asserted, so that the table and the dispatch cannot drift apart)

    @property
    def dim(self):
        return len(self.axes)

    def kvs(self):
        from pyiga_amd import bspline
        return tuple(bspline.make_knots(p, 0.0, 1.0, n, mult=m) for p, n, m in self.axes)


class MultipatchCase(NamedTuple):
    id: str
    domain: str        # 'lshape', 'notebook' or 'cubes2' (joined by hand: numbered without a device)
    p: int
    n: int
    gw: int

    def build(self):
        import _mpsolve_model as M
        if self.domain == 'lshape':
            return M.lshape(p=self.p, n=self.n)
        if self.domain == 'notebook':
            return M.notebook(p=self.p, n=self.n)
        return two_cubes(self.p, self.n)


# structured SpMV: one case past the pass bound per GW, (2p+1)^d entries in the longest row of single knots
PATCH_CASES = [
    PatchCase('2d_p1_n725', ((1, 725, 1),) * 2, 4),           # 726^2 = 527 076 rows, 4.7 M nonzeros
    PatchCase('2d_p2_n512', ((2, 512, 1),) * 2, 8),           # 514^2
    PatchCase('2d_p3_n360', ((3, 360, 1),) * 2, 16),          # 363^2
    PatchCase('3d_p2_n39', ((2, 39, 1),) * 3, 32),            # 41^3
    PatchCase('3d_p3_n30', ((3, 30, 1),) * 3, 64),            # 33^3, 12 M nonzeros
    PatchCase('3d_p4_n9', ((4, 9, 1),) * 3, 64),              # the degree of C4 (one pass)
    PatchCase('3d_mixed_mult', ((2, 7, 1), (3, 6, 2), (1, 9, 1)), 16),     # mixed degrees, double knots on axis 1
    PatchCase('2d_p2_mult2', ((2, 12, 2), (1, 10, 1)), 4),
]

# CSR SpMV: the longest row includes the interface rows (multipatch_pattern); one case past the pass bound per GW
MULTIPATCH_CASES = [
    MultipatchCase('lshape_p1_n420', 'lshape', 1, 420, 4),     # 530 881 rows
    MultipatchCase('lshape_p2_n300', 'lshape', 2, 300, 8),
    MultipatchCase('notebook_p3_n260', 'notebook', 3, 260, 16),   # 276 k rows: also the Schwarz case past the vector grid
    MultipatchCase('lshape_p5_n145', 'lshape', 5, 145, 32),
    MultipatchCase('cubes2_p3_n23', 'cubes2', 3, 23, 64),
    MultipatchCase('notebook_p4_n12', 'notebook', 4, 12, 16),
]


def two_cubes(p=3, n=4):
    """Two unit cubes side by side along x, joined by hand (no interface detection: numbered without a device)."""
    from pyiga_amd import assemble, bspline, geometry
    kvs = 3 * (bspline.make_knots(p, 0.0, 1.0, n),)
    cube = geometry.unit_cube()
    MP = assemble.Multipatch([(kvs, cube), (kvs, cube.translate((1, 0, 0)))])
    MP.join_boundaries(0, (2, 1), 1, (2, 0))
    MP.finalize()
    return MP

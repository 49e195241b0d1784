"""The cases that run every instantiation and every loop of the multigrid kernels (pyiga_amd/csrc/multigrid.hip) and of the DIRK
kernels of pyiga_amd/csrc/solve_step.hip (k_vals_axpby, k_dirk_rhs), and what decides them.

A plain helper module (no GPU needed to import it): tests/test_mg_coverage_cpu.py checks on the host that the tables below reach
what they claim, tests/test_mg_kernels_gpu.py and tests/test_parabolic_gpu.py run them.

- ``GS_CASES``: one multipatch domain per group width of with_gs_kernel (k_csr_gs<GW, U> and k_csr_gs_block<GW, U>; the width is
  spmv_gw of the longest row, as for the CSR SpMV), each swept per colour and in one block, and per width one more whose
  largest colour has more rows than the one block has row groups (BLOCK_ONE / GW).  ``GS_BIG_CASE`` has more rows in
  one colour than one pass of k_csr_gs's grid-stride loop covers (``gs_pass_rows``: NB_GS_MAX blocks of BLOCK / GW rows).  The
  loop ``r += ngroups`` is one source line shared by all widths, so one width past the bound is enough: GW = 4 needs 524 288 rows
  in a colour, GW = 64 would need about 2.6 M rows of 343 entries.
- ``TRANSFER_CASES``: multipatches joined by hand whose dof counts and band widths differ from axis to axis on every level, so
  that k_mg_transfer cannot swap No[1] / No[2], Ni[1] / Ni[2] or w[1] / w[2] unnoticed (``transfer_restated`` is the kernel's
  indexing in numpy, with these swaps as options: test_mg_coverage_cpu.py shows each of them changes the result on every case),
  with repeated knots, a graded mesh (band widths that vary along an axis: the clamp and the zero padding of make_band), a
  flipped join and three levels.
- ``DENSE_CASES``: one-level hierarchies whose free dofs are fewer than one block of k_dense_apply, between one and two blocks,
  and in the thousands.
- ``dirk6_tableaux()``: two tableaux of IGX_DIRK_MAX_STAGES stages whose last stage combines 7 vectors in k_dirk_rhs, the most
  igx_solver_dirk_run can build; COMB_MAX must hold one more than the stages.

The bounds are those the project asserts for the same operations elsewhere (RELAX_BOUND, TRANSFER_BOUND, VCYCLE_BOUND).  The rule
for a case with longer rows or more colours: measure on the host how far the float64 model lies from the long-double reference on
the case's inputs; if that exceeds a quarter of the bound, the case's bound becomes 8 times the distance (a different but equally
valid summation order on the device).  tools/mg_case_distances.py measures them (no GPU: the oracle's matrices); the figures stand
next to the cases.  None comes near a quarter of its bound, so every case keeps the project's bound.
"""
import os
import re
from typing import NamedTuple

import numpy as np
import scipy.sparse

import _solver_cases as sc

ROOT = sc.ROOT
MULTIGRID_HIP = os.path.join(ROOT, 'pyiga_amd', 'csrc', 'multigrid.hip')
IGX_H = os.path.join(ROOT, 'include', 'igx.h')

# constants of multigrid.hip (test_mg_coverage_cpu.py reads them from the source and compares)
BLOCK = 256
NB_GS_MAX = 8192
BLOCK_ONE = 1024
# the (GW, U) instantiations of k_csr_gs and k_csr_gs_block: the widths and batches of k_csr_spmv
GS_INSTANCES = {(64, 8), (32, 4), (16, 4), (8, 4), (4, 4)}
# constants of the DIRK kernels of solve_step.hip and of include/igx.h
COMB_MAX = 8
AXPBY_U = 4
DIRK_MAX_STAGES = 6

RELAX_BOUND = 1e-12          # _relmax against the sequential sweep (test_multigrid_gpu.py)
TRANSFER_BOUND = 1e-13
VCYCLE_BOUND = 1e-10
EPS = 2.0 ** -52


def gs_pass_rows(gw):
    """Rows of one colour that one grid-stride pass of k_csr_gs covers at the largest grid: more rows take a second pass."""
    return NB_GS_MAX * (BLOCK // gw)


# ---------------------------------------------------------------------------------------------
# parsing the sources
def read_source(path=MULTIGRID_HIP):
    with open(path) as f:
        return f.read()


def parse_constants(src):
    out = {}
    for name in ('BLOCK', 'NB_GS_MAX', 'BLOCK_ONE'):
        m = re.search(r'constexpr int %s = (\d+);' % name, src)
        out[name] = int(m.group(1)) if m else None
    return out


GS_TABLE = 'decltype(auto) with_gs_kernel('


def parse_gs_dispatch(src):
    """The case lines of with_gs_kernel, per kernel: {(label, GW, U)}."""
    body = sc._function_body(src, GS_TABLE)
    return {kernel: sc._cases(body, kernel) for kernel in ('k_csr_gs', 'k_csr_gs_block')}


def gs_instances_outside_table(src):
    """The template argument lists of k_csr_gs / k_csr_gs_block written anywhere but in with_gs_kernel."""
    src = src.replace(sc._function_body(src, GS_TABLE), '')
    return re.findall(r'\bk_csr_gs(?:_block)?\s*<[^>]*>', src)


def parse_dirk_constants(solve_src, header_src):
    out = {}
    for name in ('COMB_MAX', 'AXPBY_U'):
        m = re.search(r'constexpr int %s = (\d+);' % name, solve_src)
        out[name] = int(m.group(1)) if m else None
    m = re.search(r'IGX_DIRK_MAX_STAGES = (\d+)', header_src)
    out['IGX_DIRK_MAX_STAGES'] = int(m.group(1)) if m else None
    return out


# ---------------------------------------------------------------------------------------------
# the smoother: one domain per width
SIDES = {'lshape': ((0, 'left'), (0, 'bottom'), (2, 'top')),
         'notebook': ((0, 'bottom'), (0, 'right'), (1, 'top'), (2, 'left'), (2, 'bottom'), (3, 'bottom')),
         'cubes2': ((0, (2, 0)), (1, (0, 1)))}


class GsCase(NamedTuple):
    id: str
    domain: str        # 'lshape', 'notebook' or 'cubes2' (joined by hand: numbered without a device)
    p: int
    n: int             # even: the case is coarsened once
    gw: int            # spmv_gw of its longest row (asserted)
    colours: int       # of the first-fit colouring under `sides` (asserted)
    distance: float    # float64 sequential sweep against the long-double colour sweep, _relmax (tools/mg_case_distances.py)

    def build(self):
        return sc.MultipatchCase(self.id, self.domain, self.p, self.n, self.gw).build()

    @property
    def sides(self):
        return SIDES[self.domain]


GS_CASES = [
    GsCase('lshape_p1_n8', 'lshape', 1, 8, 4, 6, 2.1e-16),
    GsCase('lshape_p2_n8', 'lshape', 2, 8, 8, 12, 3.0e-16),
    GsCase('notebook_p4_n8', 'notebook', 4, 8, 16, 33, 2.4e-16),
    GsCase('lshape_p5_n8', 'lshape', 5, 8, 32, 42, 1.7e-16),
    GsCase('cubes2_p3_n4', 'cubes2', 3, 4, 64, 80, 2.2e-16),           # 637 dofs, rows of 343: GW 64 by the 3D route
    GsCase('lshape_p7_n8', 'lshape', 7, 8, 64, 79, 4.7e-16),           # rows of 225: GW 64 by the 2D route
    # a colour of more rows than the BLOCK_ONE / GW row groups of the one-block sweep, which then strides (the largest colour:
    # 784, 374, 144, 75 and 30 rows against 256, 128, 64, 32 and 16 groups; no colour of the cases above has that many)
    GsCase('lshape_p1_n32', 'lshape', 1, 32, 4, 6, 3.0e-16),
    GsCase('lshape_p2_n32', 'lshape', 2, 32, 8, 12, 4.0e-16),
    GsCase('notebook_p4_n24', 'notebook', 4, 24, 16, 33, 2.2e-16),
    GsCase('lshape_p5_n24', 'lshape', 5, 24, 32, 47, 2.1e-16),
    GsCase('cubes2_p3_n6', 'cubes2', 3, 6, 64, 64, 2.5e-16),
]
# past one pass of the colour grid at GW 4 (524 288 rows): 3 149 825 dofs, 28 M nonzeros, 6 colours under the fixed sides, the
# largest of 786 944 rows
GS_BIG_CASE = GsCase('lshape_p1_n1024', 'lshape', 1, 1024, 4, 6, 5.6e-16)


def fixed_dofs(MP, sides):
    import _mpsolve_model as M
    return M.fixed_dofs(MP, list(sides))


def colour_lists(colour):
    """The rows of every colour in ascending order, colour after colour."""
    fr = np.flatnonzero(colour >= 0)
    order = fr[np.argsort(colour[fr], kind='stable')]
    counts = np.bincount(colour[fr])
    return np.split(order, np.cumsum(counts)[:-1])


def _ld(A):
    A = scipy.sparse.csr_matrix(A)
    return scipy.sparse.csr_matrix((A.data.astype(np.longdouble), A.indices, A.indptr), shape=A.shape)


class ColourSweep:
    """Gauss-Seidel in colour order in long double, a colour at a time: x[rows] = (b - (A x - d x))[rows] / d[rows].  Rows of one
    colour do not couple, so this is the sequential sweep in (colour, index) order."""

    def __init__(self, A, colours):
        Al = _ld(A)
        self.colours = colours
        self.d = Al.diagonal()
        self.rows = [Al[r] for r in colours]

    def sweep(self, x, b, kind='forward'):
        x = np.array(x, dtype=np.longdouble)
        b = np.asarray(b, dtype=np.longdouble)
        k = len(self.colours)
        seq = {'forward': list(range(k)), 'backward': list(range(k))[::-1]}
        seq['symmetric'] = seq['forward'] + seq['backward']
        for c in seq[kind]:
            r, d = self.colours[c], self.d[self.colours[c]]
            x[r] = (b[r] - (self.rows[c] @ x - d * x[r])) / d
        return x


def relmax(a, b):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return float(np.abs(a - b).max() / np.abs(b).max())


def relax_inputs(tag, n, fixed):
    """Start vector and right-hand side of the relax tests (zero on the fixed dofs, as the device masks them)."""
    import zlib
    rng = np.random.default_rng(zlib.crc32(tag.encode()))
    x0, b = rng.standard_normal(n), rng.standard_normal(n)
    x0[fixed] = 0.0
    b[fixed] = 0.0
    return x0, b


# ---------------------------------------------------------------------------------------------
# the transfers
def _graded(p, mesh, double=()):
    """The open knot vector of degree p over `mesh` refined once (every span halved), the knots of `double` twice: its
    coarsening is the knot vector over `mesh`, so the coarse space is nested."""
    from pyiga_amd import bspline
    mesh = np.asarray(mesh, dtype=np.float64)
    inner = np.sort(np.concatenate((mesh[1:-1], np.asarray(double, dtype=np.float64))))
    coarse = bspline.KnotVector(np.concatenate((np.repeat(mesh[0], p + 1), inner, np.repeat(mesh[-1], p + 1))), p)
    return coarse.refine()


def _uniform(axes):
    from pyiga_amd import bspline
    return tuple(bspline.make_knots(p, 0.0, 1.0, n, mult=m) for p, n, m in axes)


def _aniso3d():
    # per axis (p, n, mult): 5 x 13 x 31 dofs over 3 x 7 x 16, bands of 2 / 3 / 4 (prolongation) and 3 / 5 / 7 (restriction)
    from pyiga_amd import assemble, geometry
    kvs = _uniform(((1, 4, 1), (2, 6, 2), (3, 10, 3)))
    cube = geometry.unit_cube()
    MP = assemble.Multipatch([(kvs, cube), (kvs, cube.translate((1, 0, 0)))])
    MP.join_boundaries(0, (2, 1), 1, (2, 0))
    MP.finalize()
    return MP


def _two_squares(kvs, flipped):
    """Two unit squares, the second on top of the first; flipped: the second mirrored in x, so that the join runs backwards."""
    from pyiga_amd import assemble, geometry
    squ = geometry.unit_square()
    top = squ.scale((-1, 1)).translate((1, 1)) if flipped else squ.translate((0, 1))
    MP = assemble.Multipatch([(kvs, squ), (kvs, top)])
    MP.join_boundaries(0, 'top', 1, 'bottom', flip=(True,) if flipped else None)
    MP.finalize()
    return MP


class TransferCase(NamedTuple):
    id: str
    make: object       # () -> the finest multipatch
    levels: int
    sides: tuple       # ((patch, bdspec), ...): fixed as whole sides
    tags: frozenset    # of '3d', 'repeated', 'graded', 'flipped', 'three_level'
    distance: float    # float64 P x and P^T r against long double, the larger _relmax (tools/mg_case_distances.py)

    def hierarchy(self):
        """The multipatches of every level, the finest first (coarsen_knots on every axis, the joins replayed)."""
        import _mg_model as G
        MPs = [self.make()]
        for _ in range(self.levels - 1):
            MPs.append(G.coarsen(MPs[-1]))
        return MPs


TRANSFER_CASES = [
    TransferCase('aniso3d', _aniso3d, 2, ((0, (2, 0)),), frozenset({'3d', 'repeated'}), 4.3e-16),
    TransferCase('flipped2d', lambda: _two_squares(_uniform(((2, 6, 1), (3, 10, 1))), True), 2, ((0, 'bottom'), (1, 'left')),
                 frozenset({'flipped'}), 1.5e-16),
    TransferCase('graded2d', lambda: _two_squares((_graded(1, (0.0, 0.1, 0.25, 0.55, 1.0)),
                                                   _graded(3, (0.0, 0.2, 0.3, 0.5, 0.6, 0.8, 1.0), double=(0.5,))), False), 2,
                 ((0, 'left'), (1, 'top')), frozenset({'graded', 'repeated'}), 1.7e-16),
    TransferCase('three_level2d', lambda: _two_squares(_uniform(((2, 8, 1), (3, 12, 1))), False), 3, ((0, 'bottom'),),
                 frozenset({'three_level'}), 2.8e-16),
]


def make_band(P, transposed=False):
    """(lo, v, w) of the dense 1D prolongation P (transposed: of its transpose), as make_band of multigrid.hip: row o reads the
    source indices lo[o] .. lo[o] + w with the weights v[o] (zero-padded; lo + w <= the number of source dofs)."""
    P = np.asarray(P, dtype=np.float64)
    if transposed:
        P = P.T
    no, ni = P.shape
    first = np.zeros(no, dtype=np.int64)
    w = 1
    for o in range(no):
        nz = np.flatnonzero(P[o])
        if nz.size:
            first[o] = nz[0]
            w = max(w, int(nz[-1] - nz[0] + 1))
    lo = np.maximum(0, np.minimum(first, ni - w))
    v = np.zeros((no, w))
    for o in range(no):
        t = np.arange(min(w, ni - lo[o]))
        v[o, t] = P[o, lo[o] + t]
    return lo, v, w


def transfer_restated(Ps, x, transposed=False, swap=None):
    """k_mg_transfer's indexing on one patch in numpy: the target vector (local dofs, last axis fastest) from the source `x`
    through the bands of the 1D prolongations `Ps` (2D: a one-dof outer axis in front, as the set-up adds).  `swap`: None, or
    one of the mistakes the transfer cases must expose -- 'No' decodes the target index with No[1] and No[2] exchanged, 'Ni'
    addresses the source with Ni[1] and Ni[2] exchanged, 'w' runs the loops of axes 1 and 2 with each other's width.  Indices a
    mistaken kernel would read out of range wrap here: all that matters is that the result changes."""
    Ps = [np.ones((1, 1))] * (3 - len(Ps)) + [np.asarray(P.toarray() if scipy.sparse.issparse(P) else P) for P in Ps]
    bands = [make_band(P, transposed) for P in Ps]
    No = [(P.shape[1] if transposed else P.shape[0]) for P in Ps]
    Ni = [(P.shape[0] if transposed else P.shape[1]) for P in Ps]
    lo, v, w = [b[0] for b in bands], [b[1] for b in bands], [b[2] for b in bands]
    No_d = [No[0], No[2], No[1]] if swap == 'No' else No
    Ni_a = [Ni[0], Ni[2], Ni[1]] if swap == 'Ni' else Ni
    w_l = [w[0], w[2], w[1]] if swap == 'w' else w
    x = np.asarray(x).ravel()
    i = np.arange(int(np.prod(No)))
    i2, t = i % No_d[2], i // No_d[2]
    i1, i0 = t % No_d[1], t // No_d[1]
    idx = [i0 % No[0], i1 % No[1], i2 % No[2]]
    out = np.zeros(i.size, dtype=x.dtype)
    for t0 in range(w_l[0]):
        a0 = v[0].ravel()[(idx[0] * w_l[0] + t0) % v[0].size]
        for t1 in range(w_l[1]):
            a1 = a0 * v[1].ravel()[(idx[1] * w_l[1] + t1) % v[1].size]
            for t2 in range(w_l[2]):
                a2 = v[2].ravel()[(idx[2] * w_l[2] + t2) % v[2].size]
                src = ((lo[0][idx[0]] + t0) * Ni_a[1] + (lo[1][idx[1]] + t1)) * Ni_a[2] + lo[2][idx[2]] + t2
                out += a1 * a2 * x[src % x.size]
    return out


def axis_prolongations(kvs_c, kvs_f):
    from pyiga_amd import bspline
    return [bspline.prolongation(c, f).toarray() for c, f in zip(kvs_c, kvs_f)]


# ---------------------------------------------------------------------------------------------
# the dense inverse: free dofs below one block of k_dense_apply, between one and two, in the thousands
class DenseCase(NamedTuple):
    id: str
    p: int
    n: int             # of the L-shape
    lo: int            # the free dofs lie in (lo, hi], and are no multiple of BLOCK
    hi: int

    def build(self):
        import _mpsolve_model as M
        return M.lshape(p=self.p, n=self.n)

    @property
    def sides(self):
        return SIDES['lshape']


DENSE_CASES = [
    DenseCase('lshape_p2_n4', 2, 4, 0, 255),
    DenseCase('lshape_p2_n10', 2, 10, 256, 511),
    DenseCase('lshape_p2_n24', 2, 24, 1500, 8192),
]


# ---------------------------------------------------------------------------------------------
# DIRK: tableaux of the most stages, every entry of the strict lower triangle nonzero
def dirk6_tableaux():
    """{'sdirk6': A, 'esdirk6': A}: shape (7, 6), one constant diagonal for both (esdirk6: an explicit first stage), a full strict lower
    triangle of small distinct coefficients, the last row b equal to the last stage row.  The last stage combines
    M x, five F_j and f: 7 vectors.  Not consistent schemes; the device and the host model integrate the same recurrence."""
    s = DIRK_MAX_STAGES
    out = {}
    for name, gamma, explicit in (('sdirk6', 0.25, False), ('esdirk6', 0.25, True)):
        A = np.zeros((s + 1, s))
        for i in range(s):
            for j in range(i):
                A[i, j] = 0.02 + 0.01 * ((3 * i + 5 * j) % 7) + 0.001 * i
            A[i, i] = 0.0 if (explicit and i == 0) else gamma
        A[s] = A[s - 1]
        out[name] = A
    return out

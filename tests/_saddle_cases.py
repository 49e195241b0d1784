"""The cases of the tests of the device saddle-point solver (csrc/solve_saddle.hip, solvers.SaddlePointSystem): plain data and
NumPy, no GPU, no library load.

* the pair cases th2, th3, q1p0, hi2, lo2 of tests/_pair_cases.py (imported, not copied) for the transposed layout;
* the notebook system of golden_pair.npz (`stokes_*`, 2D, nc = 2) and the 3D cavity of golden_saddle.npz (`stokes3_*`, nc = 3);
* what the host model (_saddle_model.py) gives on them -- iteration counts, errors against the golden solutions, true residuals --
  recorded here, asserted by tests/test_saddle_cpu.py and used as the yardstick of tests/test_saddle_gpu.py;
* the group-width rule of the two row kernels restated, and the kernel cases that reach every instantiation of their dispatch
  tables (with_saddle_u_kernel, with_saddle_p_kernel).
"""
from typing import NamedTuple

import numpy as np
import scipy.sparse

import _pair_cases as pc

TRANSPOSE_CASES = ('th2', 'th3', 'q1p0', 'hi2', 'lo2')

# ---------------------------------------------------------------------------------------------
# the model's results (python3 tests/test_saddle_cpu.py prints them again).  Per variant and tolerance: MINRES iterations, max |u -
# u_gold| / max |u_gold| with the pressure shifted so that its first coefficient is 0, and the true relative residual.
#   unpinned: the notebook's bcs without its pinned pressure dof, the mean of the lifted pressure right-hand side removed
#   pinned:   the notebook's bcs verbatim
MODEL = {
    ('stokes', 'unpinned', 1e-8): (78, 3.63e-8, 1.09e-8),
    ('stokes', 'unpinned', 1e-12): (95, 3.59e-8, 9.83e-13),
    ('stokes', 'pinned', 1e-8): (127, 2.95e-9, 9.27e-9),
    ('stokes', 'pinned', 1e-12): (158, 2.56e-13, 8.74e-13),
    # the 3D lid data is not discretely compatible (mean of the lifted pressure right-hand side 4.4e-2 of its norm), so the
    # unpinned solve (with a warning) answers another question than the golden, pinned one: 0.97 away, which the recorded error
    # says; what that variant checks is the iteration count, the residual and the agreement with the model's own solution.
    # At tol 1e-12 the model's estimate sits on a plateau of 1.36e-12 phi_0 from iteration 180 to 247 (the accuracy this singular,
    # projected system allows) and leaves it at 248; where on that plateau a solve crosses 1e-12 is decided by rounding (the device:
    # 178).  The variant is therefore compared at tol 1e-10, where the estimate falls by a decade in 5 iterations.
    ('stokes3', 'unpinned', 1e-8): (158, 0.972, 1.08e-8),
    ('stokes3', 'unpinned', 1e-10): (170, 0.972, 6.30e-11),
    ('stokes3', 'pinned', 1e-8): (127, 7.78e-11, 7.68e-9),
    ('stokes3', 'pinned', 1e-12): (146, 2.65e-13, 1.44e-12),
}
# rounding order (another BLAS, the device's summation trees) moves the stop by an iteration or two; the device test allows 3
MODEL_ITER_SLACK = 1
# |velocity('mean') - velocity('auto')| of the model: the two normalisations shift the pressure of one and the same solve
MODEL_VELOCITY_DIFF = 0.0
# viscosity 0.01 at tol 1e-8, unpinned: with the Schur scale (as at viscosity 1) and without it
MODEL_VISCOSITY = {'scaled': 78, 'unscaled': 109}
# mean / norm of the lifted pressure right-hand side of the notebook system: discretely compatible
MODEL_RHS_MEAN = 1e-15

# ---------------------------------------------------------------------------------------------
# the kernels' constants and width rule (solve_internal.h, solve.hip: spmv_gw; solve_saddle.hip: saddle_occupancy)
BLOCK = 256
NB_SPMV_MAX = 8192
NB_SADDLE_MAX = NB_SPMV_MAX // 2          # blocks of one row kernel at most: both launches of a product share one array of partials
GWS = (4, 8, 16, 32, 64)


def spmv_gw(maxlen):
    return 64 if maxlen >= 192 else 32 if maxlen >= 96 else 16 if maxlen >= 48 else 8 if maxlen >= 24 else 4


def pass_rows(gw):
    """Rows one grid pass of a row kernel holds at most."""
    return NB_SADDLE_MAX * BLOCK // gw


def _mesh_supports(p, n, mult):
    """(first span, last span + 1) of every function of the open knot vector of degree p with n spans on [0, 1] and interior
    knots of multiplicity mult."""
    knots = np.concatenate((np.zeros(p + 1), np.repeat(np.arange(1, n), mult), np.full(p + 1, n))).astype(np.int64)
    N = knots.size - p - 1
    return np.array([(knots[i], knots[i + p + 1]) for i in range(N)], dtype=np.int64)


def axis_ranges(trial, test):
    """(jlo, jhi) per test function of one axis: the trial functions whose mesh support meets its own; axes as (p, n, mult)."""
    su, sv = _mesh_supports(*trial), _mesh_supports(*test)
    jlo = np.searchsorted(su[:, 1], sv[:, 0], side='right')
    jhi = np.searchsorted(su[:, 0], sv[:, 1], side='left')
    return jlo, jhi


def longest_rows(trial, test):
    """Longest row of A (velocity x velocity), of B^T (velocity rows, pressure columns) and of B (pressure rows)."""
    out = []
    for rows, cols in ((trial, trial), (trial, test), (test, trial)):
        m = 1
        for r, c in zip(rows, cols):
            jlo, jhi = axis_ranges(c, r)
            m *= int((jhi - jlo).max())
        out.append(m)
    return tuple(out)


def widths(trial, test):
    """(gw of k_saddle_u, gw of k_saddle_p) of a system over these spaces."""
    a, t, b = longest_rows(trial, test)
    return spmv_gw(max(a, t)), spmv_gw(b)


def ndofs(space):
    return tuple(n * m - m + p + 1 for p, n, m in space)


class KernelCase(NamedTuple):
    id: str
    trial: tuple           # velocity space, per axis (p, n, mult)
    test: tuple            # pressure space
    nc: int
    absent: tuple          # blocks (p, q) of A never taken
    pinned: bool           # a fixed pressure dof besides the fixed velocity dofs


_TH2, _TH2P = ((3, 4, 3), (3, 3, 3)), ((2, 4, 2), (2, 3, 2))          # (C^0 cubics, multiplicity 3: rows of 49 -> width 16)
_TH3, _TH3P = ((2, 2, 2), (2, 3, 2), (2, 2, 2)), ((1, 2, 1), (1, 3, 1), (1, 2, 1))
_Q1, _P0 = ((1, 3, 1), (1, 2, 1)), ((0, 3, 1), (0, 2, 1))
_TH21, _TH21P = ((2, 4, 2), (2, 3, 2)), ((1, 4, 1), (1, 3, 1))
_TH32, _TH32P = ((3, 3, 1), (3, 4, 1), (3, 3, 1)), ((2, 3, 1), (2, 4, 1), (2, 3, 1))
_BIG, _BIGP = ((1, 530, 1), (1, 520, 1)), ((0, 530, 1), (0, 520, 1))

# every width of both tables with nc = 2 and with nc = 3 (the number of components is free of the dimension), an absent
# off-diagonal block, masked velocity rows (all), a masked pressure row, and one case past a grid pass at the narrowest width
KERNEL_CASES = [
    KernelCase('q1p0-2', _Q1, _P0, 2, (), False),
    KernelCase('q1p0-3', _Q1, _P0, 3, ((0, 2),), True),
    KernelCase('th21-2', _TH21, _TH21P, 2, ((1, 0),), True),
    KernelCase('th21-3', _TH21, _TH21P, 3, (), False),
    KernelCase('th2m-2', _TH2, _TH2P, 2, (), True),
    KernelCase('th2m-3', _TH2, _TH2P, 3, ((2, 0), (0, 1)), False),
    KernelCase('th3-2', _TH3, _TH3P, 2, ((0, 1),), False),
    KernelCase('th3-3', _TH3, _TH3P, 3, (), True),
    KernelCase('th32-2', _TH32, _TH32P, 2, (), False),
    KernelCase('th32-3', _TH32, _TH32P, 3, ((1, 2),), True),
    KernelCase('big-2', _BIG, _BIGP, 2, ((0, 1), (1, 0)), True),
]
KERNEL_BY_ID = {c.id: c for c in KERNEL_CASES}


def kernel_kvs(case, mod):
    return tuple(tuple(mod.make_knots(p, 0.0, 1.0, n, mult=m) for p, n, m in sp) for sp in (case.trial, case.test))


# ---------------------------------------------------------------------------------------------
# the golden systems
def golden_csr(g, name):
    return scipy.sparse.csr_matrix((g[name + '_data'], g[name + '_indices'], g[name + '_indptr']), shape=tuple(int(x) for x in g[name + '_shape']))


class System(NamedTuple):
    name: str
    nc: int
    spaces: tuple          # (velocity, pressure), per axis (p, n, mult)
    A: object
    B: object
    bcs: tuple
    u: np.ndarray

    @property
    def nv(self):
        return self.A.shape[0]

    def variant(self, which):
        """(bcs, project) of 'pinned' (the bcs verbatim) or 'unpinned' (without the pressure dofs; the mean projected)."""
        idx, val = self.bcs
        if which == 'pinned':
            return (idx, val), False
        keep = idx < self.nv
        return (idx[keep], val[keep]), True


def system(golden, name):
    """'stokes': the notebook system of golden_pair.npz; 'stokes3': the 3D cavity of golden_saddle.npz."""
    g = golden('pair' if name == 'stokes' else 'saddle')
    spaces = (((3, 6, 2), (3, 4, 2)), ((2, 6, 1), (2, 4, 1))) if name == 'stokes' else (_TH3, _TH3P)
    return System(name, len(spaces[0]), spaces, golden_csr(g, name + '_A_grad'), golden_csr(g, name + '_A_div'),
                  (np.asarray(g[name + '_bcs_idx'], dtype=np.int64), np.asarray(g[name + '_bcs_val'], dtype=np.float64)),
                  np.asarray(g[name + '_u']))


def model_preconditioner(sys_, free, orc, viscosity=1.0, scale=None):
    """The block-diagonal preconditioner of the model for a golden system, 1D matrices from the oracle."""
    import _saddle_model as sm
    kvs = [[orc.make_knots(p, 0.0, 1.0, n, mult=m) for p, n, m in sp] for sp in sys_.spaces]
    mats_u = [(orc.bsp_mixed_deriv_biform_1d(kv, 1, 1), orc.bsp_mixed_deriv_biform_1d(kv, 0, 0)) for kv in kvs[0]]
    mats_p = [(None, orc.bsp_mixed_deriv_biform_1d(kv, 0, 0)) for kv in kvs[1]]
    return sm.block_preconditioner(ndofs(sys_.spaces[0]), ndofs(sys_.spaces[1]), sys_.nc, free, mats_u, mats_p,
                                   scale=viscosity if scale is None else scale, viscosity=viscosity)


def model_solve(sys_, which, tol, orc, viscosity=1.0, scale=None):
    """(u with the pressure's first coefficient 0, info) of the model on a golden system."""
    import _saddle_model as sm
    bcs, project = sys_.variant(which)
    free = np.ones(sys_.nv + sys_.B.shape[0], dtype=bool)
    free[bcs[0]] = False
    P = model_preconditioner(sys_, free, orc, viscosity, scale)
    u, info = sm.solve(viscosity * sys_.A, sys_.B, sys_.nc, bcs, P=P, tol=tol, project=project)
    return sm.normalise_pressure(u, sys_.nv, 'first'), info

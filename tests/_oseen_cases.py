"""The cases of the tests of the device Oseen solver (csrc/solve_gmres.hip, solvers.OseenSystem): plain data and NumPy, no GPU, no
library load.

* the golden systems `oseen2` / `oseen3` of golden_oseen.npz (the Stokes systems of _saddle_cases.py plus the convection matrix
  of a rotating wind, viscosity `nu`);
* what the host model (_gmres_model.py) gives on them, per case, preconditioner form and restart -- Arnoldi steps, restarts, the
  error against the golden solution, the true residual -- recorded here (python3 tests/test_oseen_cpu.py prints them again),
  asserted by tests/test_oseen_cpu.py and used as the yardstick of tests/test_oseen_gpu.py;
* the shapes of the kernel tests (tests/test_gmres_kernels_gpu.py) and the constants of their bounds.
"""
from typing import NamedTuple

import numpy as np

import _saddle_cases as sc

CASES = ('oseen2', 'oseen3')
BASE = {'oseen2': 'stokes', 'oseen3': 'stokes3'}

# (case, triangular, restart, tol) -> (Arnoldi steps, restarts, max |u - u_gold| / max |u_gold|, true relative residual); block
# Kronecker preconditioner, the golden bcs verbatim (pinned pressure dof).  restart None: a cycle longer than the solve.
# restart 128 is the longest cycle the device holds, and what the device tests solve with.
MODEL = {
    ('oseen2', False, None, 1e-12): (164, 0, 8.71e-13, 5.63e-13),
    ('oseen2', True, None, 1e-12): (108, 0, 3.57e-12, 6.40e-13),
    ('oseen2', False, 128, 1e-12): (814, 6, 6.53e-11, 9.75e-13),
    ('oseen2', True, 128, 1e-12): (108, 0, 3.57e-12, 6.40e-13),
    ('oseen3', False, None, 1e-12): (128, 0, 6.59e-13, 1.12e-12),
    ('oseen3', True, None, 1e-12): (103, 0, 1.25e-13, 1.53e-12),
    ('oseen3', False, 128, 1e-12): (128, 0, 6.59e-13, 1.12e-12),
    ('oseen3', True, 128, 1e-12): (103, 0, 1.25e-13, 1.53e-12),
}
# Short cycles stagnate on these indefinite systems, the well-known weakness of restarted GMRES: at nu = 0.1 the model with
# restart 40 has not converged after 1000 steps on either case with the block-diagonal preconditioner (true residuals 6.0e-3 and
# 9.9e-2) nor on oseen2 with the triangular one (1.3e-7); oseen3 with the triangular one takes 791 steps.  With restart 5 it
# converges on none of the systems tried (the Stokes systems and viscosities up to 100 included: 5.8e-4 after 3000 steps on
# `stokes` with the triangular preconditioner).  The restart tests therefore run on the Stokes system `stokes` (convection=None,
# pinned, triangular), where restart 20 converges, and compare restart 5 with the model after RESTART5_STEPS steps.
#
# the Stokes systems (convection=None) by GMRES(128) with the block-diagonal preconditioner at tol 1e-12, against the MINRES
# goldens stokes_u / stokes3_u: (steps, error, residual) per (base, variant); `stokes` pinned restarts once (131 steps in one cycle)
MODEL_STOKES = {
    ('stokes', 'pinned'): (147, 2.01e-10, 8.67e-13),
    ('stokes', 'unpinned'): (87, 3.58e-08, 9.76e-13),
    ('stokes3', 'pinned'): (119, 2.18e-13, 1.82e-12),
}
# `stokes` pinned, triangular, tol 1e-12: (steps, restarts) of restart 20 and of one long cycle; the two solutions differ by 1.1e-9
MODEL_RESTART20 = (1700, 84)
MODEL_LONG = (73, 0)
RESTART5_STEPS = 60                      # 12 cycles of 5: 11 restarts

# ---------------------------------------------------------------------------------------------
# the kernels' constants (solve_internal.h, solve_gmres.hip)
BLOCK = 256
NB_VEC = 1024
MB = 8
RESTART = 40
# free entries of w and of the columns of V on the oseen2 patch (the fixed ones hold zeros, as every vector of a solve does): below,
# at and above a wave; one block and one more
SMALL_FREE = (1, 63, 64, 65, BLOCK, BLOCK + 1)
# columns: the tail of a chunk, one chunk, a chunk and one, several chunks, every column a solver with restart 40 holds
COLUMNS = (1, 7, 8, 9, 17, RESTART + 1)
# a plain patch whose vectors wrap the grid-stride loops: more than NB_VEC * BLOCK entries
GRID_SPACES = (((1, 362, 1), (1, 362, 1)), ((0, 362, 1), (0, 362, 1)))
GRID_COLUMNS = (9, 17)

# additions in the reduction tree of a coefficient h_k behind the thread's own chain (which is within n): 6 shuffle steps, 3 adds
# across the four waves of a block, the block partials added one after the other (at most NB_VEC, within n for n >= BLOCK; for
# smaller n one block), the sum of the two passes (1), the rounding of every product (1): 11, taken as 12
C_DOT = 12
# operations on an entry of w in one pass besides the `cols` multiply-subtracts: none; c' covers the rounding of h itself as it
# enters every product (1 per term, folded into the magnitude sum) and the final store: 2
C_UPD = 2


def dot_blocks(n, restart=RESTART):
    """Blocks of k_gm_dots: what fits the shared array of partials for restart + 1 columns, at most vec_blocks(n)."""
    return min(vec_blocks(n), (2 * sc.NB_SPMV_MAX - NB_VEC) // (restart + 1))


def vec_blocks(n):
    return max(1, min(NB_VEC, (n + BLOCK - 1) // BLOCK))


# ---------------------------------------------------------------------------------------------
# the golden systems
class System(NamedTuple):
    name: str
    nc: int
    spaces: tuple
    A: object              # nu A_grad + A_conv
    B: object
    bcs: tuple
    u: np.ndarray
    nu: float
    amp: float
    A_grad: object
    A_conv: object

    @property
    def nv(self):
        return self.A.shape[0]


def system(golden, name):
    g = golden('oseen')
    base = sc.system(golden, BASE[name])
    nu = float(g[name + '_nu'])
    Ag, Ac = sc.golden_csr(g, name + '_A_grad'), sc.golden_csr(g, name + '_A_conv')
    return System(name, base.nc, base.spaces, (nu * Ag + Ac).tocsr(), sc.golden_csr(g, name + '_A_div'),
                  (np.asarray(g[name + '_bcs_idx'], dtype=np.int64), np.asarray(g[name + '_bcs_val'], dtype=np.float64)),
                  np.asarray(g[name + '_u']), nu, float(g[name + '_amp']), Ag, Ac)


def model_solve(sys_, orc, triangular, restart, tol, maxiter=1000):
    """(u, info) of the GMRES model on a golden Oseen system, block Kronecker preconditioner."""
    import _gmres_model as gm
    free = np.ones(sys_.nv + sys_.B.shape[0], dtype=bool)
    free[sys_.bcs[0]] = False
    P = sc.model_preconditioner(sys_, free, orc, viscosity=sys_.nu)
    return gm.solve(sys_.A, sys_.B, sys_.nc, sys_.bcs, P=P, tol=tol, maxiter=maxiter, restart=maxiter if restart is None else restart,
                    triangular=triangular)


def model_stokes(golden, orc, base, which, tol=1e-12, maxiter=1000, restart=None, triangular=False):
    """(u with the pressure's first coefficient 0, info) of the GMRES model on a golden Stokes system of _saddle_cases.py."""
    import _gmres_model as gm
    M = sc.system(golden, base)
    bcs, project = M.variant(which)
    free = np.ones(M.nv + M.B.shape[0], dtype=bool)
    free[bcs[0]] = False
    P = sc.model_preconditioner(M, free, orc)
    u, info = gm.solve(M.A, M.B, M.nc, bcs, P=P, tol=tol, maxiter=maxiter, restart=maxiter if restart is None else restart,
                       project=project, triangular=triangular)
    return gm.normalise_pressure(u, M.nv, 'first'), info

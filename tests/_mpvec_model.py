"""Host model of the device solves of vector-valued forms on a multipatch (solvers.MultipatchVectorSystem,
igx_solver_create_multipatch_block in pyiga_amd/csrc/solve.hip), and the cases that run every k_csr_block_spmv instantiation.
Host only; reuses _mpsolve_model, _vecsolve_model and _solver_cases.

- ``glue(MP, mats, nc)``: the blocked global matrix  sum_p (I_nc (x) X_p) A_p (I_nc (x) X_p)^T  of the per-patch blocked matrices
  A_p, in patch order.
- ``BlockSchwarzModel``: diag(P_0, .., P_{nc-1}), one ``SchwarzModel`` per component on its slice of the blocked vectors.
- ``MPVEC_CASES``: the first five multipatch cases of the scalar CSR SpMV (one per group width, each past one grid of rows) at 2
  and 3 components.  At nc = 2 all four blocks are present; at nc = 3 the diagonal, (0, 1) and (2, 0): five blocks, so that the
  absent-block branch is taken.
- ``parse_csr_block_dispatch``: the case lines of with_csr_block_spmv_kernel.
"""
import re
from typing import NamedTuple

import numpy as np
import scipy.linalg
import scipy.sparse

import _mpsolve_model as M
import _solver_cases as sc

# the (GW, U, NC) instantiations of k_csr_block_spmv
CSR_BLOCK_SPMV_INSTANCES = {(gw, 4, 2) for gw in sc.GWS} | {(gw, 2, 3) for gw in sc.GWS}
TABLE = 'decltype(auto) with_csr_block_spmv_kernel('

PRESENT = {2: ((0, 0), (0, 1), (1, 0), (1, 1)),
           3: ((0, 0), (1, 1), (2, 2), (0, 1), (2, 0))}


def bfuns(nc):
    return [('u', nc), ('v', nc)]


def parse_csr_block_dispatch(src):
    """{(label, GW, U, NC)} of the case lines of with_csr_block_spmv_kernel that name k_csr_block_spmv<GW, U, NC>."""
    body = sc._function_body(src, TABLE)
    out = set()
    for label, gw, u, nc in re.findall(r'(case \d+|default):[^\n]*?\bk_csr_block_spmv<(\d+), (\d+), (\d+)>', body):
        out.add((None if label == 'default' else int(label.split()[1]), int(gw), int(u), int(nc)))
    return out


def csr_block_instances_outside_table(src):
    body = sc._function_body(src, TABLE)
    return re.findall(r'\bk_csr_block_spmv\s*<[^>]*>', src.replace(body, ''))


class MPVecCase(NamedTuple):
    id: str
    mp: sc.MultipatchCase
    nc: int

    @property
    def gw(self):
        return self.mp.gw

    @property
    def present(self):
        return PRESENT[self.nc]

    def build(self):
        return self.mp.build()


MPVEC_CASES = [MPVecCase('%s_nc%d' % (c.id, nc), c, nc) for c in sc.MULTIPATCH_CASES[:5] for nc in (2, 3)]

# two sides per domain: component 0 is fixed on the first, the last component on the second
CASE_SIDES = {'lshape': [(0, 'left'), (2, 'top')], 'notebook': [(0, 'bottom'), (2, 'left')], 'cubes2': [(0, (2, 0)), (1, (0, 1))]}


def glue(MP, mats, nc):
    """sum_p (I_nc (x) X_p) A_p (I_nc (x) X_p)^T in patch order: `mats[p]` the blocked (nc N_p) x (nc N_p) matrix of patch p."""
    n = MP.numdofs
    A = scipy.sparse.csr_matrix((nc * n, nc * n))
    I = scipy.sparse.identity(nc, format='csr')
    for p, Ap in enumerate(mats):
        X = scipy.sparse.kron(I, MP.patch_to_global(p), format='csr')
        A = A + X @ scipy.sparse.csr_matrix(Ap) @ X.T
    A = A.tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A


def interface_rows_gain(MP, S):
    """Per shared dof, the entries its row of the global pattern `S` has more than the longest of the local rows it joins: an
    interface row is the sum of several patches' rows, so it is longer than the rows of any one patch there."""
    local = [np.diff(sc.patch_pattern(tuple(kvs)).indptr) for kvs, _ in MP.patches]
    glob = np.diff(S.indptr)
    first = int(MP.M_ofs[-1])
    return np.array([glob[first + sd] - max(local[p][i] for p, i in members) for sd, members in enumerate(MP.shared_dofs)])


def blocked_fixed(MP, sides_per_comp, nc, extra=()):
    """Blocked global indices: component c fixed on the sides ``sides_per_comp[c]`` ([(patch, bdspec), ...]), plus `extra`."""
    n = MP.numdofs
    parts = [M.fixed_dofs(MP, sides) + c * n for c, sides in enumerate(sides_per_comp) if sides]
    parts.append(np.asarray(extra, dtype=np.int64))
    return np.unique(np.concatenate(parts))


class BlockSchwarzModel:
    """diag(P_0, .., P_{nc-1}) on blocked vectors of nc * n entries.  `setups`: per component (boxes, U, lam, mode), as
    MultipatchVectorSystem.schwarz_setup() gives them; `fixed`: the blocked fixed dofs."""

    def __init__(self, nglobal, shapes, maps, fixed, setups):
        self.n = int(nglobal)
        self.nc = len(setups)
        fixed = np.asarray(fixed, dtype=np.int64)
        self.parts = []
        for c, (boxes, U, lam, mode) in enumerate(setups):
            fc = fixed[(fixed >= c * self.n) & (fixed < (c + 1) * self.n)] - c * self.n
            self.parts.append(M.SchwarzModel(self.n, shapes, maps, fc, boxes, U, lam, mode))

    def apply(self, r):
        r = np.asarray(r)
        return np.concatenate([P.apply(r[c * self.n:(c + 1) * self.n]) for c, P in enumerate(self.parts)])

    def dense(self):
        return scipy.linalg.block_diag(*[P.dense() for P in self.parts])

"""The cases of the multigrid tests of MultipatchVectorSystem (tests/test_mpvec_mg_cpu.py, tests/test_mpvec_mg_gpu.py) and what
decides them.  A plain helper module: no GPU needed to import it.

- ``SWEEP_CASES``: the patterns of _mpvec_model.MPVEC_CASES, one per group width of with_csr_node_gs_kernel at 2 and at 3
  components.  The present blocks are those of the SpMV cases made symmetric: all four at nc = 2; at nc = 3 the diagonal, (0, 1)
  and (2, 0) with their transposed partners (1, 0) and (0, 2), so that the pair (1, 2) / (2, 1) is genuinely absent.
- ``BIG_CASE``: the L-shape at p = 1 (GW 4) whose largest colour has more nodes than one grid-stride pass of k_csr_node_gs covers
  at the block-count cap NB_NODE_GS_MAX (read from the source: _mpvec_mg_model.node_gs_pass_nodes).  First fit gives the bilinear
  pattern 4 colours of about a quarter of the nodes each (6 with the fixed sides), so n = 448 (604 k nodes) puts about 150 k nodes
  into the largest against 131 072 of one pass; the test asserts it.
- ``symmetric_patch_values``: per patch the values of every present block, the blocked patch matrix symmetric, the diagonal
  blocks' diagonals twice the absolute sum of the rest of their blocked row: every patch matrix, and so their glued sum, is
  strictly diagonally dominant, and every nc x nc diagonal block D of a node and every free sub-block of it has a condition number
  below 3.  The project's bound of the scalar sweep (RELAX_BOUND) therefore carries over.
- ``VCYCLE_CASES``: linear elasticity (mu = 1, lam = 2) on the L-shape (p = 2, n = 8, nc = 2, three levels; component 0 fixed on
  more sides than component 1) and on two cubes (p = 2, n = 4, nc = 3, two levels; the sides of _mpvec_model.CASE_SIDES).
"""
from typing import NamedTuple

import numpy as np
import scipy.sparse

import _mpvec_model as MV
import _solver_cases as sc

MU_LAM = dict(mu=1.0, lam=2.0)


def symmetric_present(present):
    return tuple(sorted(set(present) | {(q, p) for p, q in present}))


class SweepCase(NamedTuple):
    id: str
    base: MV.MPVecCase

    @property
    def nc(self):
        return self.base.nc

    @property
    def gw(self):
        return self.base.gw

    @property
    def domain(self):
        return self.base.mp.domain

    @property
    def present(self):
        return symmetric_present(self.base.present)

    def build(self):
        return self.base.build()


SWEEP_CASES = [SweepCase(c.id, c) for c in MV.MPVEC_CASES]
BIG_CASE = SweepCase('lshape_p1_n448_nc2', MV.MPVecCase('lshape_p1_n448_nc2', sc.MultipatchCase('lshape_p1_n448', 'lshape', 1, 448, 4), 2))


def sides_per_component(domain, nc):
    """Component 0 fixed on the first side of _mpvec_model.CASE_SIDES, the last component on the second, the middle one (nc = 3)
    nowhere: nodes on those sides have one fixed and one (or two) free components."""
    sides = MV.CASE_SIDES[domain]
    return [[sides[0]]] + [[] for _ in range(nc - 2)] + [[sides[1]]]


def symmetric_patch_values(patterns, present, nc, rng):
    """{(p, q): [values of patch k in the order of its pattern]} for the blocks `present` (closed under transposition)."""
    vals = {pq: [] for pq in present}
    for Sp in patterns:
        N = Sp.shape[0]
        blocks = {}
        for p in range(nc):
            for q in range(p, nc):
                if (p, q) not in vals:
                    continue
                B = scipy.sparse.csr_matrix((rng.uniform(-1.0, 1.0, Sp.nnz), Sp.indices, Sp.indptr), shape=(N, N))
                if p == q:
                    B = (0.5 * (B + B.T)).tocsr()
                blocks[(p, q)] = B
                if p != q:
                    blocks[(q, p)] = B.T.tocsr()
        rest = np.zeros((nc, N))                                   # the absolute sum of every blocked row without its diagonal entry
        for (p, q), B in blocks.items():
            rest[p] += np.asarray(abs(B).sum(axis=1)).ravel()
            if p == q:
                rest[p] -= np.abs(B.diagonal())
        on_diag = Sp.indices == np.repeat(np.arange(N), np.diff(Sp.indptr))
        assert on_diag.sum() == N
        for (p, q), B in blocks.items():
            B.sort_indices()
            assert np.array_equal(B.indptr, Sp.indptr) and np.array_equal(B.indices, Sp.indices)
            data = np.array(B.data, dtype=np.float64)
            if p == q:
                data[on_diag] = 2.0 * rest[p]
            vals[(p, q)].append(data)
    return vals


class VcycleCase(NamedTuple):
    id: str
    domain: str
    p: int
    n: int
    nc: int
    levels: int
    sides: tuple       # per component ((patch, bdspec), ...)
    values: tuple      # the Dirichlet value of every component (non-zero)

    def build(self):
        import _mpsolve_model as M
        return M.lshape(p=self.p, n=self.n) if self.domain == 'lshape' else sc.two_cubes(self.p, self.n)


_CUBES = MV.CASE_SIDES['cubes2']
VCYCLE_CASES = [
    VcycleCase('lshape_p2_n8_nc2', 'lshape', 2, 8, 2, 3, (((0, 'left'), (0, 'bottom'), (2, 'top')), ((0, 'left'),)), (0.01, -0.02)),
    VcycleCase('cubes2_p2_n4_nc3', 'cubes2', 2, 4, 3, 2, ((_CUBES[0], _CUBES[1]), (_CUBES[0],), (_CUBES[0],)), (0.01, -0.02, 0.005)),
]

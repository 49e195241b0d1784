"""Host model of the multigrid preconditioner of MultipatchVectorSystem (pyiga_amd/csrc/multigrid_block.hip
and the block hooks of multigrid.hip).  Host only; reuses _mg_model (colouring, prolongation, PCG) and _mg_cases (long double).

Vectors have nc * N entries, component-major: a *node* is a scalar dof I with its components x[p N + I].

- ``NodeSweep``: the sequential node-block Gauss-Seidel sweep in long double, a colour at a time (nodes of one colour never
  couple, so this is the sequential sweep in (colour, index) order): forward and backward, partially fixed nodes (the fixed
  components keep their entry, their column of the diagonal block goes to the right-hand side), absent blocks (zeros).
- ``node_sweep_loop``: the same sweep as a plain loop over the nodes with numpy.linalg.solve on the free sub-block (float64):
  what NodeSweep is checked against.
- ``BlockModel``: the V-cycle on given blocked level matrices with I_nc (x) P of _mg_model.global_prolongation.
- ``parse_node_gs_dispatch`` / ``node_gs_instances_outside_table`` / ``parse_node_gs_cap``: the dispatch table and the block-count
  cap of multigrid_block.hip.
"""
import os
import re

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import _mg_cases as mc
import _mg_model as G
import _solver_cases as sc

LD = np.longdouble
MULTIGRID_BLOCK_HIP = os.path.join(sc.ROOT, 'pyiga_amd', 'csrc', 'multigrid_block.hip')
TABLE = 'decltype(auto) with_csr_node_gs_kernel('


# ---------------------------------------------------------------------------------------------
# the source
def read_source(path=MULTIGRID_BLOCK_HIP):
    with open(path) as f:
        return f.read()


def parse_node_gs_dispatch(src):
    """{(label, GW, U, NC)} of the case lines of with_csr_node_gs_kernel that name k_csr_node_gs<GW, U, NC>."""
    body = sc._function_body(src, TABLE)
    out = set()
    for label, gw, u, nc in re.findall(r'(case \d+|default):[^\n]*?\bk_csr_node_gs<(\d+), (\d+), (\d+)>', body):
        out.add((None if label == 'default' else int(label.split()[1]), int(gw), int(u), int(nc)))
    return out


def node_gs_instances_outside_table(src):
    body = sc._function_body(src, TABLE)
    return re.findall(r'\bk_csr_node_gs\s*<[^>]*>', src.replace(body, ''))


def parse_node_gs_cap(src):
    """(BLOCK, NB_NODE_GS_MAX) of multigrid_block.hip."""
    return tuple(int(re.search(r'constexpr int %s = (\d+);' % name, src).group(1)) for name in ('BLOCK', 'NB_NODE_GS_MAX'))


def node_gs_pass_nodes(gw, src=None):
    """Nodes of one colour that one grid-stride pass of k_csr_node_gs covers at the largest grid."""
    block, cap = parse_node_gs_cap(read_source() if src is None else src)
    return cap * (block // gw)


# ---------------------------------------------------------------------------------------------
# colours of the nodes
def node_free(free, nc):
    """Per node: any component free (`free`: the mask over the nc * N blocked dofs)."""
    return np.asarray(free, dtype=bool).reshape(nc, -1).any(axis=0)


def node_colour_lists(indptr, indices, free, nc):
    """The nodes with a free component, colour after colour in ascending order (first fit on the scalar pattern)."""
    from pyiga_amd import solvers
    colour, _ = solvers.first_fit_colouring(indptr, indices, node_free(free, nc).astype(np.uint8))
    return mc.colour_lists(colour.astype(np.int64))


def scalar_pattern(A, nc):
    """The union of the patterns of the nc x nc blocks of the blocked matrix A (explicit zeros count)."""
    A = sp.csr_matrix(A)
    N = A.shape[0] // nc
    S = sp.csr_matrix((N, N))
    for p in range(nc):
        for q in range(nc):
            B = A[p * N:(p + 1) * N, q * N:(q + 1) * N].tocsr()
            S = S + sp.csr_matrix((np.ones(B.indices.size), B.indices, B.indptr), shape=(N, N))
    S = S.tocsr()
    S.sort_indices()
    return S


# ---------------------------------------------------------------------------------------------
# the sweep
def _solve_small(D, rhs):
    """Batched elimination without pivoting, in the order of the components: D (m, nc, nc), rhs (m, nc), any float type."""
    D, rhs = D.copy(), rhs.copy()
    nc = D.shape[1]
    for k in range(nc):
        for i in range(k + 1, nc):
            f = D[:, i, k] / D[:, k, k]
            D[:, i, k + 1:] -= f[:, None] * D[:, k, k + 1:]
            rhs[:, i] -= f * rhs[:, k]
    y = np.zeros_like(rhs)
    for k in range(nc - 1, -1, -1):
        t = rhs[:, k].copy()
        for j in range(k + 1, nc):
            t -= D[:, k, j] * y[:, j]
        y[:, k] = t / D[:, k, k]
    return y


class NodeSweep:
    """The node-block Gauss-Seidel sweep of the blocked matrix A (nc components) in long double.  `colours`: the nodes of every
    colour; `free`: the mask over the blocked dofs.  Every node of a colour gets
    x_F[I] = D_FF^-1 (b_F[I] - sum_{J != I} sum_q A_Fq[I,J] x_q[J] - sum_{q fixed at I} D_Fq x_q[I])."""

    def __init__(self, A, nc, colours, free):
        Al = mc._ld(A)
        self.nc, self.N = nc, A.shape[0] // nc
        N = self.N
        self.colours = colours
        self.free = np.asarray(free, dtype=bool).reshape(nc, N)
        self.D = np.array([[Al[p * N:(p + 1) * N, q * N:(q + 1) * N].diagonal() for q in range(nc)] for p in range(nc)])    # (nc, nc, N)
        self.rows = [Al[np.concatenate([p * N + r for p in range(nc)])] for r in colours]

    def sweep(self, x, b, kind='forward'):
        nc, N = self.nc, self.N
        x = np.array(x, dtype=LD)
        b = np.asarray(b, dtype=LD)
        k = len(self.colours)
        seq = {'forward': list(range(k)), 'backward': list(range(k))[::-1]}
        seq['symmetric'] = seq['forward'] + seq['backward']
        for c in seq[kind]:
            r = self.colours[c]
            m = r.size
            fr = self.free[:, r].T                                   # (m, nc)
            D = np.moveaxis(self.D[:, :, r], 2, 0).copy()            # (m, nc, nc)
            xn = np.stack([x[q * N + r] for q in range(nc)], axis=1)
            s = (self.rows[c] @ x).reshape(nc, m).T                  # all of row (p, I), the node's own block included
            rhs = np.stack([b[p * N + r] for p in range(nc)], axis=1) - (s - np.einsum('mpq,mq->mp', D, xn))
            # the fixed components keep their entry: their columns to the right-hand side, their rows and columns the identity's
            fx = ~fr
            rhs = rhs - np.einsum('mpq,mq->mp', D, np.where(fx, xn, LD(0)))
            eye = np.broadcast_to(np.eye(nc, dtype=LD), D.shape)
            both = fr[:, :, None] & fr[:, None, :]
            D = np.where(both, D, np.where(fx[:, :, None] & fx[:, None, :], eye, LD(0)))
            rhs = np.where(fr, rhs, LD(0))
            y = _solve_small(D, rhs)
            for p in range(nc):
                x[p * N + r[fr[:, p]]] = y[fr[:, p], p]
        return x


def node_sweep_loop(A, nc, order, free, x, b):
    """One sweep over the nodes `order`, one after the other: numpy.linalg.solve on the free sub-block of the node's diagonal
    block, float64.  The plain statement of what NodeSweep computes a colour at a time."""
    A = sp.csr_matrix(A)
    N = A.shape[0] // nc
    free = np.asarray(free, dtype=bool)
    x = np.array(x, dtype=float)
    for I in order:
        dofs = np.arange(nc) * N + I
        F = dofs[free[dofs]]
        if not F.size:
            continue
        DFF = A[F][:, F].toarray()
        r = b[F] - A[F] @ x + DFF @ x[F]                            # everything but the free part of the node's own block
        x[F] = np.linalg.solve(DFF, r)
    return x


# ---------------------------------------------------------------------------------------------
# the V-cycle
class BlockModel:
    """The V-cycle on the blocked matrices `As` (all dofs of every level, the finest first) of nc components over the
    multipatches `MPs` with the blocked fixed dofs `fixed` of every level.  Vectors are over the free dofs of the finest level
    in ascending (blocked) order.  `orders`: per level the nodes in the smoother's order (default: first fit on the union of
    the blocks' patterns)."""

    def __init__(self, As, MPs, fixed, nc, smooth_steps=1, orders=None):
        self.nu, self.nc = smooth_steps, nc
        self.levels = []
        I = sp.identity(nc, format='csr')
        for l, (A, MP, fx) in enumerate(zip(As, MPs, fixed)):
            A = sp.csr_matrix(A)
            A.sort_indices()
            N = MP.numdofs
            assert A.shape == (nc * N, nc * N)
            free = np.ones(nc * N, dtype=bool)
            free[np.asarray(fx, dtype=np.int64)] = False
            fr = np.flatnonzero(free)
            if orders is None:
                S = scalar_pattern(A, nc)
                order = np.concatenate(node_colour_lists(S.indptr, S.indices, free, nc) + [np.zeros(0, dtype=np.int64)])
            else:
                order = np.asarray(orders[l], dtype=np.int64)
            pos = np.full(N, -1, dtype=np.int64)
            pos[order] = np.arange(order.size)
            key = pos[fr % N]                                        # the place of every free dof's node in the sweep
            assert (key >= 0).all()
            Af = A[fr][:, fr].tocsr()
            C = Af.tocoo()
            low = sp.csr_matrix((C.data[key[C.row] >= key[C.col]], (C.row[key[C.row] >= key[C.col]], C.col[key[C.row] >= key[C.col]])),
                                shape=Af.shape)
            upp = sp.csr_matrix((C.data[key[C.row] <= key[C.col]], (C.row[key[C.row] <= key[C.col]], C.col[key[C.row] <= key[C.col]])),
                                shape=Af.shape)
            self.levels.append(dict(A=A, Af=Af, fr=fr, free=free, order=order, MP=MP, low=spla.splu(low.tocsc()),
                                    upp=spla.splu(upp.tocsc())))
        for a, b in zip(self.levels[:-1], self.levels[1:]):
            Pfull = sp.kron(I, G.global_prolongation(a['MP'], b['MP'])[0], format='csr')
            a['Pfull'] = Pfull
            a['P'] = Pfull[a['fr']][:, b['fr']].tocsr()
        last = self.levels[-1]
        inv = np.linalg.inv(last['Af'].toarray()) if last['fr'].size else np.zeros((0, 0))
        last['Ainv'] = 0.5 * (inv + inv.T)

    def _smooth(self, L, x, b, forward):
        return x + (L['low'] if forward else L['upp']).solve(b - L['Af'] @ x)

    def vcycle(self, b, l=0):
        L = self.levels[l]
        if l == len(self.levels) - 1:
            return L['Ainv'] @ b
        x = np.zeros_like(b)
        for _ in range(self.nu):
            x = self._smooth(L, x, b, True)
        x = x + L['P'] @ self.vcycle(L['P'].T @ (b - L['Af'] @ x), l + 1)
        for _ in range(self.nu):
            x = self._smooth(L, x, b, False)
        return x

    def apply_full(self, r):
        """The V-cycle on a vector of all blocked dofs of the finest level (fixed entries ignored / 0)."""
        L = self.levels[0]
        z = np.zeros(L['A'].shape[0])
        z[L['fr']] = self.vcycle(np.asarray(r, dtype=float)[L['fr']])
        return z


def block_2x2(K, Mm):
    """[[2K + M, K/2], [K/2, 2K + M]]: a symmetric positive definite 2-component matrix from a scalar stiffness and mass matrix."""
    return sp.bmat([[2 * K + Mm, 0.5 * K], [0.5 * K, 2 * K + Mm]], format='csr')

"""numpy model of the device solves of vector-valued forms (solvers.VectorFormSystem, igx_solver_create_block in
pyiga_amd/csrc/solve.hip), and the cases that run every block SpMV instantiation.

- ``BlockKronModel``: the block-diagonal preconditioner diag(P_0, .., P_{nc-1}) on the blocked vectors (component-major, nc * N
  entries), P_c the fast-diagonalization inverse (x)U_k . D^-1 . (x)U_k^T on the free box of component c.
- ``pcg``: preconditioned CG as the device runs it (the stop ||r|| <= tol ||r0|| tested before every iteration).
- ``VEC_CASES``: a case per group width of k_block_spmv and per number of components, each past one grid of scalar rows
  (tests/_solver_cases.py: NB_SPMV_MAX * BLOCK / GW); tests/test_vecsolve_cpu.py checks that they reach every width,
  tests/test_vecsolve_gpu.py runs them.
"""
import re
from typing import NamedTuple

import numpy as np

import _solver_cases as sc

ELASTICITY = '(2*mu*inner(0.5*(grad(u)+grad(u).T), 0.5*(grad(v)+grad(v).T)) + lam*div(u)*div(v)) * dx'
GRAD_DIV = '(div(u)*div(v) + inner(u, v)) * dx'
# vector reaction-diffusion with a one-way coupling: blocks (0, 0), (0, 1) and the other diagonal ones present, the rest absent
COUPLED = {2: '(inner(grad(u), grad(v)) + inner(as_matrix([[2, 1], [0, 1]]).dot(u), v)) * dx',
           3: '(inner(grad(u), grad(v)) + inner(as_matrix([[2, 1, 0], [0, 1, 0], [0, 0, 1]]).dot(u), v)) * dx'}
NONSYM = '(inner(as_matrix([[2, 1], [0, 0]]).dot(u), v) + inner(grad(u), grad(v))) * dx'

# the (GW, U, NC) instantiations of k_block_spmv
BLOCK_SPMV_INSTANCES = {(gw, 4, 2) for gw in sc.GWS} | {(gw, 2, 3) for gw in sc.GWS}
TABLE = 'decltype(auto) with_block_spmv_kernel('


def bfuns(nc):
    return [('u', nc), ('v', nc)]


def parse_block_dispatch(src):
    """{(label, GW, U, NC)} of the case lines of with_block_spmv_kernel that name k_block_spmv<GW, U, NC>."""
    body = sc._function_body(src, TABLE)
    out = set()
    for label, gw, u, nc in re.findall(r'(case \d+|default):[^\n]*?\bk_block_spmv<(\d+), (\d+), (\d+)>', body):
        out.add((None if label == 'default' else int(label.split()[1]), int(gw), int(u), int(nc)))
    return out


def block_instances_outside_table(src):
    body = sc._function_body(src, TABLE)
    return re.findall(r'\bk_block_spmv\s*<[^>]*>', src.replace(body, ''))


class VecCase(NamedTuple):
    id: str
    patch: sc.PatchCase
    nc: int

    @property
    def gw(self):
        return self.patch.gw

    def kvs(self):
        return self.patch.kvs()


# every width past one grid of scalar rows (the first five structured cases of the scalar SpMV), at 2 and 3 components
VEC_CASES = [VecCase('%s_nc%d' % (c.id, nc), c, nc) for c in sc.PATCH_CASES[:5] for nc in (2, 3)]


class BlockKronModel:
    """diag(P_0, .., P_{nc-1}) on blocked vectors.  `factors`: per component (lo, hi, U, lam, mode) as
    VectorFormSystem.kron_factors() gives them (mode 1: D = sum of the lam_k, 2: their product)."""

    def __init__(self, ndofs, factors):
        self.ndofs = tuple(int(n) for n in ndofs)
        self.N = int(np.prod(self.ndofs))
        self.factors = factors

    def apply(self, r):
        z = np.zeros(self.N * len(self.factors))
        for c, (lo, hi, U, lam, mode) in enumerate(self.factors):
            box = tuple(slice(a, b) for a, b in zip(lo, hi))
            x = np.asarray(r[c * self.N:(c + 1) * self.N]).reshape(self.ndofs)[box]
            for k, u in enumerate(U):
                x = np.moveaxis(np.tensordot(u.T, x, axes=(1, k)), 0, k)
            D = lam[0]
            for l in lam[1:]:
                D = np.add.outer(D, l) if mode == 1 else np.multiply.outer(D, l)
            x = x / D
            for k, u in enumerate(U):
                x = np.moveaxis(np.tensordot(u, x, axes=(1, k)), 0, k)
            zc = np.zeros(self.ndofs)
            zc[box] = x
            z[c * self.N:(c + 1) * self.N] = zc.ravel()
        return z


def pcg(A, b, M=None, tol=1e-8, maxiter=1000):
    """CG on A x = b from x = 0 with the preconditioner M (a callable or None): x, iterations, converged."""
    M = M if M is not None else (lambda y: y.copy())
    x = np.zeros_like(b)
    r = b.copy()
    stop = tol * np.linalg.norm(b)
    z = M(r)
    p = z.copy()
    rz = r @ z
    it = 0
    while np.linalg.norm(r) > stop and it < maxiter:
        it += 1
        q = A @ p
        alpha = rz / (p @ q)
        x += alpha * p
        r -= alpha * q
        z = M(r)
        rz, rz_old = r @ z, rz
        p = z + (rz / rz_old) * p
    return x, it, bool(np.linalg.norm(r) <= stop)


def side_dofs(kvs, sides, ncomp):
    """The blocked indices of the dofs of every component on the given sides ((axis, 0 | 1), ...)."""
    from pyiga_amd import assemble
    N = int(np.prod([kv.numdofs for kv in kvs]))
    one = np.unique(np.concatenate([assemble.boundary_dofs(kvs, s, ravel=True) for s in sides]))
    return np.concatenate([one + c * N for c in range(ncomp)])

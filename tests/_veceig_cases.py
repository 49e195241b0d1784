"""The cases that run every instantiation of the vector block product k_block_spmm2 (pyiga_amd/csrc/solve_eig.hip; DESIGN.md
section 27), and what decides them.

A plain helper module (no GPU needed to import it): tests/test_veceig_cpu.py checks on the host that the dispatch reaches every
``(GW, MB, NM, NC)`` and that the table does; tests/test_veceig_kernels_gpu.py runs the cases.

- The group width GW of a patch is ``spmv_gw(patch_maxlen(kvs))``, the row stride MB of a block of m columns
  ``eig_width(m)``, NM is 2 for ``block_products`` and 1 for ``block_product``, NC the number of components of the form.
- One group serves a *scalar* row: a pass of the kernel covers ``spmm_pass_rows(gw)`` scalar rows, whatever NC is.
"""
import re
from typing import NamedTuple

import _eig_cases as EC
import _solver_cases as SC
from _eig_cases import COLUMNS, GWS, WIDTHS, eig_width, spmm_pass_rows     # noqa: F401
from _solver_cases import PatchCase, patch_maxlen, spmv_gw     # noqa: F401

NCS = (2, 3)
INSTANCES = {(gw, mb, nm, nc) for gw in GWS for mb in WIDTHS for nm in (1, 2) for nc in NCS}

# every block present, the diagonal ones distinct, and the off-diagonal ones not symmetric in themselves (A_qp = A_pq^T != A_pq):
# exchanged components, a transposed block or a block read twice all change the product
FULL = {2: '(inner(grad(u), grad(v)) + inner(as_matrix([[2, 1], [1, 3]]).dot(u), v) + grad(u)[1, 0]*v[0] + u[0]*grad(v)[1, 0]) * dx',
        3: '(inner(grad(u), grad(v)) + inner(as_matrix([[2, 1, 0.5], [1, 3, 0.25], [0.5, 0.25, 4]]).dot(u), v) '
           '+ grad(u)[1, 0]*v[0] + u[0]*grad(v)[1, 0] + grad(u)[2, 1]*v[0] + u[0]*grad(v)[2, 1]) * dx'}
# the plain vector Laplacian (shifted: there is a case without fixed dofs): the off-diagonal blocks are absent
LAPLACE = '(inner(grad(u), grad(v)) + inner(u, v)) * dx'
# the diagonal blocks and one symmetric pair of off-diagonal ones: the form of the cases past one pass
PAIR = {2: '(inner(grad(u), grad(v)) + inner(as_matrix([[2, 1], [1, 3]]).dot(u), v)) * dx',
        3: '(inner(grad(u), grad(v)) + inner(as_matrix([[2, 1, 0], [1, 3, 0], [0, 0, 4]]).dot(u), v)) * dx'}


def bfuns(nc):
    return [('u', nc), ('v', nc)]


# ---------------------------------------------------------------------------------------------
# parsing the solver source (_solver_cases.read_source)
GW_TABLE = 'decltype(auto) with_block_spmm2_gw('
MB_TABLE = 'decltype(auto) with_block_spmm2_mb('
TABLE = 'decltype(auto) with_block_spmm2_kernel('


def parse_block_spmm_dispatch(src):
    """{(GW, MB, NM, NC)}: the instantiations of k_block_spmm2 that with_block_spmm2_kernel reaches (it names the (NM, NC) of
    with_block_spmm2_mb, which names the widths of with_block_spmm2_gw, which names the group widths), and the {(label, GW)}
    of the group-width switch."""
    gws = set()
    for label, gw in re.findall(r'(case \d+|default):[^\n]*?\bk_block_spmm2<(\d+), MB, \d+ / MB, NC, NM>', SC._function_body(src, GW_TABLE)):
        gws.add((None if label == 'default' else int(label.split()[1]), int(gw)))
    mbs = set()
    for label, mb in re.findall(r'(case \d+|default):[^\n]*?with_block_spmm2_gw<(\d+), NM, NC>', SC._function_body(src, MB_TABLE)):
        mbs.add((None if label == 'default' else int(label.split()[1]), int(mb)))
    pairs = {(int(nm), int(nc)) for nm, nc in re.findall(r'with_block_spmm2_mb<(\d+), (\d+)>', SC._function_body(src, TABLE))}
    return {(gw, mb, nm, nc) for _, gw in gws for _, mb in mbs for nm, nc in pairs}, gws, mbs


def block_spmm_outside_tables(src):
    """Template argument lists of k_block_spmm2 written anywhere but in with_block_spmm2_gw (the kernel's definition has none)."""
    src = src.replace(SC._function_body(src, GW_TABLE), '')
    return re.findall(r'\bk_block_spmm2\s*<[^>]*>', src)


# ---------------------------------------------------------------------------------------------
# the cases
class VecBlockCase(NamedTuple):
    patch: PatchCase
    nc: int
    columns: tuple     # m of the blocks run on it

    @property
    def id(self):
        return '%s_nc%d' % (self.patch.id, self.nc)


# the seven small patches of the scalar block product, one per group width, with 2 and with 3 components whatever the dimension
# of the patch, and every m of COLUMNS: every (GW, MB, NM, NC)
SMALL_CASES = [VecBlockCase(c.patch, nc, COLUMNS) for c in EC.SMALL_CASES for nc in NCS]

# one patch past the pass bound per group width, at one width each; two of them with 2 components, the others with 3
_WRAP = {c.gw: c for c in SC.PATCH_CASES[:5]}
WRAP_CASES = [VecBlockCase(_WRAP[4], 2, (3,)), VecBlockCase(_WRAP[8], 3, (8,)), VecBlockCase(_WRAP[16], 2, (13,)),
              VecBlockCase(_WRAP[32], 3, (4,)), VecBlockCase(_WRAP[64], 3, (5,))]

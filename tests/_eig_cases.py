"""The cases that run every instantiation of the block kernels of the eigen-solver (pyiga_amd/csrc/solve_eig.hip), and what decides
them.

A plain helper module (no GPU needed to import it): tests/test_eig_cpu.py checks on the host that the table reaches every
``(GW, MB)`` instantiation of k_spmm2 and every compiled width of the other block kernels and wraps every grid-stride loop;
tests/test_eig_kernels_gpu.py runs the cases.

- The group width GW of a patch is ``_solver_cases.spmv_gw(patch_maxlen(kvs))``: the block product takes k_spmv's row-to-group
  map.  The row stride MB of a block of m columns is the smallest compiled width >= m (``solvers.eig_width``).
- ``spmm_pass_rows(gw)``: one grid-stride pass of k_spmm2 covers at most NB_SPMV_MAX blocks of BLOCK / GW rows.
- ``gram_pass_rows()``: k_gram runs at most NB_GRAM blocks of GR_RC rows a pass.
- ``vec_pass_rows()``: k_block_comb (one thread per row) runs at most NB_VEC blocks of BLOCK rows a pass; k_resid and
  k_block_scale (one thread per entry) NB_VEC * BLOCK / MB rows, which is fewer.
"""
import re
from typing import NamedTuple

import _solver_cases as SC
from _solver_cases import BLOCK, NB_SPMV_MAX, NB_VEC, PatchCase, patch_maxlen, spmv_gw     # noqa: F401

WIDTHS = (4, 8, 16)
GWS = SC.GWS
NB_GRAM = 256
GR_RC = 32
# columns of the blocks every small case is run with: each width is met from below, exactly and (4, 8) from above
COLUMNS = (1, 3, 4, 5, 8, 13, 16)


def eig_width(m):
    return next(w for w in WIDTHS if m <= w)


def spmm_pass_rows(gw):
    return NB_SPMV_MAX * (BLOCK // gw)


def gram_pass_rows():
    return NB_GRAM * GR_RC


def vec_pass_rows():
    return NB_VEC * BLOCK


# ---------------------------------------------------------------------------------------------
# parsing the solver source (_solver_cases.read_source)
def parse_constants(src):
    out = {}
    for name in ('NB_GRAM', 'GR_RC'):
        m = re.search(r'constexpr int %s = (\d+);' % name, src)
        out[name] = int(m.group(1)) if m else None
    return out


def parse_spmm_dispatch(src):
    """{(GW, MB, NM)}: the instantiations of k_spmm2 the two dispatch functions reach (with_spmm2_kernel names the (MB, NM) of
    with_spmm2_gw, which names the group widths), and the {(label, GW)} of the group-width switch."""
    gw_body = SC._function_body(src, 'decltype(auto) with_spmm2_gw(')
    gws = set()
    for label, gw in re.findall(r'(case \d+|default):[^\n]*?\bk_spmm2<(\d+), MB, \d+ / MB, NM>', gw_body):
        gws.add((None if label == 'default' else int(label.split()[1]), int(gw)))
    body = SC._function_body(src, 'decltype(auto) with_spmm2_kernel(')
    pairs = {(int(mb), int(nm)) for mb, nm in re.findall(r'with_spmm2_gw<(\d+), (\d+)>', body)}
    return {(gw, mb, nm) for _, gw in gws for mb, nm in pairs}, gws


def spmm_outside_tables(src):
    """Template argument lists of k_spmm2 written anywhere but in with_spmm2_gw (the kernel's own definition has none)."""
    src = src.replace(SC._function_body(src, 'decltype(auto) with_spmm2_gw('), '')
    return re.findall(r'\bk_spmm2\s*<[^>]*>', src)


def parse_widths(src, kernel):
    """The widths `kernel<MB>` is launched with."""
    return {int(w) for w in re.findall(r'\b%s<(\d+)><<<' % kernel, src)}


# ---------------------------------------------------------------------------------------------
# the cases
class BlockCase(NamedTuple):
    patch: PatchCase
    columns: tuple     # m of the blocks run on it

    @property
    def id(self):
        return self.patch.id


# small patches, one per group width, run with every m of COLUMNS (so with every width): every (GW, MB) of k_spmm2
SMALL_CASES = [
    BlockCase(PatchCase('2d_p1_n9x7', ((1, 9, 1), (1, 7, 1)), 4), COLUMNS),
    BlockCase(PatchCase('2d_p2_mult2', ((2, 12, 2), (1, 10, 1)), 4), COLUMNS),          # repeated knots on axis 0
    BlockCase(PatchCase('2d_p2_n8', ((2, 8, 1), (2, 6, 1)), 8), COLUMNS),
    BlockCase(PatchCase('2d_p3_n7', ((3, 7, 1), (3, 6, 1)), 16), COLUMNS),
    BlockCase(PatchCase('3d_mixed_mult', ((2, 7, 1), (3, 6, 2), (1, 9, 1)), 16), COLUMNS),     # 3D, double knots on axis 1
    BlockCase(PatchCase('3d_p2_n4', ((2, 4, 1), (2, 5, 1), (2, 3, 1)), 32), COLUMNS),
    BlockCase(PatchCase('3d_p3_n4', ((3, 4, 1), (3, 5, 1), (3, 4, 1)), 64), COLUMNS),
]

# one patch past the pass bound of k_spmm2 per group width (those of the SpMV tests), each at one width
_WRAP = {c.gw: c for c in SC.PATCH_CASES[:5]}
WRAP_CASES = [BlockCase(_WRAP[4], (3,)), BlockCase(_WRAP[8], (8,)), BlockCase(_WRAP[16], (13,)), BlockCase(_WRAP[32], (4,)),
              BlockCase(_WRAP[64], (5,))]


class RowsCase(NamedTuple):
    id: str
    axes: tuple        # (p, n, mult) per axis
    columns: tuple

    def kvs(self):
        return PatchCase(self.id, self.axes, 0).kvs()

    def rows(self):
        out = 1
        for kv in self.kvs():
            out *= kv.numdofs
        return out


# gram, combine, residuals and the preconditioners: fewer rows than one block, a row count that is no multiple of 256, and more
# rows than NB_VEC x BLOCK (which wraps every one of their loops); every width among the columns
ROWS_CASES = [
    RowsCase('rows_4x5', ((1, 3, 1), (1, 4, 1)), (2, 7, 11)),                # 20 rows
    RowsCase('rows_23x31', ((2, 21, 1), (1, 30, 1)), (4, 5, 16)),            # 713 rows
    RowsCase('rows_514x513', ((1, 513, 1), (1, 512, 1)), (3, 8, 13)),        # 263 682 rows > 262 144
]

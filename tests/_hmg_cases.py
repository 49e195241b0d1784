"""Case tables of the local-multigrid tests (tests/test_hmg_cpu.py, tests/test_hmg_gpu.py, tests/test_hmg_kernels_gpu.py) and of
tests/golden/make_golden_hmg.py.  The spaces are those of tests/_hier_cases.py; like that table this one is written against the
interface the reference and this package share.
"""
import numpy as np
import scipy.sparse

import _hier_cases as hc

# the spaces whose index sets and prolongators are compared with the reference
SPACE_CASES = ('hb2', 'hb2p1', 'hb2d', 'nonuni', 'thb2', 'thb2d', 'thb2inf', 'thb_aniso', 'hb3', 'thb3')
FAMILIES = ('new', 'trunc', 'func_supp', 'cell_supp')

# (case, strategy, smoother): stiffness, right-hand side f_rhs, all sides Dirichlet, tol 1e-8, two smoothing steps
SOLVE_ROWS = (
    ('hb2', 'cell_supp', 'gs'),
    ('hb2', 'func_supp', 'symmetric_gs'),
    ('thb2inf', 'cell_supp', 'gs'),
    ('thb2inf', 'trunc', 'symmetric_gs'),
    ('thb2', 'cell_supp', 'gs'),
    ('thb2d', 'func_supp', 'gs'),
    ('thb_aniso', 'cell_supp', 'symmetric_gs'),
    ('thb3', 'cell_supp', 'gs'),
    ('hb3', 'new', 'gs'),
)
TOL = 1e-8
SMOOTH_STEPS = 2
CG_ROW = ('hb2d', 'func_supp', 'gs')          # slow as a stationary iteration: the case for CG
SYSTEM_CASE = 'thb2inf'


def row_key(row):
    return '%s_%s_%s' % row


def golden_matrix(G, name):
    """The matrix `<name>_A` of golden_hier.npz (symmetric ones are stored by their upper triangle) as CSR."""
    if name + '_Au_data' in G:
        key = name + '_Au'
        U = scipy.sparse.csr_matrix((G[key + '_data'], G[key + '_indices'].astype(np.int32), G[key + '_indptr']), shape=tuple(G[key + '_shape']))
        A = U + scipy.sparse.triu(U, 1).T
    else:
        key = name + '_A'
        A = scipy.sparse.csr_matrix((G[key + '_data'], G[key + '_indices'].astype(np.int32), G[key + '_indptr']), shape=tuple(G[key + '_shape']))
    A = scipy.sparse.csr_matrix(A)
    A.sort_indices()
    return A


def build(bspline, HSpace, name):
    return hc.build(bspline, HSpace, name)[0]


def pack_family(fam, dim):
    """An index-set family (per virtual level, per level, a sequence of multi-index tuples) as rows (virtual level, level,
    multi-index) in the order given."""
    rows = [(lv, i) + tuple(int(t) for t in mi) for lv, per in enumerate(fam) for i, lst in enumerate(per) for mi in lst]
    return np.array(rows, dtype=np.int32).reshape(-1, 2 + dim)


def pack_lists(lists):
    """A list of index arrays as (concatenated, offsets)."""
    lists = [np.asarray(a, dtype=np.int64).ravel() for a in lists]
    return (np.concatenate(lists) if lists else np.zeros(0, dtype=np.int64)).astype(np.int32), np.concatenate(([0], np.cumsum([a.size for a in lists]))).astype(np.int32)


def unpack_lists(flat, off):
    return [np.asarray(flat[off[k]:off[k + 1]], dtype=np.int64) for k in range(len(off) - 1)]

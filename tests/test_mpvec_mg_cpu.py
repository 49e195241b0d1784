"""Host checks of the multigrid preconditioner of MultipatchVectorSystem: the dispatch table of
pyiga_amd/csrc/multigrid_block.hip, the header and the library, and the model of tests/_mpvec_mg_model.py on block matrices built
from the oracle's scalar level matrices -- the algorithm the kernel implements is shown to be symmetric and h-robust before any
device run.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import _mg_model as G
import _mp_eig_cases as MC
import _mpsolve_model as M
import _mpvec_mg_cases as VC
import _mpvec_mg_model as VM
import _mpvec_model as MV
import _solver_cases as sc

ROOT = sc.ROOT
CSRC = os.path.join(ROOT, 'pyiga_amd', 'csrc')
# component 0 is fixed on more sides than component 1
SIDES = ([(0, 'left'), (0, 'bottom'), (2, 'top')], [(0, 'left')])


@pytest.fixture(scope='module')
def src():
    return VM.read_source()


def test_node_gs_dispatch_table_names_exactly_the_ten_instantiations(src):
    lines = VM.parse_node_gs_dispatch(src)
    assert len(lines) == 10
    assert {(gw, u, nc) for _, gw, u, nc in lines} == MV.CSR_BLOCK_SPMV_INSTANCES
    for nc in (2, 3):
        labels = {label: gw for label, gw, _, n in lines if n == nc}
        assert labels == {64: 64, 32: 32, 16: 16, 8: 8, None: 4}, (nc, labels)


def test_no_node_gs_instance_outside_the_table(src):
    assert VM.node_gs_instances_outside_table(src) == []
    for fn in sorted(os.listdir(CSRC)):
        if fn.endswith(('.hip', '.h')) and fn != 'multigrid_block.hip':
            with open(os.path.join(CSRC, fn)) as f:
                assert not re.search(r'\bk_csr_node_gs\s*<', f.read()), fn


def test_block_count_cap_is_a_named_constant(src):
    block, cap = VM.parse_node_gs_cap(src)
    assert block == 256 and cap >= 1
    assert re.search(r'std::min<long long>\(NB_NODE_GS_MAX,', src)
    assert VM.node_gs_pass_nodes(4, src) == cap * 64
    # the wrap case is sized from it
    n = VC.BIG_CASE.base.mp.n
    assert 3 * n * n / 4 > VM.node_gs_pass_nodes(VC.BIG_CASE.gw, src)


def test_header_declares_and_library_exports_the_block_calls():
    from pyiga_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'igx.h')).read()
    names = ('igx_solver_set_block_mg_smoother', 'igx_solver_set_block_mg_coarse', 'igx_solver_set_block_mg_inverse')
    assert 'igx_solver_set_block_mg_smoother(igx_solver *solver, const int32_t *colour, int smooth_steps);' in hdr
    assert 'igx_solver_set_block_mg_coarse(igx_solver *solver, igx_solver *coarse, const double *const *P, const double *mult);' in hdr
    assert 'igx_solver_set_block_mg_inverse(igx_solver *solver, const double *inv, int64_t m);' in hdr
    bound = {name for name, _, _ in _lib.SYMBOLS}
    nm = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True).stdout
    cdll = _lib.load()
    for name in names:
        assert name in bound and hasattr(cdll, name) and re.search(r'\bT %s\b' % name, nm), name
    assert _lib.MPVEC_PRECONDS['mg'] == _lib.IGX_PRECOND_MG
    # null handles are argument errors, not crashes
    assert cdll.igx_solver_set_block_mg_smoother(None, None, 1) == _lib.IGX_ERR_ARG
    assert cdll.igx_solver_set_block_mg_inverse(None, None, 1) == _lib.IGX_ERR_ARG


# ---------------------------------------------------------------------------------------------
# the model on block matrices from the oracle's scalar level matrices of the L-shape at p = 2
_LEVELS = {}


def block_levels(oracle, n, nlev):
    """(As, MPs, fixed) of `nlev` levels: [[2K + M, K/2], [K/2, 2K + M]] of the oracle's stiffness and mass matrices."""
    if (n, nlev) not in _LEVELS:
        geos = MC.oracle_geos(oracle, 'lshape')
        Ks, MPs, _ = G.oracle_levels(oracle, M.lshape, geos, 2, n, nlev, SIDES[1])
        As, fixed = [], []
        for k, (K, MP) in enumerate(zip(Ks, MPs)):
            Mm = MC.oracle_sums(oracle, MP, 'lshape', 2, n >> k, kinds=('mass',))[0]
            As.append(VM.block_2x2(K, Mm))
            fixed.append(MV.blocked_fixed(MP, SIDES, 2))
        _LEVELS[(n, nlev)] = (As, MPs, fixed)
    return _LEVELS[(n, nlev)]


def test_model_sweep_is_the_loop_over_nodes_in_colour_order(oracle):
    As, MPs, fixed = block_levels(oracle, 8, 2)
    A, N = As[0], MPs[0].numdofs
    free = np.ones(2 * N, dtype=bool)
    free[fixed[0]] = False
    nodes = VM.node_free(free, 2)
    fr2 = free.reshape(2, N)
    assert np.any(fr2.any(axis=0) & ~fr2.all(axis=0)) and np.any(~nodes)       # partially and wholly fixed nodes
    S = VM.scalar_pattern(A, 2)
    lists = VM.node_colour_lists(S.indptr, S.indices, free, 2)
    colour = G.first_fit(S.indptr, S.indices, nodes)
    assert np.array_equal(np.concatenate(lists), G.colour_order(colour))       # (the library's colouring is first fit)
    for r in lists:                                                            # nodes of one colour never couple
        assert S[r][:, r].nnz == r.size
    rng = np.random.default_rng(5)
    x0, b = rng.standard_normal(2 * N), rng.standard_normal(2 * N)
    sweep = VM.NodeSweep(A, 2, lists, free)
    order = np.concatenate(lists)
    for kind, seq in (('forward', order), ('backward', order[::-1])):
        x = sweep.sweep(x0, b, kind)
        ref = VM.node_sweep_loop(A, 2, seq, free, x0, b)
        d = float(np.abs(x - ref).max() / np.abs(ref).max())
        assert d <= 1e-13, (kind, d)
        assert np.array_equal(np.asarray(x, dtype=float)[~free], x0[~free])    # fixed components keep their entry
    # an absent block pair is a pair of zero blocks
    B = sp.bmat([[A[:N, :N], None], [None, A[N:, N:]]], format='csr')
    x = VM.NodeSweep(B, 2, lists, free).sweep(x0, b)
    ref = VM.node_sweep_loop(B, 2, order, free, x0, b)
    assert float(np.abs(x - ref).max() / np.abs(ref).max()) <= 1e-13


def test_model_sweeps_are_adjoint_and_the_cycle_is_symmetric(oracle):
    """B_fwd = (D + L)^-1 and B_bwd = (D + U)^-1 with the node blocks in D: <B_fwd x, y> = <x, B_bwd y> for a symmetric matrix, and
    the V-cycle built from them is symmetric.  Rounding level: 64 eps times the sum of the magnitudes of the terms."""
    model = VM.BlockModel(*block_levels(oracle, 16, 3), 2)
    L = model.levels[0]
    n = L['fr'].size
    rng = np.random.default_rng(2)
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    zero = np.zeros(n)
    Bx, By = model._smooth(L, zero, x, True), model._smooth(L, zero, y, False)
    a, b = Bx @ y, x @ By
    assert abs(a - b) <= 64 * 2.0 ** -52 * (np.abs(Bx) @ np.abs(y) + np.abs(x) @ np.abs(By)), (a, b)
    Vx, Vy = model.vcycle(x), model.vcycle(y)
    a, b = Vx @ y, x @ Vy
    assert abs(a - b) <= 64 * 2.0 ** -52 * (np.abs(Vx) @ np.abs(y) + np.abs(x) @ np.abs(Vy)), (a, b)
    assert x @ Vx > 0
    # the block smoother of the model is the sweep
    N = model.levels[0]['MP'].numdofs
    xf, bf = np.zeros(2 * N), np.zeros(2 * N)
    bf[L['fr']] = x
    ref = VM.node_sweep_loop(L['A'], 2, L['order'], L['free'], xf, bf)
    assert np.abs(ref[L['fr']] - Bx).max() <= 1e-12 * np.abs(Bx).max()


def test_model_pcg_count_is_h_robust(oracle):
    """PCG with V(1,1) on a random right-hand side (seed 0, tol 1e-8), the coarsest level of 4 spans per patch: the count at n = 16
    does not exceed the count at n = 8 by more than 2, and at n = 16 it is below Jacobi's."""
    its = {}
    for n, nlev in ((8, 2), (16, 3)):
        model = VM.BlockModel(*block_levels(oracle, n, nlev), 2)
        A = model.levels[0]['Af']
        b = np.random.default_rng(0).standard_normal(A.shape[0])
        x, its[n] = G.pcg(A, b, model.vcycle, 1e-8)
        assert np.linalg.norm(A @ x - b) <= 1e-7 * np.linalg.norm(b)
    d = A.diagonal()
    _, it_j = G.pcg(A, b, lambda r: r / d, 1e-8)
    print('model PCG + V(1,1) iterations', its, 'Jacobi at n = 16', it_j)
    assert its[16] <= its[8] + 2 and its[16] < it_j, (its, it_j)

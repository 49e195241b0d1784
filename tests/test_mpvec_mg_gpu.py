"""Geometric multigrid for vector-valued systems on a multipatch (solvers.MultipatchVectorSystem.set_multigrid,
igx_solver_set_block_mg_*, pyiga_amd/csrc/multigrid_block.hip) on one MI355X.

1. k_csr_node_gs at every group width, 2 and 3 components, nodes with one fixed and one free component, an absent block pair:
   one forward and one backward sweep against the long-double node sweep of tests/_mpvec_mg_model.py; and past one pass of the
   colour grid.
2. The transfers at 2 and 3 components against I (x) P with the per-component masks.
3. The V-cycle against the numpy model on the downloaded level matrices, its symmetry, the solves against spsolve, the iteration
   counts against the model's PCG and against Jacobi, determinism.
4. Refusals and lifetime.
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.linalg

from pyiga_amd import _lib, assemble, solvers

import _mg_cases as mc
import _mg_model as G
import _mpsolve_model as M
import _mpvec_mg_cases as VC
import _mpvec_mg_model as VM
import _mpvec_model as MV
import _solver_cases as sc
import _vecsolve_model as V

pytestmark = pytest.mark.gpu

LD = np.longdouble
STIFF = 'inner(grad(u),grad(v))*dx'


def _rng(tag):
    return np.random.default_rng(zlib.crc32(tag.encode()))


# ---------------------------------------------------------------------------------------------
# 1. the sweep kernel on values scattered from the host
def _raw_system(MP, nc, fixed):
    """A MultipatchVectorSystem around a bare symmetric igx_solver_create_multipatch_block solver: no block taken yet."""
    S = object.__new__(solvers.MultipatchVectorSystem)
    S.MP, S.ncomp, S.N, S.symmetric = MP, nc, MP.numdofs, True
    S.n = nc * S.N
    S.b = np.zeros(S.n)
    h = MP._device()
    S._ctx = MP._ctx                                               # (the context is made with the device handle)
    S._attach('igx_solver_create_multipatch_block', (h, nc, 1), (fixed, np.zeros(len(fixed))), 'cg', 'cg')
    MP._solvers.add(S)
    S.present = [[False] * nc for _ in range(nc)]
    return S


def _scatter_take(S, p, q, vals):
    lib = _lib.load()
    h = S.MP._device()
    _lib.check(lib.igx_multipatch_zero(h), 'igx_multipatch_zero')
    for k, v in enumerate(vals):
        _lib.check(lib.igx_multipatch_scatter_host(h, k, _lib.dptr(np.ascontiguousarray(v))), 'igx_multipatch_scatter_host')
    _lib.check(lib.igx_solver_take_multipatch_block(S.handle, p, q), 'igx_solver_take_multipatch_block')
    S.present[p][q] = True


def _glue(MP, H, patterns, vals, nc):
    """The blocked global matrix of the per-patch block values: every block over the global pattern `H`, the entries of the
    patches added at their places in it (found once per patch; absent blocks stay empty)."""
    N = MP.numdofs
    hkey = np.repeat(np.arange(N, dtype=np.int64), np.diff(H.indptr)) * N + H.indices
    pos = []
    for k, Sp in enumerate(patterns):
        Sp = Sp.tocoo()
        l2g = np.asarray(MP.patch_to_global_idx(k), dtype=np.int64)
        at = np.searchsorted(hkey, l2g[Sp.row] * N + l2g[Sp.col])
        assert np.array_equal(hkey[at], l2g[Sp.row] * N + l2g[Sp.col])
        pos.append(at)
    rows = [[None] * nc for _ in range(nc)]
    for (p, q), v in vals.items():
        data = sum(np.bincount(at, weights=v[k], minlength=H.nnz) for k, at in enumerate(pos))
        rows[p][q] = scipy.sparse.csr_matrix((data, H.indices, H.indptr), shape=(N, N))
    A = scipy.sparse.bmat(rows, format='csr')
    A.sort_indices()
    return A


def _sweep_case(case, wrap):
    MP = case.build()
    assert MP.injective
    nc, N = case.nc, MP.numdofs
    rng = _rng(case.id + 'mg')
    fixed = MV.blocked_fixed(MP, VC.sides_per_component(case.domain, nc), nc, rng.choice(nc * N, size=max(1, nc * N // 50), replace=False))
    free = np.ones(nc * N, dtype=bool)
    free[fixed] = False
    fr = free.reshape(nc, N)
    assert np.any(fr.any(axis=0) & ~fr.all(axis=0))                 # nodes with a fixed and a free component
    H = sc.multipatch_pattern(MP)
    assert sc.spmv_gw(sc.max_row(H)) == case.gw
    patterns = [sc.patch_pattern(tuple(kvs)) for kvs, _ in MP.patches]
    vals = VC.symmetric_patch_values(patterns, case.present, nc, rng)
    if nc == 3:
        assert (1, 2) not in vals and (2, 1) not in vals            # a genuinely absent pair
    S = _raw_system(MP, nc, fixed)
    try:
        for (p, q), v in vals.items():
            _scatter_take(S, p, q, v)
        info = S._set_smoother(1)
        S._mg = dict(systems=[S], smooth_steps=1, info=[info])
        order = S.mg_colour_order(0)
        lists = VM.node_colour_lists(H.indptr, H.indices, free, nc)
        assert np.array_equal(order, np.concatenate(lists)) and info['colours'] == len(lists) and info['nodes'] == order.size
        largest = max(len(r) for r in lists)
        if wrap:
            print(case.id, 'nodes', N, 'colours', len(lists), 'largest colour', largest, 'one pass', VM.node_gs_pass_nodes(case.gw))
            assert largest > VM.node_gs_pass_nodes(case.gw)
        inf = S.mg_info()[0]
        assert not inf['one_block'] and not inf['dense_inverse'] and inf['nnz'] == len(vals) * H.nnz and inf['free'] == int(free.sum())
        A = _glue(MP, H, patterns, vals, nc)
        assert abs(A - A.T).max() == 0.0
        ref = VM.NodeSweep(A, nc, lists, free)
        x0, b = mc.relax_inputs(case.id, nc * N, fixed)
        for sweep in ('forward', 'backward'):
            x = S.relax(x0, b, sweep=sweep)
            d = mc.relmax(x, ref.sweep(x0, b, sweep))
            print('node relax', case.id, sweep, 'rel. difference %.2e' % d)
            assert d <= mc.RELAX_BOUND, (case.id, sweep, d)
            assert not x[fixed].any()                               # fixed entries are exactly 0
            assert np.array_equal(S.relax(x0, b, sweep=sweep), x)   # a fixed launch geometry: bit-identical
    finally:
        S.close()
        MP.close()


@pytest.mark.parametrize('case', VC.SWEEP_CASES, ids=[c.id for c in VC.SWEEP_CASES])
def test_node_sweep_at_every_width(case):
    _sweep_case(case, False)


def test_node_sweep_past_one_pass_of_the_colour_grid():
    _sweep_case(VC.BIG_CASE, True)


# ---------------------------------------------------------------------------------------------
# 2. / 3. linear elasticity: transfers, V-cycle, solves
def _bcs(case, MP):
    N = MP.numdofs
    idx, val = [], []
    for c, sides in enumerate(case.sides):
        d = M.fixed_dofs(MP, list(sides)) + c * N
        idx.append(d)
        val.append(np.full(d.size, case.values[c]))
    return np.concatenate(idx), np.concatenate(val)


@pytest.fixture(scope='module', params=VC.VCYCLE_CASES, ids=[c.id for c in VC.VCYCLE_CASES])
def system(request):
    """(case, S, fixed, values, rhs) with the hierarchy set up once; the tests below leave it as it is."""
    case = request.param
    MP = case.build()
    N = MP.numdofs
    fixed, vals = _bcs(case, MP)
    rhs = np.concatenate([np.full(N, (-1.0) ** c * 1e-3 * (c + 1)) for c in range(case.nc)])
    S = solvers.MultipatchVectorSystem(MP, V.ELASTICITY, rhs, (fixed, vals), bfuns=V.bfuns(case.nc), **VC.MU_LAM)
    S.set_multigrid(levels=case.levels)
    yield case, S, fixed, vals, rhs
    S.close()
    MP.close()


def _model(S):
    nl = len(S.mg_info())
    levels = [S.mg_level(l) for l in range(nl)]
    return VM.BlockModel([L.matrix() for L in levels], [L.MP for L in levels], [L.bc_indices for L in levels], S.ncomp,
                         orders=[S.mg_colour_order(l) for l in range(nl)])


def test_hierarchy_shape(system):
    case, S, fixed, vals, rhs = system
    info = S.mg_info()
    assert len(info) == case.levels and info[-1]['dense_inverse'] and not any(i['one_block'] for i in info)
    for l, inf in enumerate(info):
        L = S.mg_level(l)
        assert L.ncomp == case.nc and L.n == case.nc * L.MP.numdofs and inf['dofs'] == L.n
        assert inf['spans'][0] == (case.n >> l,) * len(inf['spans'][0])
        assert inf['nnz'] == case.nc ** 2 * L.MP.pattern()[1].size
        # the same sides fixed per component: component 0 keeps more fixed dofs than the others
        per = [int(((L.bc_indices >= c * L.N) & (L.bc_indices < (c + 1) * L.N)).sum()) for c in range(case.nc)]
        assert per[0] > per[1] > 0 and sum(per) == L.bc_indices.size == L.n - inf['free']
        if l:
            assert not L.b.any() and not L.bc_values.any()


def test_transfers_against_the_kronecker_prolongation(system):
    case, S, fixed, vals, rhs = system
    rng = _rng(case.id + 'transfer')
    nc = case.nc
    for level in range(case.levels - 1):
        F, Cs = S.mg_level(level), S.mg_level(level + 1)
        P = scipy.sparse.kron(scipy.sparse.identity(nc), G.global_prolongation(F.MP, Cs.MP)[0], format='csr')
        Pl = mc._ld(P)
        ff, fc = np.ones(F.n, dtype=LD), np.ones(Cs.n, dtype=LD)
        ff[F.bc_indices] = 0
        fc[Cs.bc_indices] = 0
        xc, rf = rng.standard_normal(Cs.n), rng.standard_normal(F.n)
        y = S.prolong(xc, level)
        d = mc.relmax(y, ff * (Pl @ (fc * xc)))
        print('prolong', case.id, 'level', level, 'rel. difference %.2e' % d)
        assert d <= mc.TRANSFER_BOUND and not y[F.bc_indices].any()
        z = S.restrict(rf, level)
        d = mc.relmax(z, fc * (Pl.T @ (ff * rf)))
        print('restrict', case.id, 'level', level, 'rel. difference %.2e' % d)
        assert d <= mc.TRANSFER_BOUND and not z[Cs.bc_indices].any()


def test_vcycle_matches_the_model_and_is_symmetric(system):
    """The symmetry defect |<B x, y> - <x, B y>| is measured against sum |B x|_i |y|_i, the magnitude of the terms of the inner
    products, which is what their rounding scales with."""
    case, S, fixed, vals, rhs = system
    model = _model(S)
    rng = _rng(case.id + 'vcycle')
    x, y = rng.standard_normal(S.n), rng.standard_normal(S.n)
    Bx, By = S.apply_precond(x, 'mg'), S.apply_precond(y, 'mg')
    ref = model.apply_full(x)
    d = mc.relmax(Bx, ref)
    print('V-cycle', case.id, 'rel. difference to the model %.2e' % d)
    assert d <= mc.VCYCLE_BOUND
    assert not Bx[fixed].any()
    free = np.ones(S.n, dtype=bool)
    free[fixed] = False
    a, b = Bx[free] @ y[free], x[free] @ By[free]
    scale = np.abs(Bx[free]) @ np.abs(y[free])
    print('V-cycle', case.id, 'symmetry defect %.2e of the terms, %.2e of the product' % (abs(a - b) / scale, abs(a - b) / abs(a)))
    assert abs(a - b) <= 1e-13 * scale
    assert np.array_equal(S.apply_precond(x, 'mg'), Bx)
    prof = S.mg_profile(reps=2)
    assert prof['levels'] == case.levels and prof['launches'] > 0 and prof['total_ms'] > 0


def test_solves_against_spsolve_and_iteration_counts(system):
    case, S, fixed, vals, rhs = system
    tol = 1e-10
    A = S.matrix()
    LS = assemble.RestrictedLinearSystem(A, rhs, (fixed, vals))
    uref = LS.complete(scipy.sparse.linalg.spsolve(LS.A.tocsc(), LS.b))
    assert np.any(vals != 0)
    u = S.solve(tol=tol, maxiter=500, precond='mg')
    info = dict(S.info)
    assert info['converged'] and info['precond'] == 'mg' and info['method'] == 'cg'
    assert info['levels'] == case.levels and info['smooth_steps'] == 1
    assert np.array_equal(u[fixed], vals)
    free = np.setdiff1d(np.arange(S.n), fixed)
    res = (rhs - A @ u)[free]
    assert np.linalg.norm(res) <= 2 * tol * np.linalg.norm(LS.b)
    assert np.linalg.norm(u - uref) <= 1e-5 * np.linalg.norm(uref), np.linalg.norm(u - uref) / np.linalg.norm(uref)
    assert np.array_equal(S.solve(tol=tol, maxiter=500, precond='mg'), u)       # two solves are bit-identical
    model = _model(S)
    _, it = G.pcg(LS.A.tocsr(), np.asarray(LS.b, dtype=float), model.vcycle, tol)
    S.solve(tol=tol, maxiter=5000, precond='jacobi')
    it_j = S.info['iterations']
    print('elasticity', case.id, 'CG iterations: mg', info['iterations'], 'model', it, 'jacobi', it_j)
    assert abs(info['iterations'] - it) <= 1, (info['iterations'], it)
    assert info['iterations'] < it_j


# ---------------------------------------------------------------------------------------------
# 4. refusals and lifetime
def _small(MP, sides=(((0, 'left'),), ((0, 'left'), (2, 'top'))), extra=(), **kw):
    N = MP.numdofs
    fixed = MV.blocked_fixed(MP, [list(s) for s in sides], 2, extra)
    rhs = np.concatenate([np.full(N, 1e-3), np.full(N, -1e-3)])
    return solvers.MultipatchVectorSystem(MP, V.ELASTICITY, rhs, (fixed, np.full(fixed.size, 0.01)), bfuns=V.bfuns(2), **VC.MU_LAM, **kw)


def test_python_refusals():
    MP = M.lshape(p=2, n=4)
    N = MP.numdofs
    S = _small(MP)
    try:
        with pytest.raises(ValueError, match='mg'):
            S.solve(precond='mg')
        with pytest.raises(ValueError, match=r'set_multigrid\(\)'):
            S.apply_precond(np.ones(S.n), 'mg')
        with pytest.raises(ValueError, match='kron'):
            S.solve(precond='kron')
        with pytest.raises(ValueError, match='coarse_max'):
            S.set_multigrid(levels=1, coarse_max=10)
        assert S._mg is None
        S.set_method('bicgstab')
        with pytest.raises(ValueError, match='cg'):
            S.set_multigrid()
        S.set_method('cg')
        S.set_multigrid(levels=2)
        S.solve(precond='mg')
        assert S.info['converged'] and S.info['levels'] == 2
        with pytest.raises(ValueError, match='cg'):
            S.set_method('bicgstab')
        assert S.method == 'cg'
    finally:
        S.close()
    interior = int(np.setdiff1d(np.arange(N), M.fixed_dofs(MP, [(p, s) for p in range(3) for s in ('left', 'right', 'top', 'bottom')]))[0])
    S = _small(MP, extra=[N + interior])                           # component 1: a side and one dof of no side
    try:
        with pytest.raises(ValueError, match='component 1'):
            S.set_multigrid()
    finally:
        S.close()
    S = solvers.MultipatchVectorSystem(MP, V.NONSYM, 0.0, (M.fixed_dofs(MP, [(0, 'left')]), 0.0), bfuns=V.bfuns(2))
    try:
        assert S.method == 'bicgstab'
        with pytest.raises(ValueError, match='cg'):
            S.set_multigrid()
    finally:
        S.close()
        MP.close()


def test_c_refusals_and_lifetime():
    lib = _lib.load()
    MP = M.lshape(p=2, n=4)
    MPs = M.lshape(p=2, n=4)
    side = M.fixed_dofs(MPs, [(0, 'left')])
    scalars = [solvers.MultipatchSystem(MPs, STIFF, 'v*dx', bcs=(side, 0.0)) for _ in range(2)]
    S = _small(MP)
    try:
        S.set_multigrid(levels=2)
        L1 = S.mg_level(1)
        colour = np.zeros(S.N, dtype=np.int32)
        cp = colour.ctypes.data_as(C.POINTER(C.c_int32))
        P = [np.ones((1, 1))] * (3 * MP.numpatches)
        Pp = (_lib._dp * len(P))(*[_lib.dptr(a) for a in P])
        mult = np.ones(S.N)
        inv = np.ones((1, 1))
        # the scalar calls on a block solver, the block calls on a scalar multipatch solver
        assert lib.igx_solver_set_mg_smoother(S.handle, cp, 1, 0) == _lib.IGX_ERR_UNSUPPORTED
        assert lib.igx_solver_set_mg_coarse(S.handle, L1.handle, Pp, _lib.dptr(mult)) == _lib.IGX_ERR_UNSUPPORTED
        assert lib.igx_solver_set_mg_inverse(S.handle, _lib.dptr(inv), 1) == _lib.IGX_ERR_UNSUPPORTED
        a, b = scalars
        assert lib.igx_solver_set_block_mg_smoother(a.handle, cp, 1) == _lib.IGX_ERR_UNSUPPORTED
        assert lib.igx_solver_set_block_mg_coarse(a.handle, b.handle, Pp, _lib.dptr(mult)) == _lib.IGX_ERR_UNSUPPORTED
        assert lib.igx_solver_set_block_mg_inverse(a.handle, _lib.dptr(inv), 1) == _lib.IGX_ERR_UNSUPPORTED
        # two coupled nodes of one colour are named
        assert lib.igx_solver_set_block_mg_smoother(L1.handle, cp, 1) == _lib.IGX_ERR_ARG
        assert b'coupled' in lib.igx_last_error()
        assert lib.igx_solver_set_block_mg_smoother(S.handle, cp, 17) == _lib.IGX_ERR_ARG
        # the hierarchy is intact after the refusals
        u = S.solve(tol=1e-10, precond='mg')
        assert S.info['converged']
        # destroying a level unlinks it: the finer level loses the preconditioner
        L1.close()
        assert lib.igx_solver_set_precond(S.handle, _lib.IGX_PRECOND_MG, None, None, None, None, 0) == _lib.IGX_ERR_UNSUPPORTED
        S.set_multigrid(levels=2)
        assert np.array_equal(S.solve(tol=1e-10, precond='mg'), u)
        # closing the fine system closes the levels
        levels = [S.mg_level(l) for l in range(2)]
        S.close()
        assert all(L.handle is None for L in levels) and S._mg is None
    finally:
        S.close()
        for s in scalars:
            s.close()
        MPs.close()
    S = _small(MP)
    try:
        S.set_multigrid(levels=2)
        S.solve(precond='mg')
        MP.close()
        assert S.handle is None
        for call in (lambda: S.solve(precond='mg'), lambda: S.relax(np.zeros(S.n)), lambda: S.apply_precond(np.zeros(S.n), 'mg'),
                     lambda: S.set_multigrid()):
            with pytest.raises(_lib.IgxError):
                call()
    finally:
        S.close()
        MP.close()

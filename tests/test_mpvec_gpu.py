"""Vector-valued Dirichlet problems on a multipatch solved on the device (solvers.MultipatchVectorSystem,
igx_solver_create_multipatch_block; one MI355X).

1. k_csr_block_spmv: every case of tests/_mpvec_model.py (every group width past one grid of scalar rows, 2 and 3 components,
   absent blocks at nc = 3), with block values spread over +-20 binades scattered from the host, row by row against the
   long-double product of the glued matrix; fixed rows exactly 0; Jacobi bit for bit.
2. Stale rows: a block present on one patch only -- the other patch must scatter zeros, or its interior rows keep the previous
   block's values.
3. / 4. Linear elasticity on the L-shape (nc = 2, non-zero vector-valued Dirichlet data) and on two cubes (nc = 3) against
   spsolve of the host glue, Jacobi, Schwarz and no preconditioner; the Schwarz operator and the iteration counts against the
   host model.
5. A non-symmetric form by BiCGStab.  6. The reference's matrices and solutions (golden_mpvec.npz).
7. Lifetime, determinism and refusals.
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.linalg

from pyiga_amd import _lib, assemble, solvers
from pyiga_amd.operators import DeviceArray

import _mpsolve_model as M
import _mpvec_model as MV
import _solver_cases as sc
import _vecsolve_model as V

from conftest import golden_csr

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
MU_LAM = dict(mu=1.0, lam=2.0)
STIFF = 'inner(grad(u),grad(v))*dx'


def _rng(tag):
    return np.random.default_rng(zlib.crc32(tag.encode()))


def _spread(rng, n, binades=20):
    return rng.choice([-1.0, 1.0], n) * np.exp2(rng.uniform(-binades, binades, n))


def _ld(A):
    A = A.tocsr()
    return scipy.sparse.csr_matrix((A.data.astype(np.longdouble), A.indices, A.indptr), shape=A.shape)


def _raw_system(MP, nc, fixed, symmetric=False):
    """A MultipatchVectorSystem around a bare igx_solver_create_multipatch_block solver: no block taken yet."""
    S = object.__new__(solvers.MultipatchVectorSystem)
    S.MP, S.ncomp, S.N, S.symmetric = MP, nc, MP.numdofs, symmetric
    S.n = nc * S.N
    S.b = np.zeros(S.n)
    h = MP._device()
    S._ctx = MP._ctx
    method = 'cg' if symmetric else 'bicgstab'
    S._attach('igx_solver_create_multipatch_block', (h, nc, 1 if symmetric else 0), (fixed, np.zeros(len(fixed))), method, method)
    MP._solvers.add(S)
    S.present = [[False] * nc for _ in range(nc)]
    return S


def _scatter_take(S, p, q, vals):
    """Block (p, q) from the host values `vals[k]` of every patch k (canonical CSR order), as the block loop sums it."""
    lib = _lib.load()
    h = S.MP._device()
    _lib.check(lib.igx_multipatch_zero(h), 'igx_multipatch_zero')
    for k, v in enumerate(vals):
        _lib.check(lib.igx_multipatch_scatter_host(h, k, _lib.dptr(np.ascontiguousarray(v))), 'igx_multipatch_scatter_host')
    _lib.check(lib.igx_solver_take_multipatch_block(S.handle, p, q), 'igx_solver_take_multipatch_block')
    S.present[p][q] = True


def _patch_blocked(patterns, vals, nc):
    """Per patch the blocked matrix of its scalar blocks ``vals[(p, q)][k]`` over the patch pattern (absent blocks empty)."""
    mats = []
    for k, Sp in enumerate(patterns):
        N = Sp.shape[0]
        rows = [[scipy.sparse.csr_matrix((vals[(p, q)][k], Sp.indices, Sp.indptr), shape=(N, N)) if (p, q) in vals
                 else scipy.sparse.csr_matrix((N, N)) for q in range(nc)] for p in range(nc)]
        mats.append(scipy.sparse.bmat(rows, format='csr'))
    return mats


def _blocked_l2g(MP, k, nc):
    l2g = np.asarray(MP.patch_to_global_idx(k), dtype=np.int64)
    return np.concatenate([c * MP.numdofs + l2g for c in range(nc)])


def _glue_fast(MP, mats, nc):
    """MV.glue for injective maps without the triple products: the entries of every patch renumbered and added in patch order."""
    n = nc * MP.numdofs
    A = scipy.sparse.csr_matrix((n, n))
    for k, Ak in enumerate(mats):
        Ak = scipy.sparse.coo_matrix(Ak)
        g = _blocked_l2g(MP, k, nc)
        A = A + scipy.sparse.csr_matrix((Ak.data, (g[Ak.row], g[Ak.col])), shape=(n, n))
    A = A.tocsr()
    A.sort_indices()
    return A


# ---------------------------------------------------------------------------------------------
# 1. the kernel: every width past one grid of scalar rows, 2 and 3 components
@pytest.mark.parametrize('case', MV.MPVEC_CASES, ids=[c.id for c in MV.MPVEC_CASES])
def test_csr_block_spmv_and_jacobi(case):
    MP = case.build()
    assert MP.injective
    nc, n = case.nc, MP.numdofs
    rng = _rng(case.id)
    sides = MV.CASE_SIDES[case.mp.domain]
    per_comp = [[sides[0]]] + [[] for _ in range(nc - 2)] + [[sides[1]]]
    fixed = MV.blocked_fixed(MP, per_comp, nc, rng.choice(nc * n, size=max(1, nc * n // 50), replace=False))
    free = np.ones(nc * n, dtype=bool)
    free[fixed] = False
    # from the case data: interface rows longer than the patch rows they sum, rows with one component fixed and another free,
    # and the width the longest row selects
    H = sc.multipatch_pattern(MP)
    assert sc.spmv_gw(sc.max_row(H)) == case.gw and n > sc.spmv_pass_rows(case.gw)
    assert MV.interface_rows_gain(MP, H).min() > 0
    fr = free.reshape(nc, n)
    assert np.any(fr.any(axis=0) & ~fr.all(axis=0)) and np.any(~fr.any(axis=0))
    patterns = [sc.patch_pattern(tuple(kvs)) for kvs, _ in MP.patches]
    vals = {pq: [_spread(rng, Sp.nnz) for Sp in patterns] for pq in case.present}
    S = _raw_system(MP, nc, fixed)
    try:
        for (p, q), v in vals.items():
            _scatter_take(S, p, q, v)
        A = _glue_fast(MP, _patch_blocked(patterns, vals, nc), nc)
        lens = np.diff(A.indptr)
        assert np.array_equal(lens.reshape(nc, n), np.array([sum((p, q) in vals for q in range(nc)) for p in range(nc)])[:, None]
                              * np.diff(H.indptr)[None, :])
        x = _spread(rng, nc * n)
        y = S.spmv(x)
        xf = np.where(free, x, 0.0)
        Al = _ld(A)
        ref = np.where(free, Al @ xf.astype(np.longdouble), 0.0)
        mag = abs(Al) @ np.abs(xf).astype(np.longdouble)
        bound = 2 * lens * U53 * mag
        err = np.abs(y.astype(np.longdouble) - ref)
        bad = np.flatnonzero(free & (err > bound))
        print(case.id, 'largest error / bound %.3f' % float(np.max(err[free] / np.maximum(bound[free], 1e-300))))
        assert bad.size == 0, (case.id, bad.size, bad[:8], [float(err[i] / max(mag[i], 1e-300)) for i in bad[:4]])
        assert np.all(y[~free] == 0.0), case.id
        assert np.all(mag[free] > 0)
        x2 = x.copy()
        x2[fixed] = _spread(rng, fixed.size) * 1e3
        assert np.array_equal(S.spmv(x2), y), case.id              # the fixed entries of x are not read
        assert np.array_equal(S.spmv(x), y), case.id               # a fixed grid: two products are bit-identical
        r = _spread(_rng(case.id + 'r'), nc * n, 8)
        z = S.apply_precond(r, 'jacobi')
        assert np.array_equal(z, np.where(free, (1.0 / A.diagonal()) * r, 0.0)), case.id
    finally:
        S.close()
        MP.close()


# ---------------------------------------------------------------------------------------------
# 2. stale rows
def _two_squares(p=2, n=5):
    from pyiga_amd import bspline, geometry
    kvs = 2 * (bspline.make_knots(p, 0.0, 1.0, n),)
    squ = geometry.unit_square()
    MP = assemble.Multipatch([(kvs, squ), (kvs, squ.translate((1, 0)))])
    MP.join_boundaries(0, 'right', 1, 'left')
    MP.finalize()
    return MP


def _interior_rows(MP, k):
    """The global rows only patch k reaches (its non-shared dofs)."""
    return np.arange(int(MP.M_ofs[k]), int(MP.M_ofs[k + 1]))


def test_block_present_on_one_patch_only_leaves_no_stale_rows_host_values():
    MP = _two_squares()
    n = MP.numdofs
    rng = _rng('stale')
    patterns = [sc.patch_pattern(tuple(kvs)) for kvs, _ in MP.patches]
    vals = {(0, 0): [_spread(rng, Sp.nnz, 4) for Sp in patterns], (1, 1): [_spread(rng, Sp.nnz, 4) for Sp in patterns],
            (0, 1): [_spread(rng, patterns[0].nnz, 4), np.zeros(patterns[1].nnz)]}        # absent on patch 1: zeros are scattered
    S = _raw_system(MP, 2, np.zeros(0, dtype=np.int64))
    try:
        for pq in ((0, 0), (0, 1), (1, 1)):
            _scatter_take(S, pq[0], pq[1], vals[pq])
        A = S.matrix()
        G = MV.glue(MP, _patch_blocked(patterns, vals, 2), 2)
        assert abs(A - G).max() == 0.0
        assert abs(_glue_fast(MP, _patch_blocked(patterns, vals, 2), 2) - G).max() == 0.0     # (the kernel cases' cheaper glue)
        B01 = A[:n, n:].tocsr()
        rows1 = _interior_rows(MP, 1)
        assert rows1.size and not B01[rows1].data.any()            # patch 1's interior rows are exactly 0
        assert B01[_interior_rows(MP, 0)].data.all()
        assert not A[n:, :n].nnz                                   # block (1, 0) was never taken: absent
        assert S.present == [[True, True], [False, True]]
    finally:
        S.close()
        MP.close()


def test_block_loop_scatters_zeros_for_a_patch_without_the_block():
    """The block loop itself: the table of block (0, 1) is removed from patch 1's assembler."""
    from pyiga_amd.form_assemblers import FormAssembler
    MP = _two_squares()
    n = MP.numdofs
    form = V.COUPLED[2]
    asms = [FormAssembler(tuple(kvs), geo, form, bfuns=V.bfuns(2)) for kvs, geo in MP.patches]
    d = 2
    asms[1]._table[0][1] = [[None] * (d + 1) for _ in range(d + 1)]
    blocks = {}
    indptr, indices = MP.pattern()

    def download(p, q, h):
        data = np.empty(indices.shape[0])
        _lib.check(_lib.load().igx_multipatch_download(h, _lib.dptr(data), None), 'igx_multipatch_download')
        blocks[(p, q)] = scipy.sparse.csr_matrix((data, indices.copy(), indptr.copy()), shape=(n, n))
    try:
        present = MP._sum_vector_blocks(asms, 2, download)
    finally:
        for a in asms:
            a.patch.close()
    assert present == [[True, True], [False, True]]
    kvs, geo = MP.patches[0]
    N0 = MP.N[0]
    A0 = assemble.assemble(form, kvs, bfuns=V.bfuns(2), geo=geo, layout='blocked').tocsr()
    X0 = MP.patch_to_global(0)
    want = (X0 @ A0[:N0, N0:] @ X0.T).tocsr()
    B01 = blocks[(0, 1)]
    assert abs(B01 - want).max() <= 4 * U53 * abs(want).max()
    assert abs(want).max() > 0 and abs(blocks[(0, 0)][_interior_rows(MP, 1)]).max() > 0      # (the previous block was there)
    assert not B01[_interior_rows(MP, 1)].data.any()
    MP.close()


# ---------------------------------------------------------------------------------------------
# 3. - 5. solves against spsolve of the host glue
def _host_glue(MP, form, nc, **inputs):
    mats = [assemble.assemble(form, tuple(kvs), bfuns=V.bfuns(nc), geo=geo, layout='blocked', **inputs).tocsr()
            for kvs, geo in MP.patches]
    return MV.glue(MP, mats, nc), mats


def _terms(MP, mats, nc):
    """sum_p (I (x) X_p) |A_p| (I (x) X_p)^T: the magnitudes of the terms every entry of the glue sums."""
    return MV.glue(MP, [abs(A) for A in mats], nc)


def _check_matrix(Adev, A, T):
    D = abs(Adev - A).tocsr()
    D.eliminate_zeros()
    excess = (D - 4 * U53 * T).tocsr()
    assert excess.nnz == 0 or excess.max() <= 0.0, float(excess.max())


def _check_solution(S, u, A, LS, uref, fixed, vals, rhs, tol):
    assert np.array_equal(u[fixed], vals)
    free = np.setdiff1d(np.arange(S.n), fixed)
    res = (rhs - A @ u)[free]
    assert np.linalg.norm(res) <= 2 * tol * np.linalg.norm(LS.b), (np.linalg.norm(res), np.linalg.norm(LS.b))
    assert np.linalg.norm(u - uref) <= 1e-5 * np.linalg.norm(uref), np.linalg.norm(u - uref) / np.linalg.norm(uref)


def _model(S):
    shapes, maps = M.shapes_maps(S.MP)
    return MV.BlockSchwarzModel(S.N, shapes, maps, S.bc_indices, S.schwarz_setup())


def _free_op(S, P, free):
    def Mfree(v):
        full = np.zeros(S.n)
        full[free] = v
        return P.apply(full)[free]
    return Mfree


def g_lshape(x, y):
    return (0.01 + 0.02 * y, -0.02 + 0.01 * y * y)


def test_elasticity_2d_lshape_against_spsolve():
    MP = M.lshape(p=2, n=8)
    n = MP.numdofs
    bcs = MP.compute_dirichlet_bcs([(0, 'left', g_lshape)])
    fixed, vals = np.asarray(bcs[0], dtype=np.int64), np.asarray(bcs[1], dtype=np.float64)
    # blocked global indices: both components of the side's dofs, with the values of the two components
    side = M.fixed_dofs(MP, [(0, 'left')])
    assert np.array_equal(fixed, np.concatenate([side, side + n]))
    assert np.any(vals != 0) and not np.array_equal(vals[:side.size], vals[side.size:])
    rhs = np.concatenate([np.full(n, 1e-3), np.full(n, -2e-3)])
    S = solvers.MultipatchVectorSystem(MP, V.ELASTICITY, rhs, bcs, bfuns=V.bfuns(2), **MU_LAM)
    try:
        assert S.symmetric and S.method == 'cg' and S.ncomp == 2 and S.present == [[True, True], [True, True]]
        A, mats = _host_glue(MP, V.ELASTICITY, 2, **MU_LAM)
        LS = assemble.RestrictedLinearSystem(A, rhs, (fixed, vals))
        uref = LS.complete(scipy.sparse.linalg.spsolve(LS.A.tocsc(), LS.b))
        Adev = S.matrix()
        _check_matrix(Adev, A, _terms(MP, mats, 2))
        free = np.setdiff1d(np.arange(S.n), fixed)
        its = {}
        for precond in ('jacobi', 'schwarz', None):
            u = S.solve(tol=1e-10, maxiter=5000, precond=precond)
            assert S.info['converged'] and S.info['precond'] == (precond or 'none') and S.info['method'] == 'cg'
            _check_solution(S, u, Adev, LS, uref, fixed, vals, rhs, 1e-10)
            its[precond] = S.info['iterations']
        print('L-shape elasticity iterations', its)
        # x = 0 on the fixed dofs and the spmv is R A R^T
        x = _rng('lshape').standard_normal(S.n)
        y = S.spmv(x)
        want = np.zeros(S.n)
        want[free] = (Adev[free][:, free] @ x[free])
        assert np.max(np.abs(y - want)) <= 1e-13 * np.max(np.abs(want))
    finally:
        S.close()
    A2, b2 = MP.assemble_vector_system(V.ELASTICITY, rhs, V.bfuns(2), **MU_LAM)
    assert abs(A2 - Adev).max() == 0.0 and np.array_equal(b2, rhs)
    MP.close()


def test_rhs_form_string_and_scalar():
    MP = M.lshape(p=2, n=4)
    n = MP.numdofs
    A, b = MP.assemble_vector_system(V.ELASTICITY, 'inner(f, v) * dx', V.bfuns(2), f=(1.0, -0.5), **MU_LAM)
    want = np.zeros(2 * n)
    for k, (kvs, geo) in enumerate(MP.patches):
        bk = np.asarray(assemble.assemble('inner(f, v) * dx', kvs, bfuns=[('v', 2)], geo=geo, f=(1.0, -0.5), layout='blocked'))
        for c in range(2):
            np.add.at(want, c * n + MP.patch_to_global_idx(k), bk[c].ravel())
    assert np.array_equal(b, want) and np.all(b[:n] > 0) and np.all(b[n:] < 0)
    side = M.fixed_dofs(MP, [(0, 'left')])
    bcs = (np.concatenate([side, side + n]), np.zeros(2 * side.size))
    S = solvers.MultipatchVectorSystem(MP, V.ELASTICITY, 'inner(f, v) * dx', bcs, bfuns=V.bfuns(2), f=(1.0, -0.5), **MU_LAM)
    try:
        assert np.array_equal(S.b, want)
        u = S.solve(tol=1e-10)
        LS = assemble.RestrictedLinearSystem(A, b, bcs)
        uref = LS.complete(scipy.sparse.linalg.spsolve(LS.A.tocsc(), LS.b))
        assert S.info['converged'] and np.linalg.norm(u - uref) <= 1e-5 * np.linalg.norm(uref)
    finally:
        S.close()
    S = solvers.MultipatchVectorSystem(MP, V.ELASTICITY, 1.0, bcs, bfuns=V.bfuns(2), **MU_LAM)
    try:
        assert np.array_equal(S.b, np.ones(2 * n))
    finally:
        S.close()
        MP.close()


def test_elasticity_3d_two_cubes_against_spsolve_and_model():
    MP = sc.two_cubes(p=2, n=4)
    n = MP.numdofs
    side = M.fixed_dofs(MP, [(0, (2, 0))])                            # the far end of patch 0; the interface dofs are free
    shared = np.arange(int(MP.M_ofs[-1]), n)
    assert shared.size and not np.intersect1d(side, shared).size
    fixed = np.concatenate([side + c * n for c in range(3)])
    vals = np.zeros(fixed.size)
    rhs = np.concatenate([np.full(n, 1e-3), np.zeros(n), np.full(n, -1e-3)])
    S = solvers.MultipatchVectorSystem(MP, V.ELASTICITY, rhs, (fixed, vals), bfuns=V.bfuns(3), **MU_LAM)
    try:
        assert S.symmetric and S.method == 'cg' and S.ncomp == 3 and all(all(r) for r in S.present)
        A, mats = _host_glue(MP, V.ELASTICITY, 3, **MU_LAM)
        LS = assemble.RestrictedLinearSystem(A, rhs, (fixed, vals))
        uref = LS.complete(scipy.sparse.linalg.spsolve(LS.A.tocsc(), LS.b))
        Adev = S.matrix()
        _check_matrix(Adev, A, _terms(MP, mats, 3))
        free = np.setdiff1d(np.arange(S.n), fixed)
        isfree = np.ones(S.n, dtype=bool)
        isfree[fixed] = False
        P = _model(S)
        r = _spread(_rng('cubes'), S.n, 4)
        z = S.apply_precond(r, 'schwarz')
        zm = P.apply(r)
        assert np.max(np.abs(z - zm)) <= 1e-11 * np.max(np.abs(zm))
        assert np.all(z[~isfree] == 0.0)
        dinv = 1.0 / Adev.diagonal()[free]
        for precond, Mf in (('jacobi', lambda v: dinv * v), ('schwarz', _free_op(S, P, free))):
            u = S.solve(tol=1e-10, maxiter=5000, precond=precond)
            assert S.info['converged'] and S.info['precond'] == precond
            _check_solution(S, u, Adev, LS, uref, fixed, vals, rhs, 1e-10)
            _, it, conv = V.pcg(LS.A, LS.b, Mf, tol=1e-10, maxiter=5000)
            print('two cubes elasticity', precond, 'device', S.info['iterations'], 'model', it)
            assert conv and abs(S.info['iterations'] - it) <= 2, (precond, S.info['iterations'], it)
    finally:
        S.close()
        MP.close()


@pytest.mark.parametrize('precond', ['jacobi', 'schwarz'])
def test_nonsymmetric_lshape_bicgstab_against_spsolve(precond):
    MP = M.lshape(p=2, n=8)
    n = MP.numdofs
    side = M.fixed_dofs(MP, [(0, 'left'), (2, 'top')])
    fixed = np.concatenate([side, side + n])
    vals = np.where(fixed < n, 0.5, -0.25)
    rhs = _rng('mpnonsym').standard_normal(2 * n) * 1e-2
    with pytest.raises(ValueError, match='not symmetric'):
        solvers.MultipatchVectorSystem(MP, V.NONSYM, rhs, (fixed, vals), bfuns=V.bfuns(2), method='cg')
    S = solvers.MultipatchVectorSystem(MP, V.NONSYM, rhs, (fixed, vals), bfuns=V.bfuns(2))
    try:
        assert not S.symmetric and S.method == 'bicgstab' and S.present == [[True, True], [False, True]]
        u = S.solve(tol=1e-10, maxiter=5000, precond=precond)
        assert S.info['converged'] and S.info['breakdown'] is None and S.info['method'] == 'bicgstab'
        A, _ = _host_glue(MP, V.NONSYM, 2)
        LS = assemble.RestrictedLinearSystem(A, rhs, (fixed, vals))
        uref = LS.complete(scipy.sparse.linalg.spsolve(LS.A.tocsc(), LS.b))
        _check_solution(S, u, S.matrix(), LS, uref, fixed, vals, rhs, 1e-10)
        assert np.array_equal(S.solve(tol=1e-10, maxiter=5000, precond=precond), u)
        with pytest.raises(_lib.IgxError) as e:
            S.set_method('cg')                                     # made as non-symmetric
        assert e.value.code == _lib.IGX_ERR_UNSUPPORTED
    finally:
        S.close()
        MP.close()


# ---------------------------------------------------------------------------------------------
# 6. the reference's matrices and solutions
def _relmax(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@pytest.mark.parametrize('name, nc', [('lshape', 2), ('cubes2', 3)])
def test_golden_parity(golden, name, nc):
    g = golden('mpvec')
    MP = M.lshape(p=2, n=4) if name == 'lshape' else sc.two_cubes(p=2, n=2)
    G = golden_csr(g, name + '_A')
    fixed, vals, rhs, uref = g[name + '_fixed'], g[name + '_values'], g[name + '_rhs'], g[name + '_u']
    assert G.shape == (nc * MP.numdofs,) * 2
    if name == 'lshape':                                           # the reference's Dirichlet data, through the device's own path
        idx, v = MP.compute_dirichlet_bcs([(0, 'left', g_lshape)])
        assert np.array_equal(idx, fixed) and np.max(np.abs(v - vals)) <= 1e-12 * np.max(np.abs(vals))
    S = solvers.MultipatchVectorSystem(MP, V.ELASTICITY, rhs, (fixed, vals), bfuns=V.bfuns(nc), **MU_LAM)
    try:
        A = S.matrix()
        D = abs(A - G)
        assert (D.max() if D.nnz else 0.0) <= 1e-10 * abs(G).max()
        u = S.solve(tol=1e-13, maxiter=5000, precond='schwarz')
        assert S.info['converged'] and _relmax(u, uref) <= 1e-10, _relmax(u, uref)
        u = S.solve(tol=1e-13, maxiter=5000, precond='jacobi')
        assert S.info['converged'] and _relmax(u, uref) <= 1e-10, _relmax(u, uref)
    finally:
        S.close()
        MP.close()


# ---------------------------------------------------------------------------------------------
# 7. lifetime, determinism, refusals
def _small_system(MP, nc=2, **kw):
    n = MP.numdofs
    side = M.fixed_dofs(MP, [(0, 'left')])
    fixed = np.concatenate([side + c * n for c in range(nc)])
    rhs = np.concatenate([np.full(n, (-1.0) ** c * 1e-3) for c in range(nc)])
    return solvers.MultipatchVectorSystem(MP, V.ELASTICITY, rhs, (fixed, np.full(fixed.size, 0.01)), bfuns=V.bfuns(nc), **MU_LAM, **kw)


def f_one(*x):
    return 1.0 + 0.0 * x[0]


def test_lifetime_and_determinism():
    MP = M.lshape(p=2, n=6)
    scalar = solvers.MultipatchSystem(MP, STIFF, 'f*v*dx', bcs=(M.fixed_dofs(MP, [(0, 'left')]), 0.0), f=f_one)
    S = _small_system(MP)
    try:
        with pytest.raises(_lib.IgxError, match='restarted'):      # the vector system restarted the sums: the scalar one is stale
            scalar.solve()
        u = S.solve(tol=1e-10)
        assert S.info['converged'] and np.array_equal(S.solve(tol=1e-10), u)
        us = S.solve(tol=1e-10, precond='schwarz')
        assert np.array_equal(S.solve(tol=1e-10, precond='schwarz'), us)
        y = S.spmv(u)
        # a later scalar assembly over the same multipatch does not disturb the system: it owns its blocks
        MP.assemble_system(STIFF, 'v*dx')
        assert np.array_equal(S.solve(tol=1e-10), u) and np.array_equal(S.spmv(u), y)
        assert np.array_equal(S.solve(tol=1e-10, precond='schwarz'), us)
        for precond in ('mg', 'kron'):
            with pytest.raises(ValueError, match=precond):
                S.solve(precond=precond)
        MP.close()
        assert S.handle is None and scalar.handle is None
        for call in (lambda: S.solve(), lambda: S.spmv(np.zeros(S.n)), lambda: S.matrix()):
            with pytest.raises(_lib.IgxError):
                call()
    finally:
        S.close()
        scalar.close()
        MP.close()


def test_scalar_form_and_four_components_refused():
    MP = M.lshape(p=2, n=4)
    with pytest.raises(ValueError, match='scalar form'):
        solvers.MultipatchVectorSystem(MP, 'u * v * dx', 0.0)
    with pytest.raises(ValueError, match='2 or 3'):
        solvers.MultipatchVectorSystem(MP, 'inner(u, v) * dx', 0.0, bfuns=V.bfuns(4))
    with pytest.raises(NotImplementedError):
        MP.assemble_system(V.ELASTICITY, None, bfuns=V.bfuns(2), **MU_LAM)
    assert MP._handle is None                                      # (no device work was done)


def test_non_injective_join_refuses_schwarz_and_solves_with_jacobi():
    from pyiga_amd import bspline, geometry
    kvs = 2 * (bspline.make_knots(2, 0.0, 1.0, 4),)
    squ = geometry.unit_square()
    MP = assemble.Multipatch([(kvs, squ), (kvs, squ.translate((1, 0)))])
    MP.join_boundaries(0, 'right', 1, 'left')
    # two dofs of patch 1's far side share one global dof
    far = assemble.boundary_dofs(kvs, 'right', ravel=True)
    MP.join_dofs(1, far[:1], 0, assemble.boundary_dofs(kvs, 'right', ravel=True)[:1])
    MP.join_dofs(1, far[1:2], 0, assemble.boundary_dofs(kvs, 'right', ravel=True)[:1])
    MP.finalize()
    assert not MP.injective
    S = _small_system(MP)
    try:
        with pytest.raises(_lib.IgxError) as e:
            S.solve(precond='schwarz')
        assert e.value.code == _lib.IGX_ERR_UNSUPPORTED
        u = S.solve(tol=1e-10, maxiter=5000, precond='jacobi')
        assert S.info['converged']
        A = S.matrix()
        free = np.setdiff1d(np.arange(S.n), S.bc_indices)
        lifted = np.zeros(S.n)
        lifted[S.bc_indices] = S.bc_values
        assert np.linalg.norm((S.b - A @ u)[free]) <= 2e-10 * np.linalg.norm((S.b - A @ lifted)[free])
    finally:
        S.close()
        MP.close()


def test_abi_refusals():
    lib = _lib.load()
    MP = _two_squares(p=2, n=3)
    h = MP._device()
    n = MP.numdofs
    none = np.zeros(0, dtype=np.int64)
    i64 = C.POINTER(C.c_int64)
    out = C.c_void_p()
    for nc in (1, 4):
        assert lib.igx_solver_create_multipatch_block(h, nc, 1, none.ctypes.data_as(i64), 0, C.byref(out)) == _lib.IGX_ERR_ARG
    bad = np.array([2 * n], dtype=np.int64)
    assert lib.igx_solver_create_multipatch_block(h, 2, 1, bad.ctypes.data_as(i64), 1, C.byref(out)) == _lib.IGX_ERR_ARG
    ok = np.array([2 * n - 1], dtype=np.int64)                     # the last blocked index is in range
    assert lib.igx_solver_create_multipatch_block(h, 2, 0, ok.ctypes.data_as(i64), 1, C.byref(out)) == _lib.IGX_OK
    s = out.value
    patterns = [sc.patch_pattern(tuple(kvs)) for kvs, _ in MP.patches]
    ones = [np.ones(Sp.nnz) for Sp in patterns]
    try:
        assert lib.igx_solver_set_method(s, _lib.IGX_METHOD_CG) == _lib.IGX_ERR_UNSUPPORTED
        _lib.check(lib.igx_multipatch_zero(h), 'igx_multipatch_zero')
        assert lib.igx_solver_take_multipatch_block(s, 0, 0) == _lib.IGX_ERR_ARG       # restarted, nothing scattered
        for k, v in enumerate(ones):
            _lib.check(lib.igx_multipatch_scatter_host(h, k, _lib.dptr(v)), 'igx_multipatch_scatter_host')
        assert lib.igx_solver_take_multipatch_block(s, 2, 0) == _lib.IGX_ERR_ARG
        assert lib.igx_solver_take_multipatch_block(s, 0, -1) == _lib.IGX_ERR_ARG
        assert lib.igx_solver_take_multipatch_block(s, 0, 0) == _lib.IGX_OK
        assert lib.igx_solver_take_multipatch_block(s, 0, 0) == _lib.IGX_ERR_ARG       # taken twice
        d_x, d_y = DeviceArray.from_host(MP._ctx, np.ones(2 * n)), DeviceArray(MP._ctx, 2 * n)
        assert lib.igx_solver_spmv_d(s, d_x.ptr, d_y.ptr) == _lib.IGX_ERR_ARG          # diagonal block (1, 1) missing
        assert 'diagonal block (1, 1)' in _lib.last_error()
        assert lib.igx_solver_take_multipatch_block(s, 1, 1) == _lib.IGX_OK
        assert lib.igx_solver_spmv_d(s, d_x.ptr, d_y.ptr) == _lib.IGX_OK
        u, g = np.empty(2 * n), np.zeros(1)
        assert lib.igx_solver_solve(s, None, _lib.dptr(g), None, 1e-8, 10, 1, 0, _lib.dptr(u), None) == _lib.IGX_ERR_ARG   # b = NULL
        for precond in (_lib.IGX_PRECOND_KRON, _lib.IGX_PRECOND_MG):
            assert lib.igx_solver_set_precond(s, precond, None, None, None, None, 0) == _lib.IGX_ERR_UNSUPPORTED
        assert lib.igx_solver_set_precond(s, _lib.IGX_PRECOND_SCHWARZ, None, None, None, None, 0) == _lib.IGX_ERR_ARG    # no factors yet
        assert lib.igx_solver_set_schwarz(s, None, None, None, None, 1) == _lib.IGX_ERR_UNSUPPORTED
        # the eigen, parabolic, stepping and Newton calls
        assert lib.igx_solver_set_mass_d(s, d_x.ptr) == _lib.IGX_ERR_UNSUPPORTED
        assert lib.igx_solver_eig_begin(s, 4, None, 0) == _lib.IGX_ERR_UNSUPPORTED
        assert lib.igx_solver_take_values(s, _lib.IGX_ROLE_MASS) == _lib.IGX_ERR_UNSUPPORTED
        tab = np.array([1.0, 1.0])
        assert lib.igx_solver_set_dirk(s, 1, _lib.dptr(tab), 0.1) == _lib.IGX_ERR_UNSUPPORTED
        assert lib.igx_solver_set_stepper(s, _lib.IGX_STEPPER_DIRK, 1, _lib.dptr(tab), None, None, None) == _lib.IGX_ERR_UNSUPPORTED
        assert lib.igx_solver_step_accept(s) == _lib.IGX_ERR_UNSUPPORTED
        assert lib.igx_solver_declare_symmetric(s) == _lib.IGX_ERR_UNSUPPORTED
        assert lib.igx_solver_set_mg_inverse(s, _lib.dptr(tab), 1) == _lib.IGX_ERR_UNSUPPORTED
    finally:
        lib.igx_solver_destroy(s)
        MP.close()

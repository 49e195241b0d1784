"""The kernels of csrc/solve_saddle.hip through the C ABI: k_pair_transpose bit for bit, the two row kernels (k_saddle_u,
k_saddle_p) at every (width, nc) instantiation of their dispatch tables against a long-double row sum, the lifting call (b,
sign = -1, an unmasked x) and the dot partials held to the same row bound through igx_solver_saddle_product_d, three MINRES
iterations against the host model, the breakdowns, and the block-diagonal preconditioner against the model's.

Bound of a row of the product: (len + C) 2^-53 sum |v x|, len the entries of the row of K = [[A, B^T], [B, 0]] and C = 10 counted
from the kernels: the lanes of a group add their terms in batches (within len), the shuffle tree adds log2(GW) <= 6 levels, the
result is multiplied by s and added to b (2), and the row of B^T is appended to the accumulators of the row of A (1); 1 spare."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse

from oracle import iga_oracle as orc
from pyiga_amd import _lib, bspline, geometry
from pyiga_amd.assemblers import DevicePair, DevicePatch
from pyiga_amd.operators import DeviceArray

import _pair_cases as pc
import _saddle_cases as sc
import _saddle_model as sm
from _saddle_systems import system

pytestmark = pytest.mark.gpu

LD = np.longdouble
C_TREE = 10


def _geo(dim):
    return geometry.quarter_annulus() if dim == 2 else geometry.twisted_box()


def _boundary(ndofs):
    m = np.ones(ndofs, dtype=bool)
    m[tuple(slice(1, -1) if n > 2 else slice(0, 0) for n in ndofs)] = False
    return np.nonzero(m.ravel())[0]


class Built:
    """A saddle solver over a kernel case, made through the C ABI, with host copies of every block."""

    def __init__(self, case):
        lib = _lib.load()
        kvs_u, kvs_p = sc.kernel_kvs(case, bspline)
        d, nc = len(kvs_u), case.nc
        q = max(kv.p for kv in kvs_u + kvs_p) + 1
        self.patch = DevicePatch(kvs_u, _geo(d), nqp=q)
        self.pair = DevicePair(self.patch, kvs_p)
        self.nc, self.N, self.Np = nc, int(np.prod(self.patch.ndofs)), self.pair.shape[0]
        self.n = nc * self.N + self.Np
        bd = _boundary(self.patch.ndofs)
        fixed = [bd + c * self.N for c in range(nc)]
        if case.pinned:
            fixed.append(np.array([0, self.Np // 2]) + nc * self.N)
        self.fixed = np.ascontiguousarray(np.concatenate(fixed), dtype=np.int64)
        self.free = np.ones(self.n, dtype=bool)
        self.free[self.fixed] = False
        h = C.c_void_p()
        _lib.check(lib.igx_solver_create_saddle(self.patch.handle, self.pair.handle, nc, self.fixed.ctypes.data_as(C.POINTER(C.c_int64)),
                                                self.fixed.size, C.byref(h)), 'igx_solver_create_saddle')
        self.handle = h.value
        none4 = lambda: [[None] * 4 for _ in range(4)]
        self.A = [[None] * nc for _ in range(nc)]
        for p in range(nc):
            for qq in range(nc):
                if (p, qq) in case.absent:
                    continue
                tab = none4()
                tab[0][0] = 1.0 + p + 2 * qq if p == qq else 0.25 * (1 + p + qq)
                if p == qq:
                    tab[1][1] = tab[2][2] = 1.0
                self.patch.set_form(tab)
                self.A[p][qq] = scipy.sparse.csr_matrix(self.patch.csr('form'))
                self.patch.assemble('form', to_host=False)
                _lib.check(lib.igx_solver_take_block(self.handle, p, qq), 'igx_solver_take_block')
        self.B = []
        for qq in range(nc):
            tab = none4()
            if qq < d:
                tab[0][1 + qq] = 1.0                        # p d_q u
            else:
                tab[0][0] = 2.0
            self.patch.set_form(tab)
            Bq = scipy.sparse.csr_matrix(self.pair.csr('form'))
            Bq.sort_indices()
            self.B.append(Bq)
            self.pair.assemble('form', to_host=False)
            _lib.check(lib.igx_solver_take_pair_block(self.handle, self.pair.handle, qq), 'igx_solver_take_pair_block')
        Z = [[a if a is not None else scipy.sparse.csr_matrix((self.N, self.N)) for a in row] for row in self.A]
        Am, Bm = scipy.sparse.bmat(Z, format='csr'), scipy.sparse.hstack(self.B, format='csr')
        self.Am, self.Bm = Am, Bm
        self.K = scipy.sparse.bmat([[Am, Bm.T], [Bm, None]], format='csr')
        self.K.sort_indices()

    def op(self, fn, x):
        ctx = self.patch.ctx
        d_x, d_y = DeviceArray.from_host(ctx, np.ascontiguousarray(x)), DeviceArray(ctx, self.n)
        _lib.check(fn(self.handle, d_x.ptr, d_y.ptr), 'device op')
        return d_y.download()

    def close(self):
        _lib.load().igx_solver_destroy(self.handle)
        self.pair.close()
        self.patch.close()


@pytest.fixture(scope='module')
def built():
    cache = {}

    def get(cid):
        if cid not in cache:
            cache[cid] = Built(sc.KERNEL_BY_ID[cid])
        return cache[cid]
    yield get
    for b in cache.values():
        b.close()


@pytest.mark.parametrize('cid', [c.id for c in sc.KERNEL_CASES])
def test_transpose_bit_for_bit(cid, built):
    """The downloaded B_q has the bits of the pair's csr() values, and the downloaded B_q^T those of its host transpose."""
    S = built(cid)
    lib = _lib.load()
    for q, Bq in enumerate(S.B):
        v, vt = np.empty(Bq.nnz), np.empty(Bq.nnz)
        _lib.check(lib.igx_solver_download_pair_block(S.handle, q, 0, _lib.dptr(v)), 'igx_solver_download_pair_block')
        _lib.check(lib.igx_solver_download_pair_block(S.handle, q, 1, _lib.dptr(vt)), 'igx_solver_download_pair_block')
        T = Bq.T.tocsr()
        T.sort_indices()
        assert np.array_equal(v.view(np.int64), Bq.data.view(np.int64))
        assert np.array_equal(vt.view(np.int64), T.data.view(np.int64))
    assert lib.igx_solver_download_pair_block(S.handle, S.nc, 0, _lib.dptr(v)) == 1


@pytest.mark.parametrize('cid', ['th2', 'th3', 'q1p0', 'hi2', 'lo2'])
def test_transpose_of_the_pair_cases(cid):
    """The pair cases of tests/_pair_cases.py (2D, 3D, degree 0 with a single-span axis, multiplicity 3): the mass matrix of the
    pair taken as B_0, B_0^T bit for bit the host transpose."""
    case = pc.BY_ID[cid]
    lib = _lib.load()
    kvs_u, kvs_p = case.kvs(bspline)
    patch = DevicePatch(kvs_u, _geo(case.dim) if case.geo != 'quarter_annulus' else geometry.quarter_annulus(), nqp=case.q())
    pair = DevicePair(patch, kvs_p)
    h = C.c_void_p()
    try:
        _lib.check(lib.igx_solver_create_saddle(patch.handle, pair.handle, 2, None, 0, C.byref(h)), 'igx_solver_create_saddle')
        B = scipy.sparse.csr_matrix(pair.csr('mass'))
        B.sort_indices()
        pair.assemble('mass', to_host=False)
        _lib.check(lib.igx_solver_take_pair_block(h, pair.handle, 1), 'igx_solver_take_pair_block')
        v, vt = np.empty(B.nnz), np.empty(B.nnz)
        _lib.check(lib.igx_solver_download_pair_block(h, 1, 0, _lib.dptr(v)), 'igx_solver_download_pair_block')
        _lib.check(lib.igx_solver_download_pair_block(h, 1, 1, _lib.dptr(vt)), 'igx_solver_download_pair_block')
        T = B.T.tocsr()
        T.sort_indices()
        assert B.shape == case.shape and B.nnz == case.nnz
        assert np.array_equal(v.view(np.int64), B.data.view(np.int64)) and np.array_equal(vt.view(np.int64), T.data.view(np.int64))
    finally:
        if h.value:
            lib.igx_solver_destroy(h)
        pair.close()
        patch.close()


def _row_sums(K, x):
    t = K.data.astype(LD) * x[K.indices].astype(LD)
    lens = np.diff(K.indptr)
    starts = K.indptr[:-1][lens > 0]
    ref, mag = np.zeros(K.shape[0], dtype=LD), np.zeros(K.shape[0], dtype=LD)
    ref[lens > 0] = np.add.reduceat(t, starts)
    mag[lens > 0] = np.add.reduceat(abs(t), starts)
    return ref, mag, lens


@pytest.mark.parametrize('cid', [c.id for c in sc.KERNEL_CASES])
def test_row_kernels(cid, built):
    """igx_solver_spmv_d = R K R^T x at the case's widths: every row within the bound, masked rows exactly 0."""
    S = built(cid)
    case = sc.KERNEL_BY_ID[cid]
    x = np.random.default_rng(sum(map(ord, cid))).standard_normal(S.n)
    y = S.op(_lib.load().igx_solver_spmv_d, x)
    ref, mag, lens = _row_sums(S.K, np.where(S.free, x, 0.0))
    bound = (lens + C_TREE) * LD(2.0) ** -53 * mag
    assert not y[~S.free].any()
    nv = S.nc * S.N
    ru = (abs(y.astype(LD) - ref) / bound)[:nv][S.free[:nv]].max()
    rp = (abs(y.astype(LD) - ref) / bound)[nv:][S.free[nv:]].max()
    print('%s: widths %s, nc %d, largest |dev - ref| / bound: velocity rows %.3f, pressure rows %.3f'
          % (cid, sc.widths(case.trial, case.test), case.nc, float(ru), float(rp)))
    assert ru <= 1.0 and rp <= 1.0


def _product(S, x, b, sign, pd):
    """(y, dot) of igx_solver_saddle_product_d; b and pd host vectors or None."""
    ctx = S.patch.ctx
    up = lambda v: None if v is None else DeviceArray.from_host(ctx, np.ascontiguousarray(v))
    d_x, d_b, d_pd, d_y = up(x), up(b), up(pd), DeviceArray(ctx, S.n)
    dot = C.c_double(np.nan)
    _lib.check(_lib.load().igx_solver_saddle_product_d(S.handle, d_x.ptr, None if d_b is None else d_b.ptr, float(sign),
                                                       None if d_pd is None else d_pd.ptr, d_y.ptr, C.byref(dot)),
               'igx_solver_saddle_product_d')
    return d_y.download(), dot.value


@pytest.mark.parametrize('cid', [c.id for c in sc.KERNEL_CASES])
def test_lifting_call_and_dot_partials(cid, built):
    """The call the lifting makes -- y = free ? b - K x : 0 with an x that is NOT zero on the fixed dofs -- and the dot partials,
    at the case's widths.  Every free row within (len + 1 + C) 2^-53 (|b| + sum |v x|) of the long-double row sum (1: the term b);
    masked rows exactly 0; the same bits with the partials off.  The partials, added up on the device in their fixed order:
    within (rows + C_DOT) 2^-53 sum |pd y| of the long-double pd . y over the DEVICE's y, rows the number of rows and C_DOT = 24:
    a lane adds the rows of its group one after the other (within rows), the tree of a block has log2(256) = 8 levels, the one-block
    sum of the partials another 8 after its strided adds (within rows), and every product pd y is rounded once (1); the rest spare."""
    S = built(cid)
    case = sc.KERNEL_BY_ID[cid]
    rng = np.random.default_rng(11 + sum(map(ord, cid)))
    x, b, pd = rng.standard_normal(S.n), rng.standard_normal(S.n), rng.standard_normal(S.n)
    y, dot = _product(S, x, b, -1.0, pd)
    y0, dot0 = _product(S, x, b, -1.0, None)
    assert np.array_equal(y.view(np.int64), y0.view(np.int64)) and dot0 == 0.0
    kx, mag, lens = _row_sums(S.K, x)
    ref = b.astype(LD) - kx
    bound = (lens + 1 + C_TREE) * LD(2.0) ** -53 * (abs(b).astype(LD) + mag)
    assert not y[~S.free].any()
    nv = S.nc * S.N
    ratio = abs(y.astype(LD) - ref) / bound
    ru, rp = ratio[:nv][S.free[:nv]].max(), ratio[nv:][S.free[nv:]].max()
    t = pd.astype(LD) * y.astype(LD)
    rd = abs(LD(dot) - t.sum()) / ((S.n + 24) * LD(2.0) ** -53 * abs(t).sum())
    print('%s: lifting call, largest |dev - ref| / bound: velocity rows %.3f, pressure rows %.3f; dot partials %.4f'
          % (cid, float(ru), float(rp), float(rd)))
    assert ru <= 1.0 and rp <= 1.0 and rd <= 1.0
    # the plain product with partials: b = NULL, s = +1
    y1, dot1 = _product(S, x, None, 1.0, pd)
    r1 = (abs(y1.astype(LD) - kx) / ((lens + C_TREE) * LD(2.0) ** -53 * mag))[S.free].max()
    t1 = pd.astype(LD) * y1.astype(LD)
    assert r1 <= 1.0 and abs(LD(dot1) - t1.sum()) <= (S.n + 24) * LD(2.0) ** -53 * abs(t1).sum()
    tr, tu, tp = C.c_float(), C.c_float(), C.c_float()
    _lib.check(_lib.load().igx_solver_saddle_timing(S.handle, C.byref(tr), C.byref(tu), C.byref(tp)), 'igx_solver_saddle_timing')
    assert tr.value > 0.0 and tu.value > 0.0 and tp.value > 0.0


@pytest.mark.parametrize('cid', [c.id for c in sc.KERNEL_CASES])
def test_three_iterations_against_the_model(cid, built):
    """Three MINRES iterations without a preconditioner from Dirichlet data g != 0 and b != 0 -- the lifting, the products with
    their partials and the fused updates in the solver's own sequence -- against the host model on the host copies of the blocks.
    Accepted: 50 (len + C) 2^-53 of max |u|, len the longest row of K: the five products of the run (lifting, three iterations,
    final residual) are each within (len + C) 2^-53 of their rows' magnitude sums, which exceed the rows' values by less than 10
    for these random data."""
    S = built(cid)
    lib = _lib.load()
    rng = np.random.default_rng(7 + sum(map(ord, cid)))
    b, g = rng.standard_normal(S.n), rng.standard_normal(S.fixed.size)
    u = np.empty(S.n)
    info = _lib.SolveInfo()
    _lib.check(lib.igx_solver_set_precond(S.handle, _lib.IGX_PRECOND_NONE, None, None, None, None, 0), 'igx_solver_set_precond')
    _lib.check(lib.igx_solver_saddle_projection(S.handle, 0, None, None), 'igx_solver_saddle_projection')
    _lib.check(lib.igx_solver_solve(S.handle, _lib.dptr(b), _lib.dptr(g), None, 1e-30, 3, 1, 0, _lib.dptr(u), C.byref(info)),
               'igx_solver_solve')
    um, minfo = sm.solve(S.Am, S.Bm, S.nc, (S.fixed, g), b=b, tol=1e-30, maxiter=3)
    assert info.iterations == 3 == minfo['iterations'] and lib.igx_solver_last_breakdown(S.handle) == 0
    tol = 50 * (int(np.diff(S.K.indptr).max()) + C_TREE) * 2.0 ** -53
    err = abs(u - um).max() / abs(um).max()
    print('%s: three iterations, |dev - model| / max |model| = %.2e (allowed %.2e), relres %.3e (model %.3e)'
          % (cid, err, tol, info.relres, minfo['relres']))
    assert err <= tol and abs(info.relres - minfo['relres']) <= tol * minfo['relres']
    assert np.array_equal(u[S.fixed], g)


def test_breakdowns(built):
    """A negative entry in the Jacobi Schur part makes the preconditioner indefinite: MINRES stops before its first update with
    IGX_BREAKDOWN_INDEFINITE_PRECOND, not converged, and returns the start vector (0 on the free dofs, g on the fixed ones).  A
    scale that is not positive is refused.  A NaN right-hand side stops as IGX_BREAKDOWN_NONFINITE with the start vector."""
    S = built('th21-3')
    lib = _lib.load()
    dinv = np.ones(S.Np)
    assert lib.igx_solver_set_saddle_schur(S.handle, _lib.IGX_PRECOND_JACOBI, None, None, None, None, 0, _lib.dptr(dinv), -1.0) == 1
    dinv = np.full(S.Np, -1e6)
    _lib.check(lib.igx_solver_set_saddle_schur(S.handle, _lib.IGX_PRECOND_JACOBI, None, None, None, None, 0, _lib.dptr(dinv), 1.0),
               'igx_solver_set_saddle_schur')
    _lib.check(lib.igx_solver_set_precond(S.handle, _lib.IGX_PRECOND_JACOBI, None, None, None, None, 0), 'igx_solver_set_precond')
    rng = np.random.default_rng(1)
    b, g = rng.standard_normal(S.n), rng.standard_normal(S.fixed.size)
    u, info = np.empty(S.n), _lib.SolveInfo()
    _lib.check(lib.igx_solver_solve(S.handle, _lib.dptr(b), _lib.dptr(g), None, 1e-8, 50, 1, 0, _lib.dptr(u), C.byref(info)), 'igx_solver_solve')
    assert not info.converged and info.iterations == 0
    assert lib.igx_solver_last_breakdown(S.handle) == _lib.IGX_BREAKDOWN_INDEFINITE_PRECOND == 5
    assert not u[S.free].any() and np.array_equal(u[S.fixed], g)
    _lib.check(lib.igx_solver_set_precond(S.handle, _lib.IGX_PRECOND_NONE, None, None, None, None, 0), 'igx_solver_set_precond')
    b = np.full(S.n, np.nan)
    _lib.check(lib.igx_solver_solve(S.handle, _lib.dptr(b), _lib.dptr(g), None, 1e-8, 5, 1, 0, _lib.dptr(u), C.byref(info)), 'igx_solver_solve')
    assert not info.converged and lib.igx_solver_last_breakdown(S.handle) == _lib.IGX_BREAKDOWN_NONFINITE
    assert not u[S.free].any() and np.array_equal(u[S.fixed], g)


@pytest.mark.parametrize('which', ['unpinned', 'pinned'])
def test_preconditioner_against_the_model(which, golden):
    """igx_solver_precond_d of SaddlePointSystem on the notebook system against the model's diag(F, F, M_p^-1), with and without
    the pinned pressure dof.  Accepted: 1e-11 of max |z| -- both sides factor the same 1D matrices; cond(M_k) ~ 1e3 times 2^-53
    per axis and factor."""
    S, nv = system('stokes', which)
    try:
        free = np.ones(S.n, dtype=bool)
        free[S.bc_indices] = False
        P = sc.model_preconditioner(sc.system(golden, 'stokes'), free, orc)
        r = np.random.default_rng(3).standard_normal(S.n)
        z = S.apply_precond(r, 'kron')
        ref = P(np.where(free, r, 0.0))
        err = abs(z - ref).max() / abs(ref).max()
        print('precond_d (%s): |dev - model| / max |model| = %.2e' % (which, err))
        assert err <= 1e-11 and not z[~free].any()
        zj = S.apply_precond(r, 'jacobi')
        assert not zj[~free].any() and (zj[free] * r[free] > 0).all()
    finally:
        S.close()

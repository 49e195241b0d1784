"""The kernels of the device GMRES (csrc/solve_gmres.hip) through the inspection calls igx_solver_gmres_orth_d and
igx_solver_gmres_combine_d, against long-double sums; the B^T-only call of k_saddle_u and the triangular preconditioner against
the host model.

The vector kernels walk all n entries of the solver's vectors and know no mask: the fixed entries of w and of the columns of V hold
zeros here, as every vector of a solve does, and `free` counts the entries that do not.  Shapes (tests/_oseen_cases.py): on the
oseen2 patch (n = 328, two blocks of 256, a tail of 72) free = 1, 63, 64, 65, 256, 257; on a plain patch of 394582 entries the
grid-stride loops of all kernels wrap (more than NB_VEC blocks of 256).  Columns 1, 7, 8, 9, 17, 41: the tail of a chunk of MB = 8,
one chunk, a chunk and one, several chunks, and restart + 1.

Bounds, u = 2^-53, first order, composed over the two Gram-Schmidt passes from the reference's own long-double intermediates:
  a coefficient of one pass   (n + C_DOT) u sum_i |v_ik w_i|, plus sum_i |v_ik| (the bound of w_i) in the second pass
  an entry of w after a pass  (cols + C_UPD) u (|w_i| + sum_k |h_k v_ik|), plus what it inherited: its own bound before the pass and
                              sum_k (the bound of h_k) |v_ik|
  the norm                    ((n + C_DOT) u sum w_i^2 + 2 sum |w_i| (the bound of w_i)) / (2 ||w||) + u ||w||
C_DOT and C_UPD are counted in _oseen_cases.py from the reduction tree and the operation chain."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse

from pyiga_amd import _lib, assemble, geometry
from pyiga_amd.assemblers import DevicePair, DevicePatch
from pyiga_amd.operators import DeviceArray

import _oseen_cases as oc
import _saddle_cases as sc
from _oseen_systems import system as _system
from _saddle_systems import problem as _problem

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = LD(2.0) ** -53


class _Raw:
    """A saddle-point solver without values over a patch, GMRES(40) selected: what the inspection calls need."""

    def __init__(self, kvs_u, kvs_p, geo, nfree, seed):
        self.patch = DevicePatch(kvs_u, geo, nqp=max(kv.p for kv in kvs_u) + 1)
        self.pair = DevicePair(self.patch, kvs_p)
        self.n = 2 * int(np.prod([kv.numdofs for kv in kvs_u])) + int(np.prod([kv.numdofs for kv in kvs_p]))
        rng = np.random.default_rng(seed)
        self.free = np.zeros(self.n, dtype=bool)
        self.free[rng.choice(self.n, size=min(nfree, self.n), replace=False)] = True
        fixed = np.ascontiguousarray(np.nonzero(~self.free)[0], dtype=np.int64)
        lib = _lib.load()
        h = C.c_void_p()
        _lib.check(lib.igx_solver_create_saddle(self.patch.handle, self.pair.handle, 2, fixed.ctypes.data_as(C.POINTER(C.c_int64)),
                                                fixed.size, C.byref(h)), 'igx_solver_create_saddle')
        self.handle = h.value
        _lib.check(lib.igx_solver_set_gmres(self.handle, oc.RESTART, 0), 'igx_solver_set_gmres')
        self.ctx = self.patch.ctx

    def close(self):
        _lib.load().igx_solver_destroy(self.handle)
        self.pair.close()
        self.patch.close()


@pytest.fixture(scope='module')
def raw():
    made = {}

    def get(nfree):
        if nfree not in made:
            if nfree == 'grid':
                from pyiga_amd import bspline
                kvs_u, kvs_p = sc.kernel_kvs(sc.KernelCase('grid', oc.GRID_SPACES[0], oc.GRID_SPACES[1], 2, (), False), bspline)
                made[nfree] = _Raw(kvs_u, kvs_p, geometry.quarter_annulus(), 10 ** 9, 1)
                made[nfree].free[::1000] = False             # (zeros among the entries, as fixed dofs leave them)
            else:
                kvs_u, kvs_p, geo, _, _ = _problem('stokes')
                made[nfree] = _Raw(kvs_u, kvs_p, geo, nfree, 100 + nfree)
        return made[nfree]
    yield get
    for s in made.values():
        s.close()


def _vectors(S, cols, seed):
    """(V, w): V (cols, n) with orthonormal rows when there are enough free entries, w random; zeros on the fixed entries."""
    rng = np.random.default_rng(seed)
    nf = int(S.free.sum())
    V = np.zeros((cols, S.n))
    if nf >= cols:
        Q, _ = np.linalg.qr(rng.standard_normal((nf, cols)))
        V[:, S.free] = Q.T
    else:
        V[:, S.free] = rng.standard_normal((cols, nf)) / np.sqrt(cols)
    w = np.zeros(S.n)
    w[S.free] = rng.standard_normal(nf)
    return np.ascontiguousarray(V), w


def _check_orth(S, cols, seed):
    lib = _lib.load()
    V, w = _vectors(S, cols, seed)
    d_V, d_w = DeviceArray.from_host(S.ctx, V.ravel()), DeviceArray.from_host(S.ctx, w)
    h = np.full(cols, np.nan)
    norm = C.c_double(np.nan)
    _lib.check(lib.igx_solver_gmres_orth_d(S.handle, d_V.ptr, cols, d_w.ptr, _lib.dptr(h), C.byref(norm)), 'igx_solver_gmres_orth_d')
    wd = d_w.download()
    n = S.n
    Vl, aV = V.astype(LD), abs(V).astype(LD)
    wl = w.astype(LD)
    eh = np.zeros(cols, dtype=LD)
    ew = np.zeros(n, dtype=LD)
    href = np.zeros(cols, dtype=LD)
    for _ in range(2):
        hp = Vl @ wl
        ehp = (n + oc.C_DOT) * U * (aV @ abs(wl)) + aV @ ew
        ew = (cols + oc.C_UPD) * U * (abs(wl) + abs(hp) @ aV) + ew + ehp @ aV
        wl = wl - hp @ Vl
        href += hp
        eh += ehp
    eh += U * abs(href)
    nref = np.sqrt(wl @ wl)
    en = ((n + oc.C_DOT) * U * (wl @ wl) + 2 * (abs(wl) @ ew)) / (2 * nref) + U * nref if nref > 0 else LD(0)
    tiny = LD(1e-300)
    rh = float((abs(h.astype(LD) - href) / (eh + tiny)).max())
    rw = float((abs(wd.astype(LD) - wl) / (ew + tiny)).max())
    rn = float(abs(LD(norm.value) - nref) / (en + tiny))
    assert not wd[~S.free].any()
    return rh, rw, rn


@pytest.mark.parametrize('cols', oc.COLUMNS)
@pytest.mark.parametrize('nfree', oc.SMALL_FREE)
def test_orthogonalisation(nfree, cols, raw):
    rh, rw, rn = _check_orth(raw(nfree), cols, 7 * nfree + cols)
    print('orth free %d cols %d: largest error / bound: h %.3f, w %.3f, norm %.3f' % (nfree, cols, rh, rw, rn))
    assert rh <= 1.0 and rw <= 1.0 and rn <= 1.0


@pytest.mark.parametrize('cols', oc.GRID_COLUMNS)
def test_orthogonalisation_past_a_grid(cols, raw):
    S = raw('grid')
    assert oc.vec_blocks(S.n) == oc.NB_VEC and S.n > oc.NB_VEC * oc.BLOCK and oc.dot_blocks(S.n) < oc.NB_VEC
    rh, rw, rn = _check_orth(S, cols, cols)
    print('orth n %d cols %d: largest error / bound: h %.3f, w %.3f, norm %.3f' % (S.n, cols, rh, rw, rn))
    assert rh <= 1.0 and rw <= 1.0 and rn <= 1.0
    t = C.c_float()
    _lib.check(_lib.load().igx_solver_gmres_timing(S.handle, C.byref(t), None), 'igx_solver_gmres_timing')
    assert t.value > 0.0


@pytest.mark.parametrize('key', [(1, 1), (63, 7), (64, 8), (65, 9), (256, 17), (257, 41), ('grid', 9), ('grid', 17)])
def test_combine(key, raw):
    """t = sum_k y_k v_k against the long-double sum, entry-wise within (cols + 1) u sum_k |y_k v_ik|: one rounding per product
    (or fused multiply-add) of the chain and the store."""
    nfree, cols = key
    S = raw(nfree)
    V, _ = _vectors(S, cols, 31 + cols)
    y = np.random.default_rng(cols).standard_normal(cols)
    d_V, d_t = DeviceArray.from_host(S.ctx, V.ravel()), DeviceArray(S.ctx, S.n)
    _lib.check(_lib.load().igx_solver_gmres_combine_d(S.handle, d_V.ptr, cols, _lib.dptr(y), d_t.ptr), 'igx_solver_gmres_combine_d')
    t = d_t.download()
    ref = y.astype(LD) @ V.astype(LD)
    bound = (cols + 1) * U * (abs(y).astype(LD) @ abs(V).astype(LD))
    ratio = float((abs(t.astype(LD) - ref) / (bound + LD(1e-300))).max())
    print('combine %s cols %d: largest error / bound %.3f' % (nfree, cols, ratio))
    assert ratio <= 1.0 and not t[~S.free].any()


@pytest.mark.parametrize('name', oc.CASES)
def test_bt_only_call_of_the_velocity_rows(name, golden):
    """k_saddle_u with every block of A absent (nc = 2 and 3), reached as the triangular preconditioner reaches it: Jacobi parts,
    r_u = 0, so that z_u = dinv_u * (-(B^T z_p)) with z_p the device's own pressure part.  dinv_u is read off the diagonal form
    (r_u = 1).  Row-wise within (len + 10 + 1) u dinv_u sum |v z_p|: the bound of the saddle kernel tests and one more rounding for
    the product with dinv_u."""
    M = oc.system(golden, name)
    S, nv = _system(name, M.nu)
    try:
        geo = geometry.quarter_annulus() if name == 'oseen2' else geometry.twisted_box()
        B = scipy.sparse.csr_matrix(assemble.assemble('div(u) * p * dx', (S.kvs, S.kvs_p), bfuns=[('u', S.ncomp, 0), ('p', 1, 1)], geo=geo))
        BT = B.T.tocsr()
        free = np.ones(S.n, dtype=bool)
        free[S.bc_indices] = False
        ones = np.concatenate((np.ones(nv), np.zeros(S.n - nv)))
        dinv = S.apply_precond(ones, 'jacobi', triangular=False)[:nv]
        r = np.concatenate((np.zeros(nv), np.random.default_rng(9).standard_normal(S.n - nv)))
        z = S.apply_precond(r, 'jacobi', triangular=True)
        zp = z[nv:].astype(LD)
        assert not z[~free].any() and (z[nv:][free[nv:]] * r[nv:][free[nv:]] < 0).all()          # (z_p = -P_S r_p)
        worst = 0.0
        for i in np.nonzero(free[:nv])[0]:
            sl = slice(BT.indptr[i], BT.indptr[i + 1])
            t = BT.data[sl].astype(LD) * zp[BT.indices[sl]]
            ref, mag = -t.sum() * LD(dinv[i]), abs(t).sum() * LD(dinv[i])
            bound = (t.size + 11) * U * mag
            if bound > 0:
                worst = max(worst, float(abs(LD(z[i]) - ref) / bound))
            else:
                assert z[i] == 0.0
        print('%s (nc = %d): B^T-only rows, largest error / bound %.3f' % (name, S.ncomp, worst))
        assert worst <= 1.0
    finally:
        S.close()


@pytest.mark.parametrize('name', oc.CASES)
def test_triangular_preconditioner_against_the_model(name, golden):
    """igx_solver_precond_d with the triangular form selected against the model's solve with [[F, B^T], [0, -S]], within the 1e-11
    of max |z| the block-diagonal form is allowed (both sides factor the same 1D matrices)."""
    from oracle import iga_oracle as orc
    import _gmres_model as gm
    M = oc.system(golden, name)
    S, nv = _system(name, M.nu)
    try:
        free = np.ones(S.n, dtype=bool)
        free[S.bc_indices] = False
        P = sc.model_preconditioner(M, free, orc, viscosity=M.nu)
        T = gm.triangular_preconditioner(P, M.B, free, nv)
        r = np.random.default_rng(4).standard_normal(S.n)
        rm = np.where(free, r, 0.0)
        z = S.apply_precond(r, 'kron', triangular=True)
        err = abs(z - T(rm)).max() / abs(T(rm)).max()
        zd = S.apply_precond(r, 'kron', triangular=False)
        errd = abs(zd - P(rm)).max() / abs(P(rm)).max()
        print('%s: precond_d triangular |dev - model| / max = %.2e, diagonal %.2e' % (name, err, errd))
        assert err <= 1e-11 and errd <= 1e-11 and not z[~free].any()
        assert abs(z - zd)[:nv].max() > 1e-3 * abs(zd[:nv]).max()            # (the two forms differ)
    finally:
        S.close()

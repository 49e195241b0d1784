"""Every path of the load-vector kernels (csrc/kern_vector.hip; the generated copy of k_lv12 in csrc/rtc.hip) against a long-double
contraction with dense collocation matrices: the cases of tests/_lv_cases.py, which tests/test_lv_coverage_cpu.py ties to the
dispatch in the source.

Reference: C_k (2, G_k, N_k) = values and first derivatives of all basis functions at the patch's own Gauss nodes, by Cox-de Boor
in long double on the host (tests/_lv_model.py: nothing of the library); ref = C_0^T (x) C_1^T (x) C_2^T T in long double with
T = W f: W is the device's own weight field (patch.fields('mass')[0]), f the host's samples.

Bound, per entry:  |dev_i - ref_i| <= K eps B_i,  B = |C_0|^T (x) |C_1|^T (x) |C_2|^T |T|  from the same contraction, and
    K = sum_k P_k q + 8 + 18 p_max
sum_k P_k q: the fma chain of each axis; 8: the product W f, the atomic add of a shared dof, `accumulate`, second order; 18 p_max:
the device's Cox-de Boor tables are within 6 p roundings of the exact values on three factors (no cancellation in the values;
the derivative is a difference of two such values and is bounded against the row's absolute sum, which B contains).  At most
206 where k_lv12 runs (p <= 5, p + 1 points per span).  Derived, not fitted: a ratio above K is a finding.  The jet functional (WEIGHT = false: the weight is inside the
coefficient field) gets three more roundings.  Every test prints the largest observed |dev - ref| / (eps B)."""
import ctypes as C

import numpy as np
import pytest

from pyiga_amd import _lib, assemblers, geometry

import _lv_cases as lc
import _lv_model as lm

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
LD = np.longdouble
EXPR = '1 + x*y - 0.5*z*z + x*z'


@pytest.fixture(autouse=True)
def _wide_long_double():
    """First of all, in every test: the reference needs a long double wider than float64."""
    assert np.finfo(np.longdouble).eps < 2e-19


def _geo(case):
    if case.geo == 'cube':
        return geometry.unit_cube() if case.dim == 3 else geometry.unit_square()
    return geometry.quarter_annulus() if case.dim == 2 else geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.quarter_annulus())


def _cube(case):
    return geometry.unit_cube() if case.dim == 3 else geometry.unit_square()


def _K(case, extra=0):
    q = case.q()
    return sum((a[0] + 1) * q for a in case.axes) + 8 + 18 * max(a[0] for a in case.axes) + extra


def _tables(patch, kvs):
    return [lm.collocation_ld(kv, patch.gauss(k)[0]) for k, kv in enumerate(kvs)]


def _ratio(dev, ref, B):
    """max_i |dev_i - ref_i| / (eps B_i); an entry with B_i = 0 must be exact."""
    err = abs(dev.astype(LD) - ref)
    assert not (err[B == 0] != 0).any()
    return float((err[B > 0] / (EPS * B[B > 0])).max())


def _weights_ld(patch, dim):
    w = [patch.gauss(k)[1].astype(LD) for k in range(dim)]
    out = w[0]
    for x in w[1:]:
        out = out[..., None] * x
    return out


@pytest.mark.parametrize('cid', [c.id for c in lc.ALL_CASES])
def test_load_vector_against_long_double(cid):
    """WEIGHT = true: load_vector against the reference; the launch count says which path ran; a second call and two row slabs
    (the second starts past the first Gauss plane) give the same bits."""
    case = lc.BY_ID[cid]
    kvs, geo, dim, q = case.kvs(), _geo(case), case.dim, case.q()
    patch = assemblers.DevicePatch(kvs, geo, nqp=case.nqp)
    try:
        assert patch.nqp == q
        G = tuple(patch.info.ngauss[k] for k in range(dim))
        assert G == tuple(a.G for a in case.tables())
        f = np.random.default_rng(100 + len(cid)).uniform(-1.0, 1.0, G)
        dev = patch.load_vector(f)
        assert patch.timing()['n_launches'] == (2 if case.path == 'lv12' else dim)
        assert np.array_equal(patch.load_vector(f), dev)
        Cs = _tables(patch, kvs)
        W = patch.fields('mass')[0]
        assert W.shape == G
        T = W.astype(LD) * f.astype(LD)
        ref = lm.contract_ld(Cs, q, T)
        B = lm.contract_ld(Cs, q, T, absolute=True)
        K = _K(case)
        assert K <= 206 or case.path != 'lv12'          # (p <= 5 with p + 1 points per span; fb_PQ42: 249, fb_nqp13: 169)
        ratio = _ratio(dev, ref, B)
        print('lv %s (%s): max |dev - ref| / (eps B) = %.2f, K = %d' % (cid, case.path, ratio, K))
        assert ratio <= K
    finally:
        patch.close()
    cut = case.slab_cut()
    parts = []
    for k, row0 in enumerate(((0, cut), (cut, kvs[0].numdofs))):
        slab = assemblers.DevicePatch(kvs, geo, row0=row0, nqp=case.nqp)
        try:
            assert (slab.gauss_slab()[0] > 0) == (k == 1)
            parts.append(slab.load_vector(f))
            assert slab.timing()['n_launches'] == (2 if case.path == 'lv12' else dim)
        finally:
            slab.close()
    assert np.array_equal(np.concatenate(parts, axis=0), dev)


@pytest.mark.parametrize('cid', [c.id for c in lc.ALL_CASES])
def test_jet_functional_against_long_double(cid):
    """WEIGHT = false (what Newton's residual runs): the jet functional on the unit cube, where the coefficient fields are the
    Gauss weight products times the coefficient: the value alone, each gradient component alone (the differentiated axis is
    2, 1, 0), all together (accumulated), and the same from device arrays."""
    case = lc.BY_ID[cid]
    kvs, dim, q = case.kvs(), case.dim, case.q()
    patch = assemblers.DevicePatch(kvs, _cube(case), nqp=case.nqp)
    try:
        G = tuple(patch.info.ngauss[k] for k in range(dim))
        rng = np.random.default_rng(200 + len(cid))
        F = [rng.uniform(-1.0, 1.0, G) for _ in range(1 + dim)]
        Cs = _tables(patch, kvs)
        Wg = _weights_ld(patch, dim)
        K = _K(case, extra=3)
        refs, Bs, worst = [], [], 0.0
        for r in range(1 + dim):
            derivs = tuple(1 if r >= 1 and k == dim - r else 0 for k in range(dim))
            T = Wg * F[r].astype(LD)
            refs.append(lm.contract_ld(Cs, q, T, derivs))
            Bs.append(lm.contract_ld(Cs, q, T, derivs, absolute=True))
            jet = [None] * (1 + dim)
            jet[r] = F[r]
            dev = patch.load_vector_jet(jet)
            ratio = _ratio(dev, refs[r], Bs[r])
            worst = max(worst, ratio)
            assert ratio <= K, (cid, r, ratio, K)
        dev = patch.load_vector_jet(F)
        ratio = _ratio(dev, sum(refs), sum(Bs))
        worst = max(worst, ratio)
        print('jet %s (%s): max |dev - ref| / (eps B) = %.2f, K = %d' % (cid, case.path, worst, K))
        assert ratio <= K, (cid, 'all', ratio, K)
        assert np.array_equal(patch.load_vector_jet(F), dev)
        ptrs = patch.upload_fields(F)
        assert np.array_equal(patch.load_vector_jet_resident(ptrs, to_host=True), dev)
    finally:
        patch.close()


@pytest.mark.parametrize('cid', [c.id for c in lc.LV12_CASES])
def test_generated_copy_against_long_double(cid, tmp_path, monkeypatch):
    """igx_lv12_expr, the copy of k_lv12 with the function inside, for physical and parametric coordinates: the library entry
    itself returns IGX_OK (not IGX_ERR_UNSUPPORTED, after which DevicePatch.load_vector_expr would take the two-array path) in
    two launches.  Reference: the device's own samples of the same expression (eval_function_expr, read back from the patch's
    function buffer) times the device's weight field, contracted in long double."""
    monkeypatch.setenv('IGX_CACHE_DIR', str(tmp_path / 'cache'))
    case = lc.BY_ID[cid]
    kvs, geo, q = case.kvs(), _geo(case), case.q()
    lib = _lib.load()
    patch = assemblers.DevicePatch(kvs, geo, nqp=case.nqp)
    try:
        G = tuple(patch.info.ngauss[k] for k in range(3))
        Cs = _tables(patch, kvs)
        W = patch.fields('mass')[0].astype(LD)
        K = _K(case)
        for par in (True, False):
            one = np.empty(patch.ndofs)
            hit = C.c_int(0)
            rc = lib.igx_load_vector_expr(patch.handle, EXPR.encode(), 1 if par else 0, _lib.dptr(one), C.byref(hit))
            assert rc == _lib.IGX_OK, (cid, par, rc, _lib.last_error())
            assert patch.timing()['n_launches'] == 2
            assert np.array_equal(patch.load_vector_expr(EXPR, parametric=par), one)
            patch.eval_function_expr(EXPR, parametric=par)
            fdev = np.empty(G)
            _lib.check(lib.igx_dev_download(patch.ctx.handle, fdev.ctypes.data, patch._d_f[0], fdev.nbytes), 'igx_dev_download')
            T = W * fdev.astype(LD)
            ref = lm.contract_ld(Cs, q, T)
            B = lm.contract_ld(Cs, q, T, absolute=True)
            ratio = _ratio(one, ref, B)
            two = patch.load_vector_resident(to_host=True)             # k_lv12 itself on the same samples
            print('expr %s parametric=%d: max |dev - ref| / (eps B) = %.2f (k_lv12 on the samples: %.2f), K = %d'
                  % (cid, par, ratio, _ratio(two, ref, B), K))
            assert ratio <= K, (cid, par, ratio, K)
    finally:
        patch.close()


@pytest.mark.parametrize('cid', lc.ADJOINT_CASES)
def test_spline_evaluation_and_jet_functional_are_adjoint(cid):
    """k_spline12 and k_lv12 are each other's transpose: on the unit cube, for random dofs c and a random grid function h,
    sum(eval_spline(c)[d] W h) == sum(c * jet_functional(h in slot d)) for the value and the three derivatives.  No collocation
    matrix enters the identity; the tolerance is the sum of the two derived bounds: the spline test's (250 eps max|c| prod_k S_k
    per point, times dim for a derivative) summed against |W h|, and K eps sum_i |c_i| B_i."""
    case = lc.BY_ID[cid]
    kvs, dim, q = case.kvs(), case.dim, case.q()
    patch = assemblers.DevicePatch(kvs, geometry.unit_cube(), nqp=case.nqp)
    try:
        G = tuple(patch.info.ngauss[k] for k in range(dim))
        rng = np.random.default_rng(300 + len(cid))
        c = rng.uniform(-1.0, 1.0, patch.ndofs)
        h = rng.uniform(-1.0, 1.0, G)
        Cs = _tables(patch, kvs)
        Wg = _weights_ld(patch, dim)
        S = [[float(abs(Ck[d]).sum(axis=1).max()) for d in range(2)] for Ck in Cs]
        K = _K(case, extra=3)
        full = patch.eval_spline(patch.upload_dofs(c), want_grad=True, to_host=True)
        for d in range(1 + dim):
            derivs = tuple(1 if d >= 1 and k == dim - d else 0 for k in range(dim))
            lhs = (full[d].astype(LD) * Wg * h.astype(LD)).sum()
            jet = [None] * (1 + dim)
            jet[d] = h
            rhs = (c.astype(LD) * patch.load_vector_jet(jet).astype(LD)).sum()
            tol_spline = (dim if d else 1) * 250 * EPS * abs(c).max() * np.prod([S[k][derivs[k]] for k in range(dim)])
            B = lm.contract_ld(Cs, q, Wg * h.astype(LD), derivs, absolute=True)
            tol = tol_spline * abs(Wg * h.astype(LD)).sum() + K * EPS * (abs(c).astype(LD) * B).sum()
            print('adjoint %s slot %d: |lhs - rhs| = %.2e, tol %.2e' % (cid, d, float(abs(lhs - rhs)), float(tol)))
            assert abs(lhs - rhs) <= tol, (cid, d)
    finally:
        patch.close()

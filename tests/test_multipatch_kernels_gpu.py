"""Every kernel of pyiga_amd/csrc/multipatch.hip on the device against the host model: the cases of
tests/_multipatch_cases.py go through igx_multipatch_create with their hand-made maps, tests/_multipatch_model.py gives the
answer.  Index arithmetic, sorting and integer sums are exact, so is the summation order of injective maps: everything is
compared with array_equal, except the real-valued sums of non-injective maps (atomic adds in any order), which must lie within
the bound of recursive summation, ``gamma_{m-1} sum|a|`` plus the long double reference's own ``(m - 1) 2^-64 sum|a|``."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import _multipatch_cases as mc
import _multipatch_model as mm

pytestmark = pytest.mark.gpu

_I32P = C.POINTER(C.c_int32)
_patch_cache = {}


def _lib():
    from pyiga_amd import _lib
    return _lib


@pytest.fixture(scope='module', autouse=True)
def _close_patches():
    yield
    for pt in _patch_cache.values():
        pt.close()
    _patch_cache.clear()


def _patches(c):
    """One device patch per patch of the case (a handle of its own for every repetition of the same knot vectors)."""
    from pyiga_amd import geometry
    from pyiga_amd.assemblers import DevicePatch
    out, seen = [], {}
    for p, axes in enumerate(c.patches):
        k = seen[axes] = seen.get(axes, -1) + 1
        if (axes, k) not in _patch_cache:
            geo = geometry.unit_square() if len(axes) == 2 else geometry.unit_cube()
            _patch_cache[axes, k] = DevicePatch(c.kvs(p), geo)
        out.append(_patch_cache[axes, k])
    return out


def _create(pts, maps, nglobal):
    n = len(pts)
    handles = (C.c_void_p * n)(*[pt.handle for pt in pts])
    ptrs = (_I32P * n)(*[m.ctypes.data_as(_I32P) for m in maps])
    return _lib().load().igx_multipatch_create(pts[0].ctx.handle, n, handles, ptrs, C.c_int64(nglobal))


@contextlib.contextmanager
def _built(cid):
    """The multipatch handle of a case; freed on the way out, whatever the test does."""
    L = _lib()
    c = mc.case(cid)
    pts = _patches(c)
    h = _create(pts, c.l2g, c.nglobal)
    assert h, L.last_error()
    try:
        yield h, pts
    finally:
        L.load().igx_multipatch_destroy(h)


def _scatter_all(h, vals, bs):
    L = _lib()
    lib = L.load()
    L.check(lib.igx_multipatch_zero(h), 'igx_multipatch_zero')
    for p, (v, b) in enumerate(zip(vals, bs)):
        L.check(lib.igx_multipatch_scatter_host(h, p, L.dptr(v)), 'igx_multipatch_scatter_host')
        L.check(lib.igx_multipatch_scatter_vector(h, p, L.dptr(b)), 'igx_multipatch_scatter_vector')


def _download(h, M):
    L = _lib()
    vals, vec = np.full(M.nnz, np.nan), np.full(M.G, np.nan)
    L.check(L.load().igx_multipatch_download(h, L.dptr(vals), L.dptr(vec)), 'igx_multipatch_download')
    return vals, vec


def _assert_within_bound(dev, ld_m_sabs, what):
    ld, m, sabs = ld_m_sabs
    err = np.abs(dev.astype(np.longdouble) - ld)
    bound = mm.sum_bound(m, sabs)
    worst = int(np.argmax(err))
    print('%s: up to %d terms per position; largest error %.3e at a position of %d terms, bound there %.3e'
          % (what, int(m.max()), float(err[worst]), int(m[worst]), float(bound[worst])))
    bad = np.flatnonzero(err > bound)
    assert bad.size == 0, (what, bad[:5], err[bad[:5]], bound[bad[:5]])


@pytest.mark.parametrize('cid', mc.CASE_IDS)
def test_info_and_pattern(cid):
    L = _lib()
    lib = L.load()
    M = mc.model(cid)
    with _built(cid) as (h, _):
        info = L.MultipatchInfo()
        L.check(lib.igx_multipatch_get_info(h, C.byref(info)), 'igx_multipatch_get_info')
        got = dict(npatches=info.npatches, injective=info.injective, nrows=info.nrows, nnz=info.nnz,
                   entries=tuple(info.entries), zero_from=info.zero_from)
        assert got == M.info()
        indptr = np.full(M.G + 1, -1, dtype=np.int32)
        indices = np.full(M.nnz, -1, dtype=np.int32)
        L.check(lib.igx_multipatch_pattern(h, indptr.ctypes.data_as(_I32P), indices.ctypes.data_as(_I32P)), 'igx_multipatch_pattern')
        assert np.array_equal(indptr, M.indptr)
        assert np.array_equal(indices, M.indices)


@pytest.mark.parametrize('cid', mc.CASE_IDS)
def test_sums(cid):
    """Matrix values and load vectors.  Injective maps: the bits of the sum in patch order.  Non-injective maps: exact with
    integer values, within the summation bound with real ones."""
    M = mc.model(cid)
    with _built(cid) as (h, _):
        if M.injective:
            vals, bs = mc.values(cid, 'mat'), mc.values(cid, 'vec')
            _scatter_all(h, vals, bs)
            dv, db = _download(h, M)
            assert np.array_equal(dv, M.sum_values(vals))
            assert np.array_equal(db, M.sum_vector(bs))
        else:
            vals, bs = mc.values(cid, 'mat', integer=True), mc.values(cid, 'vec', integer=True)
            _scatter_all(h, vals, bs)
            dv, db = _download(h, M)
            assert np.array_equal(dv, M.sum_values(vals))
            assert np.array_equal(db, M.sum_vector(bs))
            vals, bs = mc.values(cid, 'mat'), mc.values(cid, 'vec')
            _scatter_all(h, vals, bs)
            dv, db = _download(h, M)
            _assert_within_bound(dv, M.sum_values_ld(vals), cid + ' values')
            _assert_within_bound(db, M.sum_vector_ld(bs), cid + ' vector')


@pytest.mark.parametrize('cid', mc.CASE_IDS)
def test_second_sum_has_no_residue_of_the_first(cid):
    """Large values, igx_multipatch_zero, other values: the model of the second values alone (integer values where the maps are
    not injective, so that the comparison is exact there too)."""
    M = mc.model(cid)
    integer = not M.injective
    with _built(cid) as (h, _):
        _scatter_all(h, mc.values(cid, 'mat', integer=integer, scale=1e6), mc.values(cid, 'vec', integer=integer, scale=1e6))
        vals, bs = mc.values(cid, 'mat', integer=integer), mc.values(cid, 'vec', integer=integer)
        _scatter_all(h, vals, bs)
        dv, db = _download(h, M)
        assert np.array_equal(dv, M.sum_values(vals))
        assert np.array_equal(db, M.sum_vector(bs))


@pytest.mark.parametrize('cid', ['permuted_2d_p4', 'p5_3d_two_cubes'])
def test_scatter_patch_equals_scatter_host(cid):
    """The values a patch holds on the device after an assembly, scattered from there, against the same values from the host."""
    L = _lib()
    lib = L.load()
    M = mc.model(cid)
    with _built(cid) as (h, pts):
        L.check(lib.igx_multipatch_zero(h), 'igx_multipatch_zero')
        vals = []
        for p, pt in enumerate(pts):
            vals.append(pt.assemble('mass', to_host=True))        # the values stay on the device as well
            L.check(lib.igx_multipatch_scatter_patch(h, p, pt.handle), 'igx_multipatch_scatter_patch')
        from_device, _ = _download(h, M)
        L.check(lib.igx_multipatch_zero(h), 'igx_multipatch_zero')
        for p, v in enumerate(vals):
            L.check(lib.igx_multipatch_scatter_host(h, p, L.dptr(v)), 'igx_multipatch_scatter_host')
        from_host, _ = _download(h, M)
        assert all(np.abs(v).min() > 0 for v in vals)
        assert np.array_equal(from_device, from_host)
        assert np.array_equal(from_device, M.sum_values(vals))


def test_values_d_equals_download():
    """The device-to-device copy into a caller's buffer of the same context (igx_dev_alloc, as MultipatchEigenSystem takes its
    mass values), pre-filled with NaN."""
    L = _lib()
    lib = L.load()
    cid = 'many_patches_middle'
    M = mc.model(cid)
    with _built(cid) as (h, pts):
        _scatter_all(h, mc.values(cid, 'mat'), mc.values(cid, 'vec'))
        ctx = pts[0].ctx.handle
        got = np.full(M.nnz, np.nan)
        d_buf = lib.igx_dev_alloc(ctx, got.nbytes)
        assert d_buf, L.last_error()
        try:
            L.check(lib.igx_dev_upload(ctx, d_buf, got.ctypes.data, got.nbytes), 'igx_dev_upload')
            L.check(lib.igx_multipatch_values_d(h, d_buf), 'igx_multipatch_values_d')
            L.check(lib.igx_dev_download(ctx, got.ctypes.data, d_buf, got.nbytes), 'igx_dev_download')
        finally:
            lib.igx_dev_free(ctx, d_buf)
        dv, _ = _download(h, M)
        assert np.array_equal(got, dv) and np.array_equal(dv, M.sum_values(mc.values(cid, 'mat')))


def test_refusals():
    L = _lib()
    lib = L.load()
    c = mc.case('scan_nglobal_%d' % mc.SCAN_TILE)
    pts = _patches(c)
    for bad, word in ((-1, '-1'), (c.nglobal, str(c.nglobal))):
        m = c.l2g[0].copy()
        m[7] = bad
        h = _create(pts, (m,), c.nglobal)
        try:
            assert not h
            assert 'outside' in L.last_error() and word in L.last_error()
        finally:
            if h:
                lib.igx_multipatch_destroy(h)
    h = _create(pts, c.l2g, 0)
    try:
        assert not h
        assert 'global dofs' in L.last_error()
    finally:
        if h:
            lib.igx_multipatch_destroy(h)
    with _built(c.id) as (h, _):
        v = np.zeros(pts[0].nnz)
        b = np.zeros(c.l2g[0].size)
        for p in (-1, 1):
            assert lib.igx_multipatch_scatter_host(h, p, L.dptr(v)) == L.IGX_ERR_ARG
            assert 'out of range' in L.last_error()
            assert lib.igx_multipatch_scatter_vector(h, p, L.dptr(b)) == L.IGX_ERR_ARG
            assert 'out of range' in L.last_error()
            assert lib.igx_multipatch_scatter_patch(h, p, pts[0].handle) == L.IGX_ERR_ARG
            assert 'out of range' in L.last_error()

"""k_face_add on the device (pyiga_amd/csrc/face_add.hip): for every case of tests/_robin_cases.py the
volume matrix is assembled on the device and downloaded, the faces are added with igx_patch_add_face (3D: the face patch's device
values) and igx_patch_add_face_host (2D and 3D), and the values are downloaded again.  The touched entries must equal
``before + r`` -- one IEEE addition, in term order where two faces meet -- and every other entry must be bit-identical; the
positions come from the numpy model tests/_robin_model.py.  The same identity on the global sums of a multipatch through
igx_multipatch_add_face[_host], and every documented error code by return value."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse

import _robin_cases as rc
import _robin_model as rm

pytestmark = pytest.mark.gpu


def _lib():
    from pyiga_amd import _lib
    return _lib


def _unit_geo(d):
    from pyiga_amd import geometry
    return geometry.unit_square() if d == 2 else geometry.unit_cube()


def _device_values(patch):
    """The values the patch holds on the device, through a one-patch multipatch with the identity map (its scatter is a copy)."""
    L = _lib()
    lib = L.load()
    n = patch.shape[0]
    l2g = np.arange(n, dtype=np.int32)
    handles = (C.c_void_p * 1)(patch.handle)
    ptrs = (C.POINTER(C.c_int32) * 1)(l2g.ctypes.data_as(C.POINTER(C.c_int32)))
    h = lib.igx_multipatch_create(patch.ctx.handle, 1, handles, ptrs, n)
    assert h, L.last_error()
    try:
        L.check(lib.igx_multipatch_zero(h), 'igx_multipatch_zero')
        L.check(lib.igx_multipatch_scatter_patch(h, 0, patch.handle), 'igx_multipatch_scatter_patch')
        out = np.empty(patch.nnz)
        L.check(lib.igx_multipatch_download(h, L.dptr(out), None), 'igx_multipatch_download')
    finally:
        lib.igx_multipatch_destroy(h)
    return out


def _face_patch(vol, kvs, axis):
    from pyiga_amd.assemblers import DevicePatch
    from pyiga_amd.form_assemblers import _identity_geo
    tkvs = rm.face_kvs(kvs, axis)
    return DevicePatch(tkvs, _identity_geo(tkvs), nqp=vol.nqp)


@pytest.mark.parametrize('name', sorted(rc.KERNEL_CASES))
def test_face_add_is_one_addition_per_touched_entry(name):
    from pyiga_amd.assemblers import DevicePatch
    kvs = rc.kernel_kvs(name)
    d = len(kvs)
    vol = DevicePatch(kvs, _unit_geo(d))
    rng = np.random.default_rng(len(name))
    try:
        indptr, indices = vol.pattern()
        mptr, mind = rm.canonical_pattern(kvs)
        assert np.array_equal(indptr, mptr) and np.array_equal(indices, mind)     # the model's canonical order is the library's
        # host values, every side in turn: where two faces meet (edges, corners) the sum is in the order of the calls
        before = vol.assemble('stiffness', to_host=True)
        assert np.array_equal(_device_values(vol), before)
        want = before.copy()
        touched = np.zeros(before.size, dtype=bool)
        for axis, side in rc.sides(d):
            r = rng.standard_normal(rm.face_nnz(kvs, axis))
            vol.add_face(axis, side, r)
            rm.add_face(want, kvs, axis, side, r)
            touched[rm.face_positions(kvs, axis, side)] = True
        after = _device_values(vol)
        assert np.array_equal(after[~touched], before[~touched])                  # bit-identical everywhere else
        assert np.array_equal(after, want), np.abs(after - want).max()
        assert touched.sum() < before.size
        if d == 3:
            # device values of the 2D face patch: its mass matrix on side 0, its stiffness matrix on side 1 of every axis
            before = vol.assemble('mass', to_host=True)
            want = before.copy()
            for axis, side in rc.sides(d):
                face = _face_patch(vol, kvs, axis)
                try:
                    r = face.assemble('stiffness' if side else 'mass', to_host=True)
                    assert r.size == rm.face_nnz(kvs, axis)
                    vol.add_face(axis, side, face)
                finally:
                    face.close()
                rm.add_face(want, kvs, axis, side, r)
            after = _device_values(vol)
            assert np.array_equal(after[~touched], before[~touched])
            assert np.array_equal(after, want), np.abs(after - want).max()
    finally:
        vol.close()


def _global_positions(MP, p, axis, side):
    """Positions among the global values of the entries of the face matrix of side (axis, side) of patch p, in face order."""
    kvs = tuple(MP.patches[p][0])
    lptr, lind = rm.canonical_pattern(kvs)
    pos = rm.face_positions(kvs, axis, side)
    I = np.searchsorted(lptr, pos, side='right') - 1
    J = lind[pos]
    l2g = np.asarray(MP.patch_to_global_idx(p))
    gptr, gind = MP.pattern()
    look = scipy.sparse.csr_matrix((np.arange(1, gind.size + 1, dtype=np.float64), gind, gptr), shape=(MP.numdofs,) * 2)
    g = np.asarray(look[l2g[I], l2g[J]]).ravel().astype(np.int64) - 1
    assert g.min() >= 0
    return g


def _mp_values(MP, h):
    L = _lib()
    out = np.empty(MP.pattern()[1].size)
    L.check(L.load().igx_multipatch_download(h, L.dptr(out), None), 'igx_multipatch_download')
    return out


def test_multipatch_face_add_lshape():
    """The L-shape: every side of every patch, among them 'bottom' of patch 0, whose corner dof is shared with patch 1, and the
    joined sides themselves (rows that are sums of two patches: reached through the position array)."""
    L = _lib()
    lib = L.load()
    MP = rc.lshape()
    try:
        MP.assemble_system('inner(grad(u),grad(v))*dx', None)
        h = MP._device()
        before = _mp_values(MP, h)
        want = before.copy()
        rng = np.random.default_rng(7)
        for p in range(MP.numpatches):
            kvs = tuple(MP.patches[p][0])
            for axis, side in rc.sides(2):
                r = rng.standard_normal(rm.face_nnz(kvs, axis))
                L.check(lib.igx_multipatch_add_face_host(h, p, axis, side, L.dptr(r), r.size), 'igx_multipatch_add_face_host')
                g = _global_positions(MP, p, axis, side)
                assert np.unique(g).size == g.size
                want[g] = want[g] + r
        after = _mp_values(MP, h)
        assert np.array_equal(after, want), np.abs(after - want).max()
        assert (after == before).sum() > 0
    finally:
        MP.close()


def test_multipatch_face_add_device_faces_3d():
    import _solver_cases as sc
    from pyiga_amd.assemblers import DevicePatch
    from pyiga_amd.form_assemblers import _identity_geo
    L = _lib()
    lib = L.load()
    MP = sc.two_cubes(2, 3)
    try:
        MP.assemble_system('inner(grad(u),grad(v))*dx', None)
        h = MP._device()
        before = _mp_values(MP, h)
        want = before.copy()
        for p in range(2):
            kvs = tuple(MP.patches[p][0])
            for axis, side in rc.sides(3):
                tkvs = rm.face_kvs(kvs, axis)
                face = DevicePatch(tkvs, _identity_geo(tkvs), nqp=3)
                try:
                    r = face.assemble('mass' if side else 'stiffness', to_host=True)
                    L.check(lib.igx_multipatch_add_face(h, p, axis, side, face.handle), 'igx_multipatch_add_face')
                finally:
                    face.close()
                g = _global_positions(MP, p, axis, side)
                want[g] = want[g] + r
        after = _mp_values(MP, h)
        assert np.array_equal(after, want), np.abs(after - want).max()
    finally:
        MP.close()


def test_multipatch_face_add_non_injective_join():
    """Two dofs of patch 0 end up in one global dof (the join of tests/test_multipatch_gpu.py): the adds are atomic.  A face that
    holds one of the two dofs still has distinct positions (exact); the face that holds both sums up to four face entries into
    one position in no fixed order, so it is compared within four roundings of the largest value."""
    from pyiga_amd import assemble, bspline, geometry
    L = _lib()
    lib = L.load()
    kvs = 2 * (bspline.make_knots(2, 0.0, 1.0, 4),)
    MP = assemble.Multipatch([(kvs, geometry.unit_square()), (kvs, geometry.unit_square().translate((1, 0)))])
    a, bb, c = 5, 12, 23
    MP.join_dofs(0, [a], 1, [bb])
    MP.join_dofs(1, [bb], 0, [c])
    MP.finalize()
    assert not MP.injective
    try:
        MP.assemble_system('inner(grad(u),grad(v))*dx', None)
        h = MP._device()
        before = _mp_values(MP, h)
        rng = np.random.default_rng(11)
        r = rng.standard_normal(rm.face_nnz(kvs, 0))
        L.check(lib.igx_multipatch_add_face_host(h, 0, 0, 0, L.dptr(r), r.size), 'igx_multipatch_add_face_host')     # 'bottom': dof 5 only
        g = _global_positions(MP, 0, 0, 0)
        assert np.unique(g).size == g.size
        want = before.copy()
        want[g] = want[g] + r
        mid = _mp_values(MP, h)
        assert np.array_equal(mid, want)
        r2 = rng.standard_normal(rm.face_nnz(kvs, 1))
        L.check(lib.igx_multipatch_add_face_host(h, 0, 1, 1, L.dptr(r2), r2.size), 'igx_multipatch_add_face_host')   # 'right': dofs 5 and 23
        g2 = _global_positions(MP, 0, 1, 1)
        assert np.unique(g2).size < g2.size
        np.add.at(want, g2, r2)
        after = _mp_values(MP, h)
        assert np.abs(after - want).max() <= 4 * np.finfo(float).eps * max(np.abs(want).max(), np.abs(r2).max())
        untouched = np.ones(before.size, dtype=bool)
        untouched[g] = False
        untouched[g2] = False
        assert np.array_equal(after[untouched], before[untouched])
    finally:
        MP.close()


def test_error_codes():
    """Every documented refusal, by return value only."""
    from pyiga_amd import bspline
    from pyiga_amd.assemblers import DevicePatch
    from pyiga_amd.form_assemblers import _identity_geo
    L = _lib()
    lib = L.load()
    kv2, kv3 = bspline.make_knots(2, 0.0, 1.0, 3), bspline.make_knots(3, 0.0, 1.0, 3)
    kvs = (kv2, kv2, kv3)
    vol = DevicePatch(kvs, _unit_geo(3))
    face_ok = DevicePatch((kv2, kv3), _identity_geo((kv2, kv3)), nqp=vol.nqp)          # the face of axis 0 and of axis 1
    face_bad = DevicePatch((kv2, kv2), _identity_geo((kv2, kv2)), nqp=vol.nqp)         # the face of axis 2 only
    slab = DevicePatch(kvs, _unit_geo(3), row0=(0, 2))
    vol2 = DevicePatch((kv2, kv3), _unit_geo(2))
    MP = rc.lshape()
    try:
        r = np.ones(rm.face_nnz(kvs, 0))
        # no values yet
        assert lib.igx_patch_add_face_host(vol.handle, 0, 0, L.dptr(r), r.size) == L.IGX_ERR_ARG
        assert lib.igx_patch_add_face(vol.handle, 0, 0, face_ok.handle) == L.IGX_ERR_ARG
        vol.assemble('mass', to_host=False)
        before = _device_values(vol)
        # a face patch without values
        assert lib.igx_patch_add_face(vol.handle, 0, 0, face_ok.handle) == L.IGX_ERR_ARG
        face_ok.assemble('mass', to_host=False)
        face_bad.assemble('mass', to_host=False)
        # axis / side out of range
        for axis, side in ((-1, 0), (3, 0), (0, 2), (0, -1)):
            assert lib.igx_patch_add_face_host(vol.handle, axis, side, L.dptr(r), r.size) == L.IGX_ERR_ARG
            assert lib.igx_patch_add_face(vol.handle, axis, side, face_ok.handle) == L.IGX_ERR_ARG
        # wrong number of values; a face of other degrees / dof counts; a face of the wrong dimension
        assert lib.igx_patch_add_face_host(vol.handle, 0, 0, L.dptr(r), r.size - 1) == L.IGX_ERR_ARG
        assert lib.igx_patch_add_face(vol.handle, 2, 0, face_ok.handle) == L.IGX_ERR_ARG
        assert lib.igx_patch_add_face(vol.handle, 0, 1, face_bad.handle) == L.IGX_ERR_ARG
        assert lib.igx_patch_add_face(vol.handle, 0, 0, vol.handle) == L.IGX_ERR_ARG
        vol2.assemble('mass', to_host=False)
        assert lib.igx_patch_add_face(vol2.handle, 0, 0, face_ok.handle) == L.IGX_ERR_ARG      # 1D faces: the _host variant
        # a row slab
        slab.assemble('mass', to_host=False)
        assert lib.igx_patch_add_face_host(slab.handle, 0, 0, L.dptr(r), r.size) == L.IGX_ERR_UNSUPPORTED
        assert lib.igx_patch_add_face(slab.handle, 0, 0, face_ok.handle) == L.IGX_ERR_UNSUPPORTED
        # nothing was added by any refused call, and the accepted ones keep the kind of the values
        assert np.array_equal(_device_values(vol), before)
        assert lib.igx_patch_add_face(vol.handle, 0, 1, face_ok.handle) == 0
        assert lib.igx_patch_add_face(vol.handle, 2, 0, face_bad.handle) == 0
        h = C.c_void_p()
        fixed = np.zeros(0, dtype=np.int64)
        assert lib.igx_solver_create(vol.handle, L.KINDS['mass'], fixed.ctypes.data_as(C.POINTER(C.c_int64)), 0, C.byref(h)) == 0
        lib.igx_solver_destroy(h)
        # multipatch: before the patch's scatter of the current sum, out of range
        hm = MP._device()
        kvm = tuple(MP.patches[0][0])
        rm_ = np.ones(rm.face_nnz(kvm, 0))
        L.check(lib.igx_multipatch_zero(hm), 'igx_multipatch_zero')
        assert lib.igx_multipatch_add_face_host(hm, 0, 0, 0, L.dptr(rm_), rm_.size) == L.IGX_ERR_ARG
        MP.assemble_system('u*v*dx', None)
        assert lib.igx_multipatch_add_face_host(hm, 3, 0, 0, L.dptr(rm_), rm_.size) == L.IGX_ERR_ARG
        assert lib.igx_multipatch_add_face_host(hm, 0, 2, 0, L.dptr(rm_), rm_.size) == L.IGX_ERR_ARG
        assert lib.igx_multipatch_add_face_host(hm, 0, 0, 0, L.dptr(rm_), rm_.size + 1) == L.IGX_ERR_ARG
        assert lib.igx_multipatch_add_face(hm, 0, 0, 0, face_ok.handle) == L.IGX_ERR_ARG               # a 2D face for a 2D patch
        assert lib.igx_multipatch_add_face_host(hm, 0, 0, 0, L.dptr(rm_), rm_.size) == 0
        L.check(lib.igx_multipatch_zero(hm), 'igx_multipatch_zero')
        assert lib.igx_multipatch_add_face_host(hm, 0, 0, 0, L.dptr(rm_), rm_.size) == L.IGX_ERR_ARG   # the sums were restarted
    finally:
        for pch in (vol, face_ok, face_bad, slab, vol2):
            pch.close()
        MP.close()

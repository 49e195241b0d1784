"""Every instantiation of the first fused stage k_bf2 and of the mirror passes k_mirror / k_mirror2 (pyiga_amd/csrc/fused.hip)
against the CPU oracle, at the sizes where their tiles, chunks, row splits and row slabs change.  k_bf3 is the default for the
forms these kernels serve, so the cases ask for them with IGX_BF=2 (in 2D: with IGX_PATH=fused); production reaches them for
3D patches beyond the offsets of k_bf3 and for non-symmetric 2D forms under IGX_PATH=fused.  The cases and the restatement of the
dispatch are in tests/_bf2_cases.py; tests/test_bf2_coverage_cpu.py ties them to the source and to the library's launch
arithmetic.  Needs a real MI355X:  pytest -m gpu.

Tolerance: max|A - A_ref| <= 1e-12 * max|A_ref| (RTOL of test_gpu_parity.py); against k_bf3 in 3D the
relation test_both_triangles_from_the_fused_stage states: stiffness bit for bit, mass within 1e-14 of the maximum.
"""
import numpy as np
import pytest
import scipy.sparse

from conftest import rel_maxdiff
from test_gpu_parity import RTOL, _bf3_check_vs_oracle, _bf3_coeff, _bf3_patch_kvs, _geo
import _bf2_cases as b2
import _bf3_cases as bc

pytestmark = pytest.mark.gpu

KNOB_NAMES = ('IGX_PATH', 'IGX_BF', 'IGX_GEOA', 'IGX_FINAL')
OTHER_CHAINS = {'bf3', 'both', 'twin', 'single', 'kron'}


@pytest.fixture(scope='module')
def iga():
    import pyiga_amd
    pyiga_amd._lib.context()          # raises if no GPU / library: there is no fallback
    return pyiga_amd


def _set_knobs(monkeypatch, knobs):
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')
    for name in KNOB_NAMES:
        if name in knobs:
            monkeypatch.setenv(name, knobs[name])
        else:
            monkeypatch.delenv(name, raising=False)


def _fn(expr):
    return lambda x, y: eval(expr, {'__builtins__': {}}, dict(x=x, y=y)) + 0.0 * x


def _pform_terms(patch, pterms):
    """(mask_v, mask_u, coefficient on the Gauss grid) of the na = 2 form: on the unit square the parameters are the physical
    point, x along the last grid axis."""
    y, x = patch.gauss(0)[0][:, None], patch.gauss(1)[0][None, :]
    split = _fn(b2.NA2_SPLIT)(x, y)
    out = []
    for r, s, half in pterms:
        c = _fn(b2.NA2_TABLE[r][s])(x, y)
        if (r, s) in b2.NA2_TWICE:
            c = c * split if half == 0 else c * (1.0 - split)
        out.append((b2.JET_MASK[r], b2.JET_MASK[s], c))
    return out


def _assemble(iga, case, algo, row0=None):
    """(CSR matrix, last_path) of the patch of a case or of a row slab; the knobs are read from the environment when the patch
    is created."""
    if case.kind == 'convdiff':
        asm = iga.assemblers.ConvDiffAssembler3D(_bf3_patch_kvs(iga, case.axes), _geo(iga, case.geo), _bf3_coeff, row0=row0)
        A = asm.assemble_csr(algo=algo)
        path = asm.patch.last_path()
        asm.patch.close()
        return A, path
    patch = iga.assemblers.DevicePatch(_bf3_patch_kvs(iga, case.axes), _geo(iga, case.geo), row0=row0)
    if case.kind == 'pform':
        patch.set_pform(_pform_terms(patch, case.pterms))
    A = patch.csr('form' if case.kind == 'pform' else case.kind, algo=algo)
    path = patch.last_path()
    patch.close()
    return A, path


def _oracle(case):
    from oracle import iga_oracle as orc
    okvs = tuple(orc.KnotVector(bc.axis_knots(a), a[0]) for a in case.axes)
    if case.kind == 'pform':
        table = [[_fn(b2.NA2_TABLE[r][s]) if max(r, s) < 3 else None for s in range(4)] for r in range(4)]
        return orc.assemble_nonsymmetric('form', okvs, orc.geo_unit_cube(2), table=table, nthreads=8)
    if case.kind == 'convdiff':
        return orc.assemble_nonsymmetric('convdiff', okvs, getattr(orc, 'geo_' + case.geo)(), coeff=_bf3_coeff, nthreads=8)
    return orc.assemble(case.kind, okvs, getattr(orc, 'geo_' + case.geo)(), nthreads=8)


def _check_path(path, route, tag):
    """Exactly the chain restated: k_bf2 ('fused' without 'bf3' / 'both'), the mirror pass for the symmetric kinds, k_geoA where
    restated, nothing else."""
    want = {'fused'} | ({'mirror'} if route.mirror else set()) | ({'geoA'} if route.geoA else set())
    assert not (path & OTHER_CHAINS), (tag, sorted(path))
    assert path == want, (tag, sorted(path), sorted(want))


def _route(case):
    route = b2.bf2_route(case.axes, case.kind, case.knobs, [(b2.JET_MASK[r], b2.JET_MASK[s]) for r, s, _ in case.pterms] if case.pterms else None)
    assert route is not None and route.key == case.key and route.mirror == case.mirror, (case.id, route)
    return route


def _same(A, B):
    return np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices) and np.array_equal(A.data, B.data)


def _check_vs_bf3(iga, case, A, monkeypatch, tag):
    """3D: the default chain (k_bf3) forms the same element matrices: stiffness bit for bit, mass (per-axis symmetry in k_bf3)
    within 1e-14 of the maximum."""
    _set_knobs(monkeypatch, {})
    B, bpath = _assemble(iga, case, 'sumfact')
    assert 'bf3' in bpath and 'mirror' not in bpath, (tag, sorted(bpath))
    assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices), tag
    if case.kind == 'stiffness':
        assert np.array_equal(A.data, B.data), (tag, np.abs(A.data - B.data).max())
    else:
        assert np.abs(A.data - B.data).max() <= 1e-14 * np.abs(B.data).max(), (tag, np.abs(A.data - B.data).max() / np.abs(B.data).max())


def _check(iga, case, monkeypatch):
    route = _route(case)
    sym = case.mirror is not None
    _set_knobs(monkeypatch, case.knobs)
    A, path = _assemble(iga, case, 'sumfact')
    tag = (case.id, tuple(case.key), sorted(path))
    _check_path(path, route, tag)
    kvs = _bf3_patch_kvs(iga, case.axes)
    _bf3_check_vs_oracle(A, _oracle(case), kvs, case.kind, tag, symmetric=sym)
    E, _ = _assemble(iga, case, 'entrywise')
    assert np.array_equal(A.indptr, E.indptr) and np.array_equal(A.indices, E.indices), tag
    assert rel_maxdiff(A, E) <= RTOL, (tag, rel_maxdiff(A, E))
    if len(case.axes) == 3 and sym:
        _check_vs_bf3(iga, case, A, monkeypatch, tag)
    return A, route


_EDGE = b2.EDGE_CASES + b2.MIRROR_CASES


@pytest.mark.parametrize('case', _EDGE, ids=[c.id for c in _EDGE])
def test_every_bf2_and_mirror_instantiation_vs_oracle(iga, case, monkeypatch):
    """Every k_bf2 instantiation a patch can reach -- mass and stiffness in 2D and 3D, the 2D parametric jet form with two
    arrays in a slot and the 3D convection-diffusion form (non-symmetric: all outer pairs, no mirror pass), for P = 2 .. 6 --
    with one span, 2 p, RMAX, RMAX + 1 and 2 RMAX + 1 dofs on the last axis and a swept axis of one span or cut into chunks; every mirror instantiation with RCM and RCM + 1 dofs on the last axis, its rows split over
    blocks, k_mirror2 with whole and with ragged groups of rows.  The chain ran as restated (not k_bf3, not the stage kernels),
    every value written, exact symmetry for the symmetric kinds, the structural pattern and the values of the CPU oracle (the
    reference's loop nest), the entry-wise kernels, and in 3D the relation to k_bf3."""
    _check(iga, case, monkeypatch)


def test_tail_split_of_the_chunk_plan(iga, monkeypatch):
    """bf2_choose_chunks with more blocks than the chip holds: whole blocks for the full rounds, the rest of the blocks in
    tail_k chunks of the swept axis (decoded by bid >= main_blocks, the last chunk clipped).  The shape gets a tail split for
    one to six resident blocks per CU on 256 CUs (test_bf2_coverage_cpu.py), hence the check of the CU count.  Against the
    oracle (9.6 million nonzeros at p = 1: three seconds), the entry-wise kernels and k_bf3."""
    import subprocess
    import sys
    # (torch in a child process: this one has initialised the library's HIP runtime, beside which torch's finds no device)
    out = subprocess.run([sys.executable, '-c', 'import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)'],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    ncu = int(out.stdout.split()[-1])
    if ncu != b2.NCU:
        pytest.skip('the tail-split shape is worked out for %d CUs, this device has %d' % (b2.NCU, ncu))
    case = b2.TAIL_CASE
    _check(iga, case, monkeypatch)


@pytest.mark.parametrize('case', b2.SLAB_CASES, ids=[c.id for c in b2.SLAB_CASES])
def test_row_slabs_through_bf2_and_mirror(iga, case, monkeypatch):
    """Row slabs: in 3D of axis 0 (the outer pairs; cut at 0, 1, N0 // 2, N0), in 2D of the swept axis itself (mid_lo, mid_hi =
    r0_hi + p for the mirror sources, gmid_lo; cut at 0, 1, p, N0 // 2, N0 - 1, N0) on a patch that is cut into chunks and two
    tiles.  The whole patch against the oracle like every case; every slab takes the same path; the stacked slabs are the whole
    patch bit for bit (the invariant of every chain)."""
    A, route = _check(iga, case, monkeypatch)
    _set_knobs(monkeypatch, case.knobs)
    parts = []
    for lo, hi in zip(case.slabs[:-1], case.slabs[1:]):
        S, spath = _assemble(iga, case, 'sumfact', row0=(lo, hi))
        _check_path(spath, route, (case.id, lo, hi))
        assert not np.isnan(S.data).any(), (case.id, lo, hi)
        parts.append(S)
    V = scipy.sparse.vstack(parts).tocsr()
    assert _same(V, A), (case.id, 'slabs')

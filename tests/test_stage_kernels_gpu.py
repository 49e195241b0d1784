"""Every instantiation of the stage chain of the global sum factorisation -- k_stageA, k_stageB, k_combine, k_final, k_final_q,
k_final_mfma (pyiga_amd/csrc/sumfact.hip, sumfact_stages.h, sumfact_hi.hip) -- against the CPU oracle, and the sizes at which
their launch arithmetic changes.  The cases and the restatement of the dispatch are in tests/_stage_cases.py;
tests/test_stage_coverage_cpu.py ties them to the sources.  Needs a real MI355X:  pytest -m gpu.

Tolerance: max|A - A_ref| <= 1e-12 * max|A_ref| (RTOL of test_gpu_parity.py).
"""
import numpy as np
import pytest
import scipy.sparse

from conftest import rel_maxdiff
from test_gpu_parity import RTOL, _bf3_check_vs_oracle, _bf3_patch_kvs, _geo
import _bf3_cases as bc
import _stage_cases as st

pytestmark = pytest.mark.gpu

OTHER_CHAINS = {'fused', 'bf3', 'single', 'twin', 'mirror', 'kron'}


@pytest.fixture(scope='module')
def iga():
    import pyiga_amd
    pyiga_amd._lib.context()          # raises if no GPU / library: there is no fallback
    return pyiga_amd


def _coeff(x, y, z):
    return 1.0 + x * x + 0.5 * z


def _table(table, dim):
    """The 4 x 4 table of expressions; a 2D patch has no d/dz."""
    T = st.TABLES[table]
    return T if dim == 3 else [[e if max(r, s) < 3 else None for s, e in enumerate(row)] for r, row in enumerate(T)]


def oracle_matrix(axes, geo, kind, table):
    from oracle import iga_oracle as orc
    okvs = tuple(orc.KnotVector(bc.axis_knots(a), a[0]) for a in axes)
    ogeo = getattr(orc, 'geo_' + geo)()
    if kind == 'convdiff':
        return orc.assemble_nonsymmetric('convdiff', okvs, ogeo, coeff=_coeff, nthreads=8)
    if kind == 'form':
        return orc.assemble_nonsymmetric('form', okvs, ogeo, table=st.table_oracle(_table(table, len(axes)), len(axes)), nthreads=8)
    return orc.assemble(kind, okvs, ogeo, nthreads=8)


def _assemble(iga, axes, geo, kind, table, algo, row0=None):
    """(CSR matrix, last_path) of one patch or row slab; the knobs are read from the environment when the patch is created."""
    kvs = _bf3_patch_kvs(iga, axes)
    g = _geo(iga, geo)
    if kind == 'convdiff':
        asm = iga.assemblers.ConvDiffAssembler3D(kvs, g, _coeff, row0=row0)
        A = asm.assemble_csr(algo=algo)
        path = asm.patch.last_path()
        asm.patch.close()
        return A, path
    patch = iga.assemblers.DevicePatch(kvs, g, row0=row0)
    if kind == 'form':
        patch.set_form_expr(_table(table, len(axes)))
    A = patch.csr(kind, algo=algo)
    path = patch.last_path()
    patch.close()
    return A, path


def _set_knobs(monkeypatch, knobs):
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')
    for name in ('IGX_PATH', 'IGX_GEOA', 'IGX_FINAL'):
        if name in knobs:
            monkeypatch.setenv(name, knobs[name])
        else:
            monkeypatch.delenv(name, raising=False)


def _check_path(path, keys, tag):
    assert keys is not None, tag
    assert not (path & OTHER_CHAINS), (tag, sorted(path))
    assert ('geoA' in path) == (keys.stageA == 'geoA'), (tag, sorted(path))


def _check(iga, axes, geo, kind, table, knobs, tag, entrywise=True):
    """The stage chain ran as restated; every value written, exact symmetry for the symmetric kinds, the pattern and the values
    of the oracle, the values of the entry-wise kernels.  Returns the matrix and the keys."""
    keys = st.stage_keys(axes, kind, knobs, table, geo)
    A, path = _assemble(iga, axes, geo, kind, table, 'sumfact')
    tag = (tag, keys.stageA, keys.stageB, keys.nterm, keys.final)
    _check_path(path, keys, tag)
    R = oracle_matrix(axes, geo, kind, table)
    _bf3_check_vs_oracle(A, R, _bf3_patch_kvs(iga, axes), kind, tag, symmetric=kind in ('mass', 'stiffness'))
    if entrywise:
        E, _ = _assemble(iga, axes, geo, kind, table, 'entrywise')
        assert rel_maxdiff(A, E) <= RTOL, (tag, rel_maxdiff(A, E))
    return A, keys


@pytest.mark.parametrize('case', st.STAGE_CASES, ids=[c.id for c in st.STAGE_CASES])
def test_every_stage_instantiation_vs_oracle(iga, case, monkeypatch):
    """One patch per reachable instantiation of k_stageA, k_stageB (every NTERM at a compile-time and a run-time q), k_final,
    k_final_q and k_final_mfma, and k_combine: the chain ran as the restatement says (no fused stage, no twin, no single
    launch; k_geoA exactly where restated), every value written, exact symmetry for mass and stiffness, the structural pattern
    and the values of the CPU oracle, the entry-wise kernels, and -- one case per final-kernel family and stage-A variant --
    row slabs of axis 0 cut at 0, 1, N0 // 2, N0 stacked equal the whole patch bit for bit."""
    _set_knobs(monkeypatch, case.knobs)
    A, keys = _check(iga, case.axes, case.geo, case.kind, case.table, case.knobs, case.id)
    for want, got in ((case.stageA, keys.stageA), (case.stageB, keys.stageB), (case.final, keys.final)):
        assert want is None or want == got, (case.id, want, got)
    if not case.slabs:
        return
    N0 = bc.numdofs(case.axes[0])
    cuts = sorted(set([0, 1, N0 // 2, N0]))
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        S, spath = _assemble(iga, case.axes, case.geo, case.kind, case.table, 'sumfact', row0=(lo, hi))
        _check_path(spath, keys, (case.id, lo, hi))
        parts.append(S)
    V = scipy.sparse.vstack(parts).tocsr()
    assert np.array_equal(V.indptr, A.indptr) and np.array_equal(V.indices, A.indices) and np.array_equal(V.data, A.data), (case.id, 'slabs')


_ROW_PARAMS = [(s, h) for s in st.FINAL_ROW_SWEEPS for h in (0, 1)]


@pytest.mark.parametrize('sweep,half', _ROW_PARAMS, ids=['%s-%s' % (s[0], ('low', 'high')[h]) for s, h in _ROW_PARAMS])
def test_final_rows_per_wave_task(iga, sweep, half, monkeypatch):
    """k_final gives a wave CR <= crmax = min(64, 512 / q - p) consecutive rows: the last axis runs over crmax - 1 .. 2 crmax + 2
    dofs (in two halves) -- one, two and three chunks, every position of the last chunk's edge -- at the fast and at the generic
    instantiation (double knots on the mid and the last axis), against the oracle at every size."""
    name, fn, crmax = sweep
    kernels = set()
    for N in st.final_row_sizes(crmax, half):
        axes, kind, knobs, table = fn(N)
        _set_knobs(monkeypatch, knobs)
        _, keys = _check(iga, axes, st.GEOS_3D[0] if len(axes) == 3 else st.GEOS_2D[0], kind, table, knobs, (name, N), entrywise=False)
        kernels.add(keys.final)
    assert len(kernels) == 1 and next(iter(kernels)).kernel == 'k_final'


def test_final_row_tiles(iga, monkeypatch):
    """k_final cuts the rows of the last axis into tiles once a tile's basis segment passes 64 KiB of LDS: the first sizes with
    two and with three tiles and one span either side of each, against the oracle."""
    name, fn = st.FINAL_TILE_SWEEP
    tiles = []
    for n1 in st.final_tile_sizes():
        axes, kind, knobs, table = fn(n1)
        _set_knobs(monkeypatch, knobs)
        _, keys = _check(iga, axes, 'bspline_quarter_annulus', kind, table, knobs, (name, n1), entrywise=False)
        tiles.append(keys.shape['ntiles'])
    assert sorted(set(tiles)) == [1, 2, 3]


@pytest.mark.parametrize('sweep', st.FINALQ_SWEEPS, ids=[s[0] for s in st.FINALQ_SWEEPS])
def test_finalq_row_chunks(iga, sweep, monkeypatch):
    """A wave of k_final_q owns R = 64 / P rows: the last axis runs over R - 1 .. 2 R + 1 dofs (one, two and three chunks, every
    number of rows in the last one) at P = 2, 3 (64 is no multiple of it) and 6, against the oracle."""
    name, P, fn = sweep
    for N in st.finalq_sizes(P):
        axes, kind, knobs, table = fn(N)
        _set_knobs(monkeypatch, knobs)
        _, keys = _check(iga, axes, st.GEOS_3D[0] if len(axes) == 3 else st.GEOS_2D[0], kind, table, knobs, (name, N), entrywise=False)
        assert keys.final.kernel == 'k_final_q' and keys.final.args[0] == P


@pytest.mark.parametrize('case', st.FINALQ_LPW_CASES, ids=[c[0] for c in st.FINALQ_LPW_CASES])
def test_finalq_lines_per_block(iga, case, monkeypatch):
    """The lines per block of k_final_q: a launch of less than one resident round (2D) and one of several rounds (3D)."""
    name, axes, kind, knobs, per_super = case
    _set_knobs(monkeypatch, knobs)
    _, keys = _check(iga, axes, st.GEOS_3D[1] if len(axes) == 3 else st.GEOS_2D[1], kind, None, knobs, name)
    assert keys.final.kernel == 'k_final_q' and keys.shape['q_per_super'] == per_super


@pytest.mark.parametrize('sweep', st.CHUNK_SWEEPS, ids=[s[0] for s in st.CHUNK_SWEEPS])
def test_sweep_chunks(iga, sweep, monkeypatch):
    """k_stageA and k_stageB cut a sweep with few blocks into chunks that re-walk P - 1 warm-up spans: the swept axis runs over
    8 P - 1 .. 8 P + 2 spans and 12 P (in 2D, stage A: 2 P - 1 .. 2 P + 2 and 3 P) -- one, two and three chunks -- with single and
    with double knots, symmetric and non-symmetric forms, against the oracle and the entry-wise kernels."""
    name, which, fn, P, factor = sweep
    seen = set()
    for n in st.chunk_sweep_sizes(P, factor):
        axes, kind, knobs, table = fn(n)
        _set_knobs(monkeypatch, knobs)
        _, keys = _check(iga, axes, st.GEOS_3D[n % 2] if len(axes) == 3 else st.GEOS_2D[n % 2], kind, table, knobs, (name, n))
        assert keys.stageA != 'geoA' or which == 'chunksB'
        seen.add(keys.shape[which][0])
    assert seen == {1, 2, 3}

"""The pair window of k_geoA's pair-product sweep (geoa.hip): on an axis 0 whose interior knots are single it stays in place and
the register names rotate -- one phase per leaving function, a copy of a plane's code per phase; on an axis with repeated knots
the window moves as before.  `IGX_NO_GEOA_ROT=1` (read when a patch is created) takes the moving form everywhere.  Both forms
form the same products and add them in the same order: the matrix must be the same BITS, and equal the long-double contraction
of the CPU oracle and the entry-wise kernels within the bound of tests/test_gpu_parity.py.  Needs a real MI355X:  pytest -m gpu.

Shapes: the smallest at which the rotation can go wrong -- 2 x 2 spans on the other axes; axis 0 with 2P + 1 .. 2P + 3 spans
(every phase twice and the wrap), span ends on, before and behind the boundary of a batch of eight planes, one span, repeated
knots, row slabs that begin at every phase.
"""
import numpy as np
import pytest
import scipy.sparse

from conftest import rel_maxdiff

pytestmark = pytest.mark.gpu

RTOL = 1e-12            # sum-factorised against the oracle and against entry-wise: the bound of tests/test_gpu_parity.py
KNOB = 'IGX_NO_GEOA_ROT'
NS = 8                  # planes of a batch (geoa.hip)
BF3 = {'geoA', 'fused', 'both', 'bf3'}


@pytest.fixture(scope='module')
def iga():
    import pyiga_amd
    pyiga_amd._lib.context()          # raises if no GPU / library: there is no fallback
    return pyiga_amd


GEOS = {'cylinder': ('geo_cylinder', lambda g: g.tensor_product(g.line_segment(0.0, 1.0), g.quarter_annulus())),
        'twisted_box': ('geo_twisted_box', lambda g: g.twisted_box()),
        'bspline_quarter_annulus': ('geo_bspline_quarter_annulus', lambda g: g.bspline_quarter_annulus())}

_oracle_cache = {}


def oracle(kind, kvs, gname):
    """The CPU oracle's matrix (long-double contraction), computed once per (form, knots, map)."""
    from oracle import iga_oracle as orc
    key = (kind, gname, tuple((kv.p, tuple(np.asarray(kv.kv))) for kv in kvs))
    if key not in _oracle_cache:
        okvs = tuple(orc.KnotVector(np.asarray(kv.kv), kv.p) for kv in kvs)
        _oracle_cache[key] = orc.assemble(kind, okvs, getattr(orc, GEOS[gname][0])(), nthreads=8)
    return _oracle_cache[key]


def kv_mults(iga, p, mults):
    n = len(mults) + 1
    inner = np.repeat(np.arange(1, n) / n, mults)
    return iga.bspline.KnotVector(np.concatenate([np.zeros(p + 1), inner, np.ones(p + 1)]), p)


def assemble(iga, monkeypatch, kvs, gname, kind, moving=False, row0=None, env=()):
    """(matrix, last_path, whether the window rotated) of one patch or row slab."""
    with monkeypatch.context() as m:
        m.setenv('IGX_DEBUG_POISON', '1')
        m.delenv(KNOB, raising=False)
        if moving:
            m.setenv(KNOB, '1')
        for k, v in env:
            m.setenv(k, v)
        patch = iga.assemblers.DevicePatch(kvs, GEOS[gname][1](iga.geometry), row0=row0)      # (knobs are read here)
    A = patch.csr(kind, algo='sumfact')
    out = A, patch.last_path(), patch.geoa_rotated()
    patch.close()
    return out


def same_bits(A, B):
    return np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices) and \
        np.array_equal(A.data.view(np.int64), B.data.view(np.int64))


def check(iga, monkeypatch, kvs, gname, kind, rotates=True, path=None, env=()):
    """Default against the moving form (same bits), the oracle and the entry-wise kernels; -> the matrix."""
    A, pa, ra = assemble(iga, monkeypatch, kvs, gname, kind, env=env)
    B, pb, rb = assemble(iga, monkeypatch, kvs, gname, kind, moving=True, env=env)
    tag = (kind, gname, [kv.p for kv in kvs], [kv.numdofs for kv in kvs], sorted(pa))
    assert 'geoA' in pa and pa == pb, tag
    if path is not None:
        assert pa == path, tag
    assert ra == rotates and not rb, (tag, ra, rb)
    assert not np.isnan(A.data).any(), tag
    assert same_bits(A, B), (tag, int((A.data != B.data).sum()))
    assert abs(A - A.T).max() == 0.0, tag
    R = oracle(kind, kvs, gname)
    assert A.shape == R.shape and rel_maxdiff(A, R) <= RTOL, (tag, rel_maxdiff(A, R))
    with monkeypatch.context() as m:
        m.setenv('IGX_DEBUG_POISON', '1')
        patch = iga.assemblers.DevicePatch(kvs, GEOS[gname][1](iga.geometry))
    E = patch.csr(kind, algo='entrywise')
    patch.close()
    assert np.array_equal(A.indptr, E.indptr) and np.array_equal(A.indices, E.indices), tag
    assert rel_maxdiff(A, E) <= RTOL, (tag, rel_maxdiff(A, E))
    return A


def cube(iga, p, n0):
    mk = iga.bspline.make_knots
    return mk(p, 0., 1., n0), mk(p, 0., 1., 2), mk(p, 0., 1., 2)


@pytest.mark.parametrize('extra', [1, 2, 3])
@pytest.mark.parametrize('p', [2, 3, 4])
def test_every_phase_twice_and_the_wrap(iga, monkeypatch, p, extra):
    """Axis 0 with 2P + 1, 2P + 2, 2P + 3 spans at P = 3, 4, 5: every residue of the rotation twice, then the wrap; the last span
    of the axis retires P functions in one span end (the steps behind the first come from the step table)."""
    P = p + 1
    check(iga, monkeypatch, cube(iga, p, 2 * P + extra), 'cylinder' if extra != 2 else 'twisted_box', 'stiffness', path=BF3)


@pytest.mark.parametrize('p', [2, 3, 4])
def test_span_ends_around_a_batch_boundary(iga, monkeypatch, p):
    """q = 3, 4, 5 planes per span against batches of eight: on eight spans a span ends with the last plane of a batch, and for
    q = 3, 5 also one plane before and one plane behind a batch boundary (q = 4 meets a boundary only head-on)."""
    q, n0 = p + 1, 8
    where = {((s + 1) * q) % NS for s in range(n0)}        # planes of the current batch that a span end leaves behind it
    assert 0 in where and (q == 4 or {NS - 1, 1} <= where)
    check(iga, monkeypatch, cube(iga, p, n0), 'twisted_box', 'stiffness', path=BF3)


@pytest.mark.parametrize('n0', [1, 2])
def test_the_last_spans_of_the_axis(iga, monkeypatch, n0):
    """One span: the only span end retires all P functions; two: a single step, then P."""
    check(iga, monkeypatch, cube(iga, 3, n0), 'cylinder', 'stiffness', path=BF3)


@pytest.mark.parametrize('mults', [(1, 2, 1, 1, 1, 1, 1), (1, 1, 3, 1, 1, 2, 1)])
def test_repeated_knots_on_axis_0_take_the_moving_form(iga, monkeypatch, mults):
    """Multiplicity 2 and p on axis 0: the window shifts by the multiplicity, the plan must not rotate."""
    mk = iga.bspline.make_knots
    kvs = (kv_mults(iga, 3, mults), mk(3, 0., 1., 2), mk(3, 0., 1., 2))
    check(iga, monkeypatch, kvs, 'twisted_box', 'stiffness', rotates=False, path=BF3)


@pytest.mark.parametrize('p', [2, 3, 4])
def test_row_slabs_cut_at_every_phase(iga, monkeypatch, p):
    """A 13-span axis cut behind rows 1 .. P + 1: a slab's sweep starts its rotation at the slab's first span, so the cuts put the
    same pair into every register of the rotation; stacked, the slabs are the whole patch bit for bit."""
    P = p + 1
    kvs = cube(iga, p, 13)
    A, path, rot = assemble(iga, monkeypatch, kvs, 'cylinder', 'stiffness')
    assert path == BF3 and rot
    for lo in range(1, P + 2):
        parts = []
        for r0 in ((0, lo), (lo, kvs[0].numdofs)):
            S, spath, srot = assemble(iga, monkeypatch, kvs, 'cylinder', 'stiffness', row0=r0)
            assert spath == BF3 and srot, (r0, sorted(spath))
            parts.append(S)
        V = scipy.sparse.vstack(parts).tocsr()
        assert same_bits(V, A), (p, lo)


def test_diagonal_slices_written_or_skipped(iga, monkeypatch):
    """IGX_NO_DIAG_SKIP=1 against the default: the diagonal pair of a span end is another register in every phase."""
    kvs = cube(iga, 4, 11)
    A, pa, ra = assemble(iga, monkeypatch, kvs, 'cylinder', 'stiffness')
    B, pb, rb = assemble(iga, monkeypatch, kvs, 'cylinder', 'stiffness', env=(('IGX_NO_DIAG_SKIP', '1'),))
    assert pa == pb == BF3 and ra and rb
    assert same_bits(A, B), int((A.data != B.data).sum())
    check(iga, monkeypatch, kvs, 'cylinder', 'stiffness', path=BF3, env=(('IGX_NO_DIAG_SKIP', '1'),))


@pytest.mark.parametrize('p', [2, 4])
def test_mass_form_on_the_same_block(iga, monkeypatch, p):
    """One array: seven of the eight waves of a block evaluate their plane and sweep nothing."""
    check(iga, monkeypatch, cube(iga, p, 2 * p + 5), 'cylinder', 'mass', path=BF3)


@pytest.mark.parametrize('kind', ['stiffness', 'mass'])
def test_2d_instantiation(iga, monkeypatch, kind):
    """2D, 11 x 4 spans (IGX_PATH=unfused: a patch this small would otherwise take the single-launch kernel)."""
    mk = iga.bspline.make_knots
    kvs = (mk(3, 0., 1., 11), mk(3, 0., 1., 4))
    check(iga, monkeypatch, kvs, 'bspline_quarter_annulus', kind, env=(('IGX_PATH', 'unfused'),))

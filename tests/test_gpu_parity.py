"""Parity of the HIP path (through the C ABI) with the oracle, the reference's fixtures and the
golden vectors.  Needs a real MI355X:  pytest -m gpu.

Tolerances:
  * the four bundled fixtures: max|A - A_ref| < 1e-14 absolute (the reference's own tolerance,
    test/test_assemble.py:138-168)
  * everything else: max|A - A_ref| <= 1e-12 * max|A_ref|
"""
import os

import numpy as np
import pytest
import scipy.sparse

from conftest import GOLDEN, golden_csr, rel_maxdiff, form_inputs, form_tables, FORMS, form2d_cases, PFORMS2, PFORMS3, pform_inputs2
import _bf3_cases as bc
import _geoa_cases as gc

pytestmark = pytest.mark.gpu

RTOL = 1e-12


@pytest.fixture(scope='module')
def iga():
    import pyiga_amd
    pyiga_amd._lib.context()          # raises if no GPU / library: there is no fallback
    return pyiga_amd


def _kv(iga, okv):
    return iga.bspline.KnotVector(okv.kv.copy(), okv.p)


def _geo(iga, name):
    g = iga.geometry
    return {'quarter_annulus': g.quarter_annulus, 'bspline_quarter_annulus': g.bspline_quarter_annulus,
            'twisted_box': g.twisted_box, 'unit_square': g.unit_square, 'unit_cube': g.unit_cube,
            'cylinder': lambda: g.tensor_product(g.line_segment(0.0, 1.0), g.quarter_annulus())}[name]()


# ------------------------------------------------------------------------------------------
def test_knots_bits(iga, golden):
    g = golden('knots')
    for key in g.files:
        if key.startswith('leggauss') or key in ('p3_n5_m2', 'p2_ab'):
            continue
        p, n = (int(x[1:]) for x in key.split('_'))
        assert np.array_equal(iga.bspline.make_knots(p, 0.0, 1.0, n).kv, g[key])
    assert np.array_equal(iga.bspline.make_knots(3, 0.0, 1.0, 5, mult=2).kv, g['p3_n5_m2'])


def test_active_deriv(iga, golden):
    """bspline_cy.active_deriv / pyx_findspan on the device vs the reference's values."""
    g = golden('bspline')
    for name in sorted({k[:-3] for k in g.files if k.endswith('_kv')}):
        kv = iga.bspline.KnotVector(g[name + '_kv'], int(g[name + '_p']))
        nodes = g[name + '_nodes']
        ref = g[name + '_deriv']
        out = iga.bspline.active_deriv(kv, nodes, 1)
        assert out.shape == ref.shape
        assert np.abs(out - ref).max() <= 1e-14 * np.abs(ref).max(), name
        assert np.array_equal(iga.bspline.findspans(kv, nodes), g[name + '_spans'])
        assert np.array_equal(kv.mesh_support_idx_all(), g[name + '_meshsupp'])
        # scalar argument form
        one = iga.bspline.active_deriv(kv, float(nodes[3]), 1)
        assert one.shape == (2, kv.p + 1) and np.allclose(one, ref[:, :, 3], rtol=0, atol=1e-13)
        # second derivatives agree with the oracle's restatement
        from oracle import iga_oracle as orc
        okv = orc.KnotVector(g[name + '_kv'], kv.p)
        d2 = iga.bspline.active_deriv(kv, nodes, 2)
        r2 = orc.active_deriv(okv, nodes, 2)
        assert np.abs(d2 - r2).max() <= 1e-13 * max(1.0, np.abs(r2).max())
    # boundary points: u = last knot belongs to the last span
    kv = iga.bspline.make_knots(3, 0.0, 1.0, 4)
    assert iga.bspline.findspans(kv, np.array([0.0, 1.0]))[1] == kv.kv.size - kv.p - 2


@pytest.mark.parametrize('name', ['quarter_annulus', 'bspline_quarter_annulus', 'twisted_box', 'cylinder',
                                  'unit_square', 'unit_cube'])
def test_grid_jacobian(iga, golden, name):
    g = golden('geometry')
    geo = _geo(iga, name)
    assert np.allclose(geo.coeffs, g[name + '_coeffs'], rtol=0, atol=1e-15)
    d = geo.sdim
    grid = [g['%s_grid%d' % (name, k)] for k in range(d)]
    jac = geo.grid_jacobian(grid)
    assert jac.shape == g[name + '_jac'].shape
    assert np.abs(jac - g[name + '_jac']).max() < 1e-13
    ev = geo.grid_eval(grid)
    assert np.abs(ev - g[name + '_eval']).max() < 1e-13


def test_fields(iga, oracle):
    """precompute_fields on the device vs the oracle (assemblers.pyx:1389-1449 etc.)."""
    for d, gname, ogeo, p, n in ((2, 'quarter_annulus', oracle.geo_quarter_annulus(), 3, 5),
                                 (3, 'cylinder', oracle.geo_cylinder(), 2, 3),
                                 (3, 'twisted_box', oracle.geo_twisted_box(), 3, 2)):
        okv = oracle.make_knots(p, 0., 1., n)
        kvs = (_kv(iga, okv),) * d
        patch = iga.assemblers.DevicePatch(kvs, _geo(iga, gname))
        for kind in ('mass', 'stiffness'):
            oasm = oracle.Assembler(kind, (okv,) * d, ogeo)
            F = patch.fields(kind)                       # (F, G0, G1[, G2])
            ref = np.moveaxis(oasm.fields, -1, 0)
            assert F.shape == ref.shape
            assert np.abs(F - ref).max() <= 1e-13 * np.abs(ref).max()
        for k in range(d):
            nodes, w = patch.gauss(k)
            assert np.array_equal(nodes, oasm.grid[k]) and np.array_equal(w, oasm.gw[k])
        patch.close()


def test_pattern(iga, oracle, golden):
    g = golden('sparsity')
    for name, d in (('d3_p2_n3', 3), ('d2_p3_n4', 2), ('d2_mixed', 2), ('d3_mult', 3)):
        kvs = tuple(iga.bspline.KnotVector(g['%s_kv%d' % (name, k)], int(g['%s_p%d' % (name, k)])) for k in range(d))
        geo = iga.geometry.unit_cube(dim=d)
        patch = iga.assemblers.DevicePatch(kvs, geo)
        indptr, indices = patch.pattern()
        n = patch.shape[0]
        I, J = g[name + '_lt0_I'], g[name + '_lt0_J']
        R = scipy.sparse.coo_matrix((np.ones(len(I)), (I, J)), shape=(n, n)).tocsr()
        R.sort_indices()
        assert indptr.dtype == np.int32 and indices.dtype == np.int32
        assert np.array_equal(indptr, R.indptr) and np.array_equal(indices, R.indices)
        # host-side emission order of the generic driver matches the reference
        for lt in (0, 1):
            I2, J2 = iga.assemble._ml_nonzero(kvs, kvs, lower_tri=bool(lt))
            assert np.array_equal(I2, g['%s_lt%d_I' % (name, lt)]) and np.array_equal(J2, g['%s_lt%d_J' % (name, lt)])
        patch.close()


def test_multi_entries(iga, golden):
    g = golden('entries')
    kv = iga.bspline.make_knots(2, 0., 1., 4)
    cyl = _geo(iga, 'cylinder')
    for name, cls in (('stiff3d', iga.assemblers.StiffnessAssembler3D), ('mass3d', iga.assemblers.MassAssembler3D)):
        asm = cls((kv, kv, kv), cyl)
        assert asm.arity == 2 and asm.kvs[0][0] is kv
        idx, ref = g[name + '_idx'], g[name + '_multi']
        out = asm.multi_entries(idx)
        assert np.abs(out - ref).max() <= RTOL * np.abs(ref).max()
        assert np.array_equal(out == 0.0, ref == 0.0)        # out-of-pattern pairs -> exact 0.0
        assert asm.entry(int(idx[2, 0]), int(idx[2, 1])) == out[2]
        assert np.array_equal(asm.multi_entries([tuple(r) for r in idx[:5]]), out[:5])   # iterable of pairs
    kv2 = iga.bspline.make_knots(3, 0., 1., 6)
    for name, cls in (('stiff2d', iga.assemblers.StiffnessAssembler2D), ('mass2d', iga.assemblers.MassAssembler2D)):
        asm = cls((kv2, kv2), _geo(iga, 'quarter_annulus'))
        out = asm.multi_entries(g[name + '_idx'])
        ref = g[name + '_multi']
        assert np.abs(out - ref).max() <= RTOL * np.abs(ref).max()


FIXTURES = [('d2_p3_n15', 'mass', 2), ('d2_p3_n15', 'stiff', 2), ('d3_p2_n10', 'mass', 3), ('d3_p2_n10', 'stiff', 3)]


@pytest.mark.parametrize('algo', ['sumfact', 'entrywise'])
@pytest.mark.parametrize('tag,kind,d', FIXTURES)
def test_reference_fixtures(iga, tag, kind, d, algo):
    """test/test_assemble.py:138-168 with the reference's own files and tolerance."""
    if d == 2:
        kvs = (iga.bspline.make_knots(3, 0.0, 1.0, 15),) * 2
        geo = iga.geometry.bspline_quarter_annulus()
        cls = iga.assemblers.MassAssembler2D if kind == 'mass' else iga.assemblers.StiffnessAssembler2D
    else:
        kvs = (iga.bspline.make_knots(2, 0.0, 1.0, 10),) * 3
        geo = iga.geometry.twisted_box()
        cls = iga.assemblers.MassAssembler3D if kind == 'mass' else iga.assemblers.StiffnessAssembler3D
    A = iga.assemble.assemble_entries(cls(kvs, geo), symmetric=True, algo=algo)
    A_ref = iga.utils.read_sparse_matrix(os.path.join(GOLDEN, 'poisson_neu_%s_%s.mtx.gz' % (tag, kind)))
    assert abs(A - A_ref).max() < 1e-14
    assert abs(A - A.T).max() == 0.0                      # exactly symmetric, like the reference
    assert A.data.dtype == np.float64 and A.indices.dtype == np.int32 and A.has_canonical_format
    # public API (auto algorithm)
    fn = iga.assemble.mass if kind == 'mass' else iga.assemble.stiffness
    assert abs(fn(kvs, geo) - A_ref).max() < 1e-14


def _matrix_cases(iga):
    mk = iga.bspline.make_knots
    return [
        ('d2_p3_n8_annulus_mass', 'mass', (mk(3, 0., 1., 8),) * 2, 'quarter_annulus', False),
        ('d2_p3_n8_annulus_stiff', 'stiffness', (mk(3, 0., 1., 8),) * 2, 'quarter_annulus', False),
        ('d2_p43_n56_square_mass', 'mass', (mk(4, 0., 1., 5), mk(3, 0., 1., 6)), 'unit_square', False),
        ('d2_p43_n56_square_stiff', 'stiffness', (mk(4, 0., 1., 5), mk(3, 0., 1., 6)), 'unit_square', False),
        ('d2_mult_annulus_mass', 'mass', (mk(3, 0., 1., 5, mult=2), mk(2, 0., 1., 4)), 'bspline_quarter_annulus', False),
        ('d2_mult_annulus_stiff', 'stiffness', (mk(3, 0., 1., 5, mult=2), mk(2, 0., 1., 4)), 'bspline_quarter_annulus', False),
        ('d3_p4_n3_cyl_stiff_lower', 'stiffness', (mk(4, 0., 1., 3),) * 3, 'cylinder', True),
        ('d3_p5_n3_cyl_stiff_lower', 'stiffness', (mk(5, 0., 1., 3),) * 3, 'cylinder', True),
        ('d3_p323_n342_tbox_mass_lower', 'mass', (mk(3, 0., 1., 3), mk(2, 0., 1., 4), mk(3, 0., 1., 2)), 'twisted_box', True),
        ('d3_p323_n342_tbox_stiff_lower', 'stiffness', (mk(3, 0., 1., 3), mk(2, 0., 1., 4), mk(3, 0., 1., 2)), 'twisted_box', True),
        ('d3_mult_cyl_stiff_lower', 'stiffness', (mk(2, 0., 1., 3, mult=2), mk(2, 0., 1., 3), mk(3, 0., 1., 2)), 'cylinder', True),
        ('d3_mult_cyl_mass_lower', 'mass', (mk(2, 0., 1., 3, mult=2), mk(2, 0., 1., 3), mk(3, 0., 1., 2)), 'cylinder', True),
    ] + [(name + sfx, kind, kvs, 'cylinder', True) for name, kvs in _r6_shapes(iga).items()
         for sfx, kind in (('_stiff_lower', 'stiffness'), ('_mass_lower', 'mass'))]


def _r6_shapes(iga):
    """Round 6: the shapes k_bf3 was generalised to (round 5: repeated knots on the mid axis, mid / last axis one degree below
    nqp) and is being generalised to (repeated knots on the last axis, a degree gap of two), as reference-made matrices."""
    mk = iga.bspline.make_knots
    return {'d3_midmult_cyl': (mk(3, 0., 1., 3), mk(3, 0., 1., 5, mult=2), mk(3, 0., 1., 4)),
            'd3_p443_cyl': (mk(4, 0., 1., 3), mk(4, 0., 1., 4), mk(3, 0., 1., 5)),
            'd3_p433_cyl': (mk(4, 0., 1., 3), mk(3, 0., 1., 5), mk(3, 0., 1., 5)),
            'd3_lastmult_cyl': (mk(3, 0., 1., 3), mk(3, 0., 1., 4), mk(3, 0., 1., 5, mult=2)),
            'd3_p424_cyl': (mk(4, 0., 1., 3), mk(2, 0., 1., 5), mk(4, 0., 1., 4))}


@pytest.mark.parametrize('algo', ['sumfact', 'entrywise'])
def test_golden_matrices(iga, golden, algo, monkeypatch):
    """Full matrices produced by the real reference: NURBS, unequal degrees per axis (shared
    nqp = max p + 1), repeated interior knots, p = 4 and 5 in 3D."""
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')           # NaN-fill: every value must be written
    g = golden('matrices')
    for name, kind, kvs, gname, lower in _matrix_cases(iga):
        fn = iga.assemble.bsp_mass_2d if kind == 'mass' else iga.assemble.bsp_stiffness_2d   # any d
        cls = iga.assemble._ASSEMBLER[(kind, len(kvs))]
        A = iga.assemble.assemble_entries(cls(kvs, _geo(iga, gname)), symmetric=True, algo=algo)
        assert not np.isnan(A.data).any(), name
        assert abs(A - A.T).max() == 0.0
        if lower:
            A = scipy.sparse.tril(A, format='csr')
        R = golden_csr(g, name)
        assert A.shape == R.shape and A.nnz >= R.nnz
        assert rel_maxdiff(A, R) <= RTOL, (name, rel_maxdiff(A, R))
        del fn


def test_kronecker_path(iga, golden):
    """geo=None -> Kronecker product of 1D matrices; identity geometry gives the same matrix
    (test/test_assemble.py:10-40,83-100)."""
    g = golden('kron')
    kv = iga.bspline.KnotVector(g['kv1d'], 4)
    assert np.abs(iga.assemble.bsp_mass_1d(kv).toarray() - g['M1d']).max() < 1e-14
    assert np.abs(iga.assemble.bsp_stiffness_1d(kv).toarray() - g['K1d']).max() < 1e-12
    assert np.abs(iga.assemble.mass(kv).toarray() - g['M1d']).max() < 1e-14
    mk = iga.bspline.make_knots
    kvs2 = (mk(4, 0., 1., 10), mk(3, 0., 1., 12))
    kvs3 = (mk(3, 0., 1., 4), mk(3, 0., 1., 5), mk(3, 0., 1., 6))
    for name, fn, kvs in (('kron2d_stiff', iga.assemble.stiffness, kvs2), ('kron2d_mass', iga.assemble.mass, kvs2),
                          ('kron3d_stiff', iga.assemble.stiffness, kvs3), ('kron3d_mass', iga.assemble.mass, kvs3)):
        assert rel_maxdiff(fn(kvs), golden_csr(g, name)) < 1e-13
    assert np.allclose(iga.assemble.bsp_stiffness_2d(kvs2, geo=None).toarray(),
                       iga.assemble.bsp_stiffness_2d(kvs2, geo=iga.geometry.unit_square()).toarray(), rtol=0, atol=1e-14)
    assert np.allclose(iga.assemble.bsp_stiffness_3d(kvs3, geo=None).toarray(),
                       iga.assemble.bsp_stiffness_3d(kvs3, geo=iga.geometry.unit_cube()).toarray(), rtol=0, atol=1e-14)


def test_api_errors(iga):
    kv = iga.bspline.make_knots(2, 0., 1., 4)
    with pytest.raises(AssertionError):
        iga.assemble.mass(kv, geo=iga.geometry.unit_square())            # 1D rejects geo
    with pytest.raises(AssertionError):
        iga.assemble.stiffness((kv, kv, kv), geo=iga.geometry.unit_square())   # dimension mismatch
    with pytest.raises(AssertionError):
        iga.assemble.stiffness((kv,) * 4, geo=None)
    A = iga.assemble.stiffness((kv, kv), iga.geometry.unit_square(), format='csc')
    assert A.format == 'csc'


class _OpaqueGeo:
    """A geometry object that only offers grid_jacobian (like pyiga's UserFunction)."""

    def __init__(self, inner):
        self._inner = inner
        self.dim, self.sdim = inner.dim, inner.sdim

    def grid_jacobian(self, grid):
        return self._inner.grid_jacobian(grid)


def test_jacobian_array_geometry(iga):
    kv = iga.bspline.make_knots(3, 0., 1., 5)
    for geo, kvs in ((iga.geometry.quarter_annulus(), (kv, kv)), (_geo(iga, 'cylinder'), (kv, kv, kv))):
        for fn in (iga.assemble.mass, iga.assemble.stiffness):
            A = fn(kvs, geo)
            B = fn(kvs, _OpaqueGeo(geo))
            assert rel_maxdiff(B, A) < 1e-14


def test_foreign_assembler_driver(iga, oracle):
    """assemble_entries drives any object with the reference's assembler interface."""
    okv = oracle.make_knots(2, 0., 1., 4)
    oasm = oracle.Assembler('stiffness', (okv, okv), oracle.geo_quarter_annulus())

    class Foreign:
        arity = 2
        kvs = ((_kv(iga, okv),) * 2,) * 2

        def multi_entries(self, idx):
            return oasm.multi_entries(idx)
    A = iga.assemble.assemble_entries(Foreign(), symmetric=True)
    kv = _kv(iga, okv)
    B = iga.assemble.stiffness((kv, kv), iga.geometry.quarter_annulus())
    assert rel_maxdiff(A, B) < RTOL


# ------------------------------------------------------------------------------------------
# size-independent properties at larger sizes (no oracle needed)
@pytest.mark.parametrize('d,p,n', [(2, 3, 256), (3, 2, 24), (3, 4, 10), (2, 5, 40), (3, 1, 12)])
def test_properties_larger(iga, d, p, n, monkeypatch):
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')
    kv = iga.bspline.make_knots(p, 0., 1., n)
    geo = iga.geometry.quarter_annulus() if d == 2 else _geo(iga, 'cylinder')
    kvs = (kv,) * d
    K = iga.assemble.stiffness(kvs, geo)
    M = iga.assemble.mass(kvs, geo)
    for A in (K, M):
        assert not np.isnan(A.data).any()
        assert abs(A - A.T).max() == 0.0
    # constants are in the kernel of the stiffness form (partition of unity)
    assert np.abs(K @ np.ones(K.shape[0])).max() <= 1e-11 * abs(K).max()
    # sum of the mass matrix = measure of the domain: quarter annulus r in [1,2] (x height 1)
    # (the integrand |det J| is rational for NURBS: Gauss quadrature converges, it is not exact)
    assert abs(M.sum() - 0.75 * np.pi) < (1e-5 if p < 2 else 1e-9)
    # sum-factorised == entry-wise at this size
    if K.nnz < 3e7:
        cls = iga.assemble._ASSEMBLER[('stiffness', d)]
        E = cls(kvs, geo).assemble_csr(algo='entrywise')
        assert rel_maxdiff(K, E) <= RTOL


@pytest.mark.parametrize('algo', ['sumfact', 'entrywise'])
@pytest.mark.parametrize('d,p,n,G', [(3, 2, 9, 2), (3, 3, 7, 3), (2, 3, 20, 4), (3, 4, 6, 2), (2, 2, 200, 5), (2, 3, 90, 3)])
def test_row_slabs_equal_full(iga, d, p, n, G, algo, monkeypatch):
    """Multi-GPU decomposition: each slab of axis-0 dof planes reproduces its rows of the full
    matrix bit for bit, with no exchange between slabs.  (2D, n = 200 / 90: the whole patch is beyond / just inside the
    single-launch kernel's range while a slab alone would be well inside it: the path is chosen for the patch, not the slab.)"""
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')
    kv = iga.bspline.make_knots(p, 0., 1., n)
    kvs = (kv,) * d
    geo = iga.geometry.quarter_annulus() if d == 2 else _geo(iga, 'cylinder')
    for kind in ('mass', 'stiffness'):
        full = iga.assemblers.DevicePatch(kvs, geo).csr(kind, algo=algo)
        N0 = kv.numdofs
        bounds = [N0 * g // G for g in range(G + 1)]
        blocks = []
        for g in range(G):
            patch = iga.assemblers.DevicePatch(kvs, geo, row0=(bounds[g], bounds[g + 1]))
            blk = patch.csr(kind, algo=algo)
            assert not np.isnan(blk.data).any()
            lo, hi = patch.row_range
            assert blk.shape[0] == hi - lo
            blocks.append(blk)
            patch.close()
        stacked = scipy.sparse.vstack(blocks).tocsr()
        assert stacked.shape == full.shape and stacked.nnz == full.nnz
        assert np.array_equal(stacked.indices, full.indices) and np.array_equal(stacked.indptr, full.indptr)
        assert np.array_equal(stacked.data, full.data)


def test_final_stage_variants_agree(iga, monkeypatch):
    """The three final-stage kernels (quadrature-lane: default where it applies; LDS-table VALU; matrix-core)
    give the same matrix, each exactly symmetric -- and each the oracle's (a mistake the three share does not pass); degrees 2
    to 5.  (Every instantiation of the three, one case each: tests/_stage_cases.py, tests/test_stage_kernels_gpu.py.)"""
    from oracle import iga_oracle as orc
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')
    mk = iga.bspline.make_knots
    cases = [((mk(2, 0., 1., 10),) * 3, 'twisted_box'), ((mk(4, 0., 1., 5),) * 3, 'cylinder'),
             ((mk(3, 0., 1., 40), mk(3, 0., 1., 33)), 'quarter_annulus'),
             ((mk(2, 0., 1., 3, mult=2), mk(2, 0., 1., 3), mk(3, 0., 1., 4)), 'cylinder'),
             ((mk(5, 0., 1., 2), mk(5, 0., 1., 2), mk(5, 0., 1., 3)), 'cylinder')]
    for kvs, gname in cases:
        okvs = tuple(orc.KnotVector(np.asarray(kv.kv), kv.p) for kv in kvs)
        for kind in ('mass', 'stiffness'):
            R = orc.assemble(kind, okvs, getattr(orc, 'geo_' + gname)(), nthreads=8)
            out = {}
            for sel in ('q', 'valu', 'mfma'):
                monkeypatch.setenv('IGX_FINAL', sel)
                patch = iga.assemblers.DevicePatch(kvs, _geo(iga, gname))
                out[sel] = patch.csr(kind, algo='sumfact')
                patch.close()
                assert not np.isnan(out[sel].data).any()
                assert abs(out[sel] - out[sel].T).max() == 0.0
                assert out[sel].nnz == R.nnz and rel_maxdiff(out[sel], R) <= RTOL, (sel, kind, gname, rel_maxdiff(out[sel], R))
            assert rel_maxdiff(out['mfma'], out['valu']) <= 1e-14
            assert rel_maxdiff(out['q'], out['valu']) <= 1e-14
    monkeypatch.delenv('IGX_FINAL')


CONVDIFF = '(inner(diff_coeff*grad(u),grad(v)) + inner((x[1],-x[0],1.0),grad(u))*v)*dx'


@pytest.mark.parametrize('algo', ['auto', 'sumfact', 'entrywise'])
def test_convdiff_custom_form(iga, golden, algo, monkeypatch):
    """Row f1 of SURVEY section 8 (BASELINE config 5): the run-time compiled convection-diffusion form,
    non-symmetric, against matrices produced by the real reference."""
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')
    g = golden('convdiff')
    mk = iga.bspline.make_knots
    cases = [('d3_p2_n3_cyl', (mk(2, 0., 1., 3),) * 3, 'cylinder'),
             ('d3_p32_n243_tbox', (mk(3, 0., 1., 2), mk(2, 0., 1., 4), mk(2, 0., 1., 3)), 'twisted_box'),
             ('d3_mult_cyl', (mk(2, 0., 1., 3, mult=2), mk(2, 0., 1., 3), mk(3, 0., 1., 2)), 'cylinder')]
    for name, kvs, gname in cases:
        geo = _geo(iga, gname)
        asm = iga.assemblers.ConvDiffAssembler3D(kvs, geo, lambda x, y, z: 1.0 + x)
        A = iga.assemble.assemble_entries(asm, symmetric=False, algo=algo)
        R = golden_csr(g, name)
        assert A.shape == R.shape and A.nnz == R.nnz and not np.isnan(A.data).any()
        assert rel_maxdiff(A, R) <= RTOL, (name, rel_maxdiff(A, R))
        out = asm.multi_entries(g[name + '_idx'])
        ref = g[name + '_multi']
        assert np.abs(out - ref).max() <= RTOL * np.abs(ref).max()
        assert np.array_equal(out == 0.0, ref == 0.0)
    # the reference's string interface
    kv = mk(2, 0., 1., 3)
    A = iga.assemble.assemble(CONVDIFF, (kv, kv, kv), geo=_geo(iga, 'cylinder'), diff_coeff=lambda x, y, z: 1.0 + x)
    assert rel_maxdiff(A, golden_csr(g, 'd3_p2_n3_cyl')) <= RTOL
    assert rel_maxdiff(iga.assemble.assemble('inner(grad(u), grad(v)) * dx', (kv, kv, kv), geo=_geo(iga, 'cylinder')),
                       iga.assemble.stiffness((kv, kv, kv), _geo(iga, 'cylinder'))) == 0.0
    with pytest.raises(NotImplementedError):
        iga.assemble.assemble('u * dx(v) * dx', (kv, kv, kv), geo=_geo(iga, 'cylinder'))


@pytest.mark.parametrize('p,n,G', [(2, 9, 2), (3, 7, 3), (4, 6, 2), (1, 8, 3)])
def test_convdiff_sumfact_vs_oracle_and_slabs(iga, oracle, p, n, G, monkeypatch):
    """Non-symmetric sum factorisation: against the oracle's entry-wise sums, against the device
    entry-wise kernels, and slab by slab (bit-identical rows, no exchange)."""
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')
    coeff = lambda x, y, z: 1.0 + x * x + 0.5 * z
    kvs = (iga.bspline.make_knots(p, 0., 1., n), iga.bspline.make_knots(p, 0., 1., n + 1, mult=min(p, 2)),
           iga.bspline.make_knots(p, 0., 1., n - 1))
    okvs = tuple(oracle.KnotVector(kv.kv, kv.p) for kv in kvs)
    asm = iga.assemblers.ConvDiffAssembler3D(kvs, _geo(iga, 'cylinder'), coeff)
    A = asm.assemble_csr(algo='sumfact')
    assert asm.patch.timing()['algo_used'] == 2 and not np.isnan(A.data).any()
    E = asm.assemble_csr(algo='entrywise')
    R = oracle.assemble_nonsymmetric('convdiff', okvs, oracle.geo_cylinder(), coeff=coeff, nthreads=8)
    assert A.nnz == R.nnz and np.array_equal(A.indices, R.indices) and np.array_equal(A.indptr, R.indptr)
    assert rel_maxdiff(A, R) <= RTOL and rel_maxdiff(A, E) <= RTOL
    assert abs(A - A.T).max() > 1e-3 * abs(A).max()          # really non-symmetric
    N0 = kvs[0].numdofs
    bounds = [N0 * g // G for g in range(G + 1)]
    blocks = []
    for g in range(G):
        sl = iga.assemblers.ConvDiffAssembler3D(kvs, _geo(iga, 'cylinder'), coeff, row0=(bounds[g], bounds[g + 1]))
        blocks.append(sl.assemble_csr(algo='sumfact'))
        sl.patch.close()
    S = scipy.sparse.vstack(blocks).tocsr()
    assert np.array_equal(S.indices, A.indices) and np.array_equal(S.indptr, A.indptr) and np.array_equal(S.data, A.data)


# ---------------------------------------------------------------------------------------------
# load vectors
def _f3(x, y, z):
    return np.cos(x) * np.exp(y) * np.sin(z)


def _f2(x, y):
    return np.exp(x + y)


def _close(a, b, tol=RTOL):
    return a.shape == b.shape and np.abs(a - b).max() <= tol * np.abs(b).max()


def test_inner_products_vs_reference(iga, golden):
    """inner_products and the L2Functional assemblers against vectors from the real reference
    (recipes: test/test_assemble.py:223-245)."""
    g = golden('rhs')
    mk = iga.bspline.make_knots
    ip = iga.assemble.inner_products
    kvs = [mk(p, 0.0, 1.0, 8 + p) for p in range(3, 6)]
    tbox, ann = _geo(iga, 'twisted_box'), _geo(iga, 'quarter_annulus')
    assert _close(ip(kvs, _f3), g['d3_param'])
    assert _close(ip(kvs, _f3, geo=iga.geometry.unit_cube()), g['d3_param'])
    assert _close(ip(kvs, _f3, geo=tbox), g['d3_tbox'])
    assert _close(ip(kvs, _f3, f_physical=True, geo=tbox), g['d3_tbox_phys'])
    asm = iga.assemblers.L2FunctionalAssembler3D(kvs, tbox, f=_f3)
    assert asm.arity == 1 and _close(asm.assemble_vector(), g['d3_tbox_asm'])
    v = asm.assemble_vector().ravel()
    assert asm.entry1(37) == v[37] and np.array_equal(asm.multi_entries1([0, 5, v.size - 1]), v[[0, 5, v.size - 1]])
    assert _close(iga.assemblers.L2FunctionalAssemblerPhys3D(kvs, tbox, f=_f3).assemble_vector(), g['d3_tbox_phys_asm'])
    kv3 = (mk(2, 0.0, 1.0, 5), mk(3, 0.0, 1.0, 4, mult=2), mk(2, 0.0, 1.0, 6))
    assert _close(ip(kv3, _f3, f_physical=True, geo=_geo(iga, 'cylinder')), g['d3_cyl_phys'])
    kv2 = (mk(3, 0.0, 1.0, 6), mk(2, 0.0, 1.0, 5))
    assert _close(ip(kv2, _f2), g['d2_param'])
    assert _close(ip(kv2, _f2, geo=ann), g['d2_ann'])
    assert _close(ip(kv2, _f2, f_physical=True, geo=ann), g['d2_ann_phys'])
    assert _close(ip(kv2, lambda x, y: (x * y, x - y), f_physical=True, geo=ann), g['d2_ann_vec_phys'])
    assert _close(iga.assemblers.L2FunctionalAssembler2D(kv2, ann, f=_f2).assemble_vector(), g['d2_ann_asm'])
    sp = iga.bspline.BSplineFunc(kv2, np.arange(kv2[0].numdofs * kv2[1].numdofs, dtype=float).reshape(kv2[0].numdofs, -1) / 10.0)
    assert _close(ip(kv2, sp, geo=ann), g['d2_splinef'])
    assert _close(ip(mk(3, 0.0, 1.0, 7), lambda x: 1 + x ** 2), g['d1_param'])
    with pytest.raises(AssertionError):
        ip(kv2, _f2, f_physical=True)


def test_poisson_solve_end_to_end(iga, golden):
    """test/test_solve.py:6-32 with the two assembled objects (stiffness matrix, load vector) coming from the
    device and everything else (boundary dofs and values, the reference's solution) from the fixture."""
    import scipy.sparse.linalg
    g = golden('rhs')
    kvs = 2 * (iga.bspline.make_knots(3, 0.0, 1.0, 10),)
    ann = _geo(iga, 'quarter_annulus')
    rhs = iga.assemble.inner_products(kvs, lambda x, y: 2 * (np.cos(x + y) - np.exp(y - x)), f_physical=True, geo=ann).ravel()
    assert np.abs(rhs - g['poisson2d_rhs']).max() <= RTOL * np.abs(g['poisson2d_rhs']).max()
    A = iga.assemble.stiffness(kvs, geo=ann)
    bc_idx, bc_val = g['poisson2d_bc_idx'], g['poisson2d_bc_val']
    free = np.setdiff1d(np.arange(A.shape[0]), bc_idx)
    u = np.zeros(A.shape[0])
    u[bc_idx] = bc_val
    b = rhs[free] - A[free][:, bc_idx] @ bc_val
    u[free] = scipy.sparse.linalg.spsolve(A[free][:, free].tocsc(), b)
    assert np.abs(u - g['poisson2d_u']).max() <= 1e-10 * np.abs(g['poisson2d_u']).max()
    assert np.sqrt(np.mean((u - g['poisson2d_u_ex']) ** 2)) < 5e-5


@pytest.mark.parametrize('d,p,n,G', [(3, 2, 9, 2), (3, 4, 6, 3), (2, 3, 20, 4)])
def test_load_vector_slabs_and_oracle(iga, oracle, d, p, n, G):
    """Row slabs reproduce their part of the load vector bit for bit; the whole vector matches the oracle."""
    kv = iga.bspline.make_knots(p, 0., 1., n)
    kvs = (kv,) * d
    geo = _geo(iga, 'quarter_annulus' if d == 2 else 'cylinder')
    ogeo = oracle.geo_quarter_annulus() if d == 2 else oracle.geo_cylinder()
    f = _f2 if d == 2 else _f3
    full = iga.assemble.inner_products(kvs, f, f_physical=True, geo=geo)
    ref = oracle.inner_products((oracle.make_knots(p, 0., 1., n),) * d, f, f_physical=True, geo=ogeo)
    assert _close(full, ref)
    grid = None
    N0 = kv.numdofs
    bounds = [N0 * k // G for k in range(G + 1)]
    parts = []
    for k in range(G):
        patch = iga.assemblers.DevicePatch(kvs, geo, row0=(bounds[k], bounds[k + 1]))
        if grid is None:
            grid = tuple(patch.gauss(a)[0] for a in range(d))
            fvals = iga.utils.grid_eval_transformed(f, grid, geo)
        parts.append(patch.load_vector(fvals))
        patch.close()
    # (inner_products evaluates a plain callable on the device -- device libm; the slabs here get the host's samples: compare
    # them with the whole patch on the same samples, bit for bit, and the two ways of sampling to rounding)
    whole = iga.assemblers.DevicePatch(kvs, geo)
    full_sampled = whole.load_vector(fvals)
    whole.close()
    assert np.array_equal(np.concatenate(parts, axis=0), full_sampled)
    assert np.abs(full - full_sampled).max() <= 1e-13 * np.abs(full_sampled).max()


@pytest.mark.parametrize('p,n1', [(2, 37), (3, 40), (4, 48), (5, 33), (5, 65), (4, 41), (3, 67)])
def test_load_vector_fused_chunks(iga, oracle, p, n1):
    """k_lv12 (round 4: the first two contractions of the 3D load vector in one kernel) with SEVERAL chunks of the mid axis:
    the dofs shared by two chunks are added onto zeros (two addends: the order cannot matter) -- against the oracle,
    repeatable bit for bit, slab by slab, and with a differentiated basis (the jet functional)."""
    mk = iga.bspline.make_knots
    kvs = (mk(p, 0., 1., 4), mk(p, 0., 1., n1), mk(p, 0., 1., 6))
    geo = _geo(iga, 'cylinder')
    full = iga.assemble.inner_products(kvs, _f3, f_physical=True, geo=geo)
    okvs = tuple(oracle.make_knots(p, 0., 1., n) for n in (4, n1, 6))
    ref = oracle.inner_products(okvs, _f3, f_physical=True, geo=oracle.geo_cylinder())
    assert _close(full, ref)
    for _ in range(3):
        assert np.array_equal(iga.assemble.inner_products(kvs, _f3, f_physical=True, geo=geo), full)
    N0 = kvs[0].numdofs
    parts, fvals = [], None
    for lo, hi in ((0, 2), (2, N0)):
        patch = iga.assemblers.DevicePatch(kvs, geo, row0=(lo, hi))
        if fvals is None:
            fvals = iga.utils.grid_eval_transformed(_f3, tuple(patch.gauss(a)[0] for a in range(3)), geo)
        parts.append(patch.load_vector(fvals))
        patch.close()
    whole = iga.assemblers.DevicePatch(kvs, geo)                  # (the same host samples for the whole patch: bit for bit)
    full_sampled = whole.load_vector(fvals)
    whole.close()
    assert np.array_equal(np.concatenate(parts, axis=0), full_sampled)
    assert np.abs(full - full_sampled).max() <= 1e-13 * np.abs(full_sampled).max()
    # gradient functional (differentiated basis functions on each axis in turn): the basis is a partition of unity, so the
    # whole vector of  inner(c, grad(v)) dx  sums to zero; against the separate contractions of an unequal-degree space
    cube = iga.geometry.unit_cube()
    fz = iga.assemble.assemble('inner((1.0, 2.0, -3.0), grad(v)) * dx', kvs, geo=cube)
    assert fz.shape == full.shape and abs(fz.sum()) <= 1e-12 * np.abs(fz).max() * fz.size
    assert np.array_equal(iga.assemble.assemble('inner((1.0, 2.0, -3.0), grad(v)) * dx', kvs, geo=cube), fz)


def test_partial_rows(iga):
    """arbitrary row subsets through batched multi_entries (pyiga/_hdiscr.py:5-11)."""
    mk = iga.bspline.make_knots
    for kvs, gname, cls in (((mk(3, 0., 1., 7), mk(2, 0., 1., 9, mult=2)), 'quarter_annulus', iga.assemblers.StiffnessAssembler2D),
                            ((mk(2, 0., 1., 5), mk(3, 0., 1., 4), mk(2, 0., 1., 6)), 'cylinder', iga.assemblers.MassAssembler3D)):
        asm = cls(kvs, _geo(iga, gname))
        A = iga.assemble.assemble_entries(asm, symmetric=True)
        n = A.shape[0]
        rows = np.array([0, n - 1, n // 2, 3, n // 3, n // 3 + 1])
        S = iga.assemble.assemble_partial_rows(asm, rows)
        assert S.shape == A.shape
        mask = np.zeros(n, bool)
        mask[rows] = True
        assert S[~mask].nnz == 0
        ref = A[rows]
        got = S[rows]
        assert np.array_equal(ref.indices, got.indices) and np.array_equal(ref.indptr, got.indptr)
        assert np.abs(ref.data - got.data).max() <= RTOL * np.abs(A.data).max()
        assert iga.assemble.assemble_partial_rows(asm, []).nnz == 0


def test_convdiff_properties_large(iga):
    """Beyond the oracle's reach: the form annihilates constants (a(1, v) = 0, so every row sums to zero),
    the sum-factorised stages agree with the entry-wise kernel on scattered rows, nothing is left unwritten."""
    os.environ['IGX_DEBUG_POISON'] = '1'
    try:
        kvs = (iga.bspline.make_knots(3, 0., 1., 20), iga.bspline.make_knots(4, 0., 1., 14), iga.bspline.make_knots(3, 0., 1., 17))
        asm = iga.assemblers.ConvDiffAssembler3D(kvs, _geo(iga, 'cylinder'), lambda x, y, z: 2.0 + np.sin(x + z))
        A = asm.assemble_csr(algo='sumfact')
    finally:
        del os.environ['IGX_DEBUG_POISON']
    assert not np.isnan(A.data).any()
    assert np.abs(A @ np.ones(A.shape[1])).max() <= 1e-11 * np.abs(A.data).max()
    rows = np.unique(np.linspace(0, A.shape[0] - 1, 40).astype(int))
    S = iga.assemble.assemble_partial_rows(asm, rows)
    assert np.abs(S[rows].data - A[rows].data).max() <= RTOL * np.abs(A.data).max()


# ---------------------------------------------------------------------------------------------
# general form strings: front-end (pyiga_amd/forms.py) + IGX_FORM kernels
def _form_spaces(iga):
    mk = iga.bspline.make_knots
    return {'cyl_p2': ((mk(2, 0.0, 1.0, 3),) * 3, 'cylinder'),
            'tbox_mixed': ((mk(3, 0.0, 1.0, 2), mk(2, 0.0, 1.0, 4, mult=2), mk(1, 0.0, 1.0, 3)), 'twisted_box')}


@pytest.mark.parametrize('algo', ['sumfact', 'entrywise'])
def test_general_forms_vs_reference(iga, golden, algo, monkeypatch):
    """Form strings through the front-end and both device algorithms, against the matrices the reference
    compiled from the same strings; the same forms given as coefficient tables; multi_entries."""
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')
    g = golden('forms')
    inp = form_inputs()
    tables = form_tables()
    for sname, (kvs, gname) in _form_spaces(iga).items():
        geo = _geo(iga, gname)
        for fname, (form, names) in FORMS.items():
            R = golden_csr(g, '%s_%s' % (sname, fname))
            asm = iga.assemble.instantiate_assembler(form, kvs, dict(geo=geo, **{k: inp[k] for k in names}))
            assert isinstance(asm, iga.assemblers.GeneralFormAssembler3D)
            A = asm.assemble_csr(algo=algo)
            assert asm.patch.timing()['algo_used'] == {'sumfact': 2, 'entrywise': 1}[algo]
            assert A.nnz == R.nnz and np.array_equal(A.indices, R.indices) and not np.isnan(A.data).any()
            assert rel_maxdiff(A, R) <= RTOL, (sname, fname, rel_maxdiff(A, R))
            A2 = iga.assemblers.GeneralFormAssembler3D(kvs, geo, tables[fname]).assemble_csr(algo=algo)
            assert rel_maxdiff(A2, R) <= RTOL
            if algo == 'entrywise':
                rng = np.random.default_rng(5)
                idx = rng.integers(0, R.shape[0], (60, 2)).astype(np.uintp)
                assert np.abs(asm.multi_entries(idx) - np.asarray(R[idx[:, 0], idx[:, 1]]).ravel()).max() <= RTOL * np.abs(R.data).max()
    kv = iga.bspline.make_knots(2, 0.0, 1.0, 3)
    A = iga.assemble.assemble(FORMS['full'][0], (kv, kv, kv), geo=_geo(iga, 'cylinder'), **inp)
    assert rel_maxdiff(A, golden_csr(g, 'cyl_p2_full')) <= RTOL
    for bad in ('u * dx(v) * dx', 'inner(grad(u), grad(u)) * dx', 'u * v', 'inner(grad(u), grad(v)) * u * dx'):
        with pytest.raises(NotImplementedError):
            iga.assemble.assemble(bad, (kv, kv, kv), geo=_geo(iga, 'cylinder'))


def test_general_form_consistency_and_slabs(iga, oracle):
    """The general form reproduces the dedicated kernels (stiffness, mass, convection-diffusion) to rounding,
    matches the oracle at a size with several spans per slab, and row slabs are bit-identical."""
    kvs = (iga.bspline.make_knots(3, 0., 1., 7), iga.bspline.make_knots(2, 0., 1., 8, mult=2), iga.bspline.make_knots(4, 0., 1., 6))
    geo = _geo(iga, 'cylinder')
    G = iga.assemblers.GeneralFormAssembler3D
    K = iga.assemble.stiffness(kvs, geo)
    M = iga.assemble.mass(kvs, geo)
    assert rel_maxdiff(G(kvs, geo, 'inner(grad(u), grad(v)) * dx').assemble_csr(), K) <= RTOL
    assert rel_maxdiff(G(kvs, geo, 'u * v * dx').assemble_csr(), M) <= RTOL
    dc = lambda x, y, z: 1.0 + x
    C = iga.assemblers.ConvDiffAssembler3D(kvs, geo, dc).assemble_csr()
    F = G(kvs, geo, CONVDIFF, inputs=dict(diff_coeff=dc)).assemble_csr()
    assert rel_maxdiff(F, C) <= RTOL
    table = form_tables()['full']
    asm = G(kvs, geo, table)
    A = asm.assemble_csr(algo='sumfact')
    okvs = tuple(oracle.KnotVector(kv.kv, kv.p) for kv in kvs)
    R = oracle.assemble_nonsymmetric('form', okvs, oracle.geo_cylinder(), table=table, nthreads=8)
    assert rel_maxdiff(A, R) <= RTOL and rel_maxdiff(asm.assemble_csr(algo='entrywise'), R) <= RTOL
    N0 = kvs[0].numdofs
    bounds = [0, N0 // 3, 2 * N0 // 3, N0]
    parts = []
    for k in range(3):
        sl = G(kvs, geo, table, row0=(bounds[k], bounds[k + 1]))
        parts.append(sl.assemble_csr(algo='sumfact'))
        sl.patch.close()
    S = scipy.sparse.vstack(parts).tocsr()
    assert np.array_equal(S.indices, A.indices) and np.array_equal(S.data, A.data)


def test_form_tables_on_the_fast_chain(iga, monkeypatch):
    """Round 6: a first-order form given as a string is a coefficient TABLE (constants and expressions) that k_geoA<FORM = 2 | 3>
    evaluates inside the axis-0 sweep -- no field arrays -- and k_bf3 finishes: `geoA` and `bf3` in last_path().  A symmetric
    table takes the symmetric chain (both triangles from the same element matrices: exactly symmetric, `both`).  Checked against
    the entry-wise kernel (the reference's loop nest over fields written by the generated field kernel), against
    a * stiffness + c * mass where the form is that, every value written (NaN poison), row slabs bit for bit; degrees 2 .. 5,
    NURBS and B-spline maps, a map of degree 2 along axis 0, repeated knots on axis 0 and the mid axis.
    (pyiga/vform.py:705-731, pyiga/codegen/cython.py:325-387: the reference generates one kernel per form.)"""
    mk = iga.bspline.make_knots
    g = iga.geometry
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')
    G = iga.assemblers.GeneralFormAssembler3D
    geos = {'cylinder': _geo(iga, 'cylinder'), 'twisted_box': _geo(iga, 'twisted_box'),
            'annulus_x_line': g.tensor_product(g.quarter_annulus(), g.line_segment(0.0, 1.0)),        # degree 2 (NURBS) along axis 0
            'bannulus_x_line': g.tensor_product(g.bspline_quarter_annulus(), g.line_segment(0.0, 1.5, intervals=2))}
    c = lambda x, y, z: 1.0 + x * y + 0.5 * z
    forms = [('(2 * inner(grad(u), grad(v)) + 3 * u * v) * dx', {}, True),
             ('(c * inner(grad(u), grad(v)) + u * v) * dx', {'c': c}, True),
             ('(inner(grad(u), grad(v)) + inner((x[1], -x[0], 1.0), grad(u)) * v) * dx', {}, False),
             ('(c * inner(grad(u), grad(v)) + inner((1.0, c, 2.0), grad(u)) * v + u * inner((0.5, 1.0, c), grad(v)) + 2 * c * u * v) * dx', {'c': c}, False),
             ('(inner(dot(((2.0, 0.5, 0.0), (0.5, 3.0, 0.25), (0.0, 0.25, 1.0)), grad(u)), grad(v))) * dx', {}, True),
             ('c * u * v * dx', {'c': c}, True)]
    cases = [((mk(2, 0., 1., 5), mk(2, 0., 1., 4), mk(2, 0., 1., 6)), 'cylinder'),
             ((mk(3, 0., 1., 4), mk(3, 0., 1., 9), mk(3, 0., 1., 5)), 'annulus_x_line'),
             ((mk(4, 0., 1., 3), mk(4, 0., 1., 4), mk(4, 0., 1., 40)), 'cylinder'),
             ((mk(5, 0., 1., 3), mk(5, 0., 1., 3), mk(5, 0., 1., 4)), 'twisted_box'),
             ((mk(3, 0., 1., 4, mult=2), mk(3, 0., 1., 6, mult=2), mk(3, 0., 1., 7)), 'bannulus_x_line'),
             ((mk(4, 0., 1., 3), mk(3, 0., 1., 6), mk(4, 0., 1., 5)), 'twisted_box'),                  # mid axis one degree below nqp: symmetric tables only
             # repeated knots on the LAST axis: the table goes to the twin patch as it is (physical coefficients), whose chain stores
             # into this patch's layout (test_repeated_knots_on_the_last_axis_through_the_twin)
             ((mk(3, 0., 1., 4), mk(3, 0., 1., 6), mk(3, 0., 1., 5, mult=2)), 'cylinder'),
             ((mk(2, 0., 1., 3), mk(4, 0., 1., 38), mk(4, 0., 1., 4, mult=3)), 'bannulus_x_line')]
    for kvs, gname in cases:
        geo = geos[gname]
        lastmult = kvs[2].numdofs > kvs[2].numspans + kvs[2].p
        for form, inputs, sym in forms:
            asm = G(kvs, geo, form, inputs=inputs)
            assert asm.compiled
            A = asm.assemble_csr(algo='sumfact')
            path = asm.patch.last_path()
            E = asm.assemble_csr(algo='entrywise')
            tag = (form, [kv.p for kv in kvs], gname, sorted(path))
            equal_degrees = len({kv.p for kv in kvs[1:]}) == 1 and kvs[1].p + 1 == max(kv.p for kv in kvs) + 1
            if sym or equal_degrees:
                assert 'geoA' in path and 'bf3' in path, tag
                assert ('both' in path) == sym, tag
                assert ('twin' in path) == lastmult, tag
            assert not np.isnan(A.data).any(), tag
            assert rel_maxdiff(A, E) <= RTOL, (tag, rel_maxdiff(A, E))
            if sym:
                assert abs(A - A.T).max() == 0.0, tag
            N0 = kvs[0].numdofs
            parts = []
            for lo, hi in ((0, N0 // 2), (N0 // 2, N0)):
                sl = G(kvs, geo, form, inputs=inputs, row0=(lo, hi))
                parts.append(sl.assemble_csr(algo='sumfact'))
                sl.patch.close()
            S = scipy.sparse.vstack(parts).tocsr()
            assert np.array_equal(S.indices, A.indices) and np.array_equal(S.data, A.data), tag
            asm.patch.close()
        K, M = iga.assemble.stiffness(kvs, geo), iga.assemble.mass(kvs, geo)
        A = G(kvs, geo, forms[0][0]).assemble_csr()
        assert rel_maxdiff(A, 2 * K + 3 * M) <= RTOL, (gname, rel_maxdiff(A, 2 * K + 3 * M))


def test_arity1_form_strings(iga, golden):
    """Form strings that only contain v assemble a load vector (pyiga/assemble.py:837-897, arity 1;
    test/test_assemble.py:426-429), against vectors from the reference."""
    g = golden('forms')
    mk = iga.bspline.make_knots
    kv2 = (mk(3, 0.0, 1.0, 6), mk(2, 0.0, 1.0, 5))
    ann = _geo(iga, 'quarter_annulus')
    f1 = iga.assemble.assemble('f * v * dx', kv2, geo=ann, f=lambda x, y: x * y ** 2)
    assert _close(f1, g['func_d2'])
    assert _close(f1, iga.assemble.inner_products(kv2, lambda x, y: x * y ** 2, geo=ann, f_physical=True), 1e-15)
    kv = mk(2, 0.0, 1.0, 3)
    f3 = iga.assemble.assemble('(2 * f + x[0]) * v * dx', (kv, kv, kv), geo=_geo(iga, 'cylinder'),
                               f=lambda x, y, z: np.cos(x) * np.exp(y) * np.sin(z))
    assert _close(f3, g['func_d3'])
    # derivatives of v in the functional
    inp = form_inputs()
    b2 = form2d_cases()['full'][1]['b']
    fg2 = iga.assemble.assemble('(f * v + inner(b, grad(v))) * dx', kv2, geo=ann, f=lambda x, y: x * y ** 2, b=b2)
    assert _close(fg2, g['funcgrad_d2'])
    kvm = (mk(3, 0.0, 1.0, 2), mk(2, 0.0, 1.0, 4, mult=2), mk(1, 0.0, 1.0, 3))
    fg3 = iga.assemble.assemble('inner(b, grad(v)) * dx', kvm, geo=_geo(iga, 'twisted_box'), b=inp['b'])
    assert _close(fg3, g['funcgrad_d3'])
    # divergence theorem on the unit cube: integral of grad(v).e_x = v(1,.,.) - v(0,.,.) integrated over the face -> sums to 0 over
    # interior functions, and the whole vector sums to 0 because the basis is a partition of unity
    fz = iga.assemble.assemble('inner((1.0, 2.0, -3.0), grad(v)) * dx', (kv, kv, kv), geo=iga.geometry.unit_cube())
    assert abs(fz.sum()) <= 1e-13
    # slabs reproduce their rows bit for bit
    from pyiga_amd import forms
    full = iga.assemblers.GeneralFunctionalAssembler3D(kvm, _geo(iga, 'twisted_box'), 'inner(b, grad(v)) * dx', inputs=dict(b=inp['b']))
    parts = []
    N0 = kvm[0].numdofs
    for lo, hi in ((0, 2), (2, N0)):
        sl = iga.assemblers.GeneralFunctionalAssembler3D(kvm, _geo(iga, 'twisted_box'), 'inner(b, grad(v)) * dx', inputs=dict(b=inp['b']), row0=(lo, hi))
        parts.append(sl.assemble_vector())
    assert np.array_equal(np.concatenate(parts, axis=0), full.assemble_vector())


@pytest.mark.parametrize('d', [2, 3])
def test_tiny_and_odd_sizes(iga, d, monkeypatch):
    """Corner sizes of the sum-factorised kernels (one span, fewer rows than a wave chunk, row counts that
    are not a multiple of the chunk, degree 1, mixed degrees): sum-factorised == entry-wise, all written."""
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')
    mk = iga.bspline.make_knots
    geo = _geo(iga, 'quarter_annulus' if d == 2 else 'cylinder')
    cases = [(1, 1), (1, 2), (2, 1), (3, 1), (5, 1), (2, 2), (4, 2), (1, 13), (3, 23), (5, 11)]
    if d == 3:
        cases = [(1, 1), (2, 1), (4, 1), (5, 2), (1, 9), (3, 13), (5, 7)]
    for p, n in cases:
        kvs = tuple(mk(max(1, p - (k == 1)), 0., 1., n + k) for k in range(d))
        for kind in ('mass', 'stiffness'):
            patch = iga.assemblers.DevicePatch(kvs, geo)
            A = patch.csr(kind, algo='sumfact')
            E = patch.csr(kind, algo='entrywise')
            patch.close()
            assert not np.isnan(A.data).any(), (p, n, kind)
            assert rel_maxdiff(A, E) <= RTOL, (p, n, kind, rel_maxdiff(A, E))
            assert abs(A - A.T).max() == 0.0


def test_geometry_mesh_finer_than_space(iga, monkeypatch):
    """A geometry map with many more knot spans than the space (Gauss points of ONE element fall into several geometry
    spans): the single-launch 2D kernel sizes its control-net window by the geometry knots under a tile's Gauss window, the
    line kernels by the whole line.  Every path against the entry-wise kernel, which evaluates the map point by point."""
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')
    mk = iga.bspline.make_knots
    gk = (mk(2, 0.0, 1.0, 37), mk(3, 0.0, 1.0, 41))
    t0, t1 = (np.array([k.kv[i + 1:i + 1 + k.p].mean() for i in range(k.numdofs)]) for k in gk)      # Greville abscissae
    X, Y = np.meshgrid(t1, t0)                          # last component axis: (x, y); x runs with the LAST grid axis
    coeffs = np.stack([X + 0.07 * np.sin(3 * Y) * np.cos(2 * X), Y + 0.05 * np.sin(4 * X + Y)], axis=-1)
    geo = iga.bspline.BSplineFunc(gk, coeffs)
    for p, n in ((3, (9, 7)), (2, (23, 5)), (1, (4, 30))):
        kvs = (mk(p, 0.0, 1.0, n[0]), mk(p, 0.0, 1.0, n[1]))
        for kind in ('mass', 'stiffness'):
            ref = None
            for path in ('', 'single', 'unfused'):
                if path:
                    monkeypatch.setenv('IGX_PATH', path)
                else:
                    monkeypatch.delenv('IGX_PATH', raising=False)
                patch = iga.assemblers.DevicePatch(kvs, geo)
                if ref is None:
                    ref = patch.csr(kind, algo='entrywise')
                A = patch.csr(kind, algo='sumfact')
                if path == 'single':
                    assert patch.last_path() == {'single'}
                patch.close()
                assert not np.isnan(A.data).any(), (p, n, kind, path)
                assert rel_maxdiff(A, ref) <= RTOL, (p, n, kind, path, rel_maxdiff(A, ref))
                assert abs(A - A.T).max() == 0.0


def test_multi_entries_edge_inputs(iga):
    """multi_entries (pyiga/genericasm.pxi:722-758) with the inputs a caller may hand over: no pairs at all, an iterable of
    tuples instead of an array, a non-contiguous view, pairs outside the pattern (exact 0.0, the reference's zero-initialised
    output) and repeated pairs."""
    mk = iga.bspline.make_knots
    for kvs, geo, cls in (((mk(3, 0., 1., 6), mk(2, 0., 1., 5)), iga.geometry.quarter_annulus(), iga.assemblers.StiffnessAssembler2D),
                          ((mk(2, 0., 1., 4),) * 3, _geo(iga, 'twisted_box'), iga.assemblers.MassAssembler3D)):
        asm = cls(kvs, geo)
        A = asm.assemble_csr()
        n = A.shape[0]
        out = asm.multi_entries(np.zeros((0, 2), dtype=np.uintp))
        assert isinstance(out, np.ndarray) and out.shape == (0,) and out.dtype == np.float64
        assert asm.multi_entries([]).shape == (0,)
        pairs = [(0, 0), (n - 1, n - 1), (0, n - 1), (n - 1, 0), (3, 4), (3, 4), (4, 3)]
        want = np.array([A[i, j] for i, j in pairs])
        assert want[2] == 0.0 and want[3] == 0.0
        got_list = asm.multi_entries(iter(pairs))
        big = np.zeros((len(pairs), 4), dtype=np.uintp)
        big[:, ::2] = pairs
        got_view = asm.multi_entries(big[:, ::2])
        for got in (got_list, got_view):
            assert got.shape == (len(pairs),)
            assert got[2] == 0.0 and got[3] == 0.0 and got[4] == got[5]
            assert np.abs(got - want).max() <= RTOL * abs(A).max()
        assert abs(asm.entry(3, 4) - want[4]) <= RTOL * abs(A).max()


def test_general_forms_2d(iga, golden):
    """2D form strings (entry-wise kernel) against the reference's compiled assemblers; the general form
    against the dedicated 2D stiffness / mass kernels; multi_entries."""
    g = golden('forms')
    mk = iga.bspline.make_knots
    kvs = (mk(3, 0.0, 1.0, 4), mk(2, 0.0, 1.0, 5, mult=2))
    ann = _geo(iga, 'quarter_annulus')
    for fname, (form, inputs, table) in form2d_cases().items():
        R = golden_csr(g, 'd2_%s' % fname)
        A = iga.assemble.assemble(form, kvs, geo=ann, **inputs)
        assert A.nnz == R.nnz and np.array_equal(A.indices, R.indices)
        assert rel_maxdiff(A, R) <= RTOL, (fname, rel_maxdiff(A, R))
        asm = iga.assemblers.GeneralFormAssembler2D(kvs, ann, table)
        for algo, code in (('sumfact', 2), ('entrywise', 1), ('auto', 2)):
            B = asm.assemble_csr(algo=algo)
            assert asm.patch.timing()['algo_used'] == code
            assert rel_maxdiff(B, R) <= RTOL, (fname, algo, rel_maxdiff(B, R))
        idx = np.random.default_rng(2).integers(0, R.shape[0], (40, 2)).astype(np.uintp)
        assert np.abs(asm.multi_entries(idx) - np.asarray(R[idx[:, 0], idx[:, 1]]).ravel()).max() <= RTOL * np.abs(R.data).max()
    kv = (mk(3, 0.0, 1.0, 9), mk(4, 0.0, 1.0, 7))
    G2 = iga.assemblers.GeneralFormAssembler2D
    assert rel_maxdiff(G2(kv, ann, 'inner(grad(u), grad(v)) * dx').assemble_csr(), iga.assemble.stiffness(kv, ann)) <= RTOL
    assert rel_maxdiff(G2(kv, ann, '2 * u * v * dx').assemble_csr(), 2 * iga.assemble.mass(kv, ann)) <= RTOL
    # larger, non-uniform knots, slabs: sum-factorised == entry-wise, rows bit-identical
    kvl = (mk(3, 0.0, 1.0, 37), mk(2, 0.0, 1.0, 23, mult=2))
    form, inputs, _ = form2d_cases()['full']
    full = G2(kvl, ann, form, inputs=inputs)
    A = full.assemble_csr(algo='sumfact')
    assert rel_maxdiff(A, full.assemble_csr(algo='entrywise')) <= RTOL
    N0 = kvl[0].numdofs
    parts = []
    for lo, hi in ((0, N0 // 2), (N0 // 2, N0)):
        sl = G2(kvl, ann, form, inputs=inputs, row0=(lo, hi))
        parts.append(sl.assemble_csr(algo='sumfact'))
    S = scipy.sparse.vstack(parts).tocsr()
    assert np.array_equal(S.indices, A.indices) and np.array_equal(S.data, A.data)


# ---------------------------------------------------------------------------------------------
# BASELINE.json's full sizes, through size-independent properties
def _axis_ranges(kv):
    """per dof: first column, number of columns, exclusive prefix sum (the 1D pattern of a knot vector)."""
    s = kv.mesh_support_idx_all()
    first = np.searchsorted(s[:, 1], s[:, 0], side='right')
    last = np.searchsorted(s[:, 0], s[:, 1], side='left')
    c = (last - first).astype(np.int64)
    return first.astype(np.int64), c, np.concatenate(([0], np.cumsum(c)))


def _positions(kvs, I, J):
    """CSR position of entry (I, J) from the per-axis tables, for arrays of ravelled indices."""
    nd = tuple(kv.numdofs for kv in kvs)
    mi, mj = np.unravel_index(I, nd), np.unravel_index(J, nd)
    ax = [_axis_ranges(kv) for kv in kvs]
    S = [a[2][-1] for a in ax]
    # indptr(I) = rp0*S1*S2 + c0*(rp1*S2 + c1*rp2); offset = ((j0-jlo0)*c1 + (j1-jlo1))*c2 + (j2-jlo2)
    ind = np.zeros_like(I)
    cprod = np.ones_like(I)
    for k in range(len(kvs)):
        rest = int(np.prod(S[k + 1:])) if k + 1 < len(kvs) else 1
        ind = ind + cprod * ax[k][2][mi[k]] * rest
        cprod = cprod * ax[k][1][mi[k]]
    off = np.zeros_like(I)
    for k in range(len(kvs)):
        off = off * ax[k][1][mi[k]] + (mj[k] - ax[k][0][mi[k]])
    return ind + off, ind


def test_full_size_c3(iga, monkeypatch):
    """BASELINE config 3 at full size (3D p=2 n=64, 34 M nonzeros): mass + stiffness."""
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')
    kv = iga.bspline.make_knots(2, 0., 1., 64)
    geo = _geo(iga, 'cylinder')
    K = iga.assemble.stiffness((kv,) * 3, geo)
    M = iga.assemble.mass((kv,) * 3, geo)
    assert K.nnz == 34012224 and not np.isnan(K.data).any() and not np.isnan(M.data).any()
    assert abs(K - K.T).max() == 0.0 and abs(M - M.T).max() == 0.0
    assert np.abs(K @ np.ones(K.shape[0])).max() <= 1e-11 * abs(K).max()
    assert abs(M.sum() - 0.75 * np.pi) < 1e-9


def test_full_size_c4(iga, oracle, monkeypatch):
    """BASELINE config 4 at full size (3D p=4, 128^3 spans, 1.59 G nonzeros), memory-light: the values come
    back without the index arrays; row sums vanish (K 1 = 0), sampled rows agree with the entry-wise kernel,
    sampled entry pairs are exactly symmetric, nothing is left unwritten."""
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')
    kv = iga.bspline.make_knots(4, 0., 1., 128)
    kvs = (kv, kv, kv)
    asm = iga.assemblers.StiffnessAssembler3D(kvs, _geo(iga, 'cylinder'))
    assert asm.patch.nnz == 1593413632
    data = asm.patch.assemble('stiffness', algo='sumfact', to_host=True)
    assert asm.patch.timing()['algo_used'] == 2
    assert not np.isnan(data).any()
    n = asm.patch.shape[0]
    rows = np.arange(n, dtype=np.int64)
    _, indptr = _positions(kvs, rows, rows)
    assert indptr[0] == 0 and np.all(np.diff(indptr) > 0)
    scale = np.abs(data).max()
    rowsum = np.add.reduceat(data, indptr)
    assert np.abs(rowsum).max() <= 1e-10 * scale
    rng = np.random.default_rng(7)
    N = kv.numdofs
    line = np.arange(N) + (71 * N + 40) * N                       # every row of one line of the last axis: all tile positions
    sample = np.unique(np.concatenate(([0, n - 1, n // 2], line, rng.integers(0, n, 40))))
    S = iga.assemble.assemble_partial_rows(asm, sample)          # entry-wise kernel, ~175 rows
    for r in sample:
        lo = indptr[r]
        ref = S.data[S.indptr[r]:S.indptr[r + 1]]
        assert np.abs(data[lo:lo + ref.size] - ref).max() <= RTOL * scale
        cols = S.indices[S.indptr[r]:S.indptr[r + 1]].astype(np.int64)
        pos_t, _ = _positions(kvs, cols, np.full_like(cols, r))
        assert np.array_equal(data[pos_t], data[lo:lo + ref.size])      # A[J, I] == A[I, J] bit for bit
    # ... and against the CPU oracle at THIS size: the reference's entry sums with the fields evaluated on each pair's support
    # intersection only (oracle.local_entries; bit-identical to the oracle assembler that the reference goldens pin)
    okv = oracle.make_knots(4, 0., 1., 128)
    def picks(r):
        cols = S.indices[S.indptr[r]:S.indptr[r + 1]]
        return np.stack([np.full(3, r), cols[[0, cols.size // 2, -1]]], 1)
    # every row of one line of the last axis (all positions inside all tiles of the fused stage: one whole tile column of
    # k_bf3, the default; k_bf2 has tests/test_bf2_kernels_gpu.py), three entries each, and every entry of one interior row
    full_row = int(line[57])
    fr_cols = S.indices[S.indptr[full_row]:S.indptr[full_row + 1]]
    pr = np.concatenate([picks(r) for r in sample[::6]] + [picks(r) for r in line] + [np.stack([np.full(fr_cols.size, full_row), fr_cols], 1)])
    ref = oracle.local_entries('stiffness', (okv,) * 3, oracle.geo_cylinder(), pr)
    pos, _ = _positions(kvs, pr[:, 0].astype(np.int64), pr[:, 1].astype(np.int64))
    assert np.abs(data[pos] - ref).max() <= RTOL * scale
    # ... and the work-balanced row slabs of the 8-GPU split reproduce their rows of this matrix bit for bit (first, an inner and
    # the last slab: what every rank of `bench.py --gpus 8` computes)
    asm.patch.close()
    for r in (0, 3, 7):
        lo, hi = iga.distributed.slab_range(N, r, 8, 4)
        sl = iga.assemblers.DevicePatch(kvs, _geo(iga, 'cylinder'), row0=(lo, hi))
        part = sl.assemble('stiffness', algo='sumfact', to_host=True)
        a, b = indptr[lo * N * N], (indptr[hi * N * N] if hi < N else data.size)
        assert part.size == b - a and np.array_equal(part, data[a:b]), r
        sl.close()


def test_full_size_c4_every_entry(iga):
    """BASELINE config 4 at full size, EVERY one of the 1.59 G entries: the sum-factorised chain (k_geoA + k_bf3) against the
    entry-wise kernels -- the reference's loop nest (pyiga/assemblers.pyx:1455-1540) with its own summation order, the second,
    independent device implementation that the oracle pins at the sizes it reaches -- compared in chunks on the host."""
    kv = iga.bspline.make_knots(4, 0., 1., 128)
    asm = iga.assemblers.StiffnessAssembler3D((kv, kv, kv), _geo(iga, 'cylinder'))
    data = asm.patch.assemble('stiffness', algo='sumfact', to_host=True)
    assert asm.patch.timing()['algo_used'] == 2 and data.size == 1593413632
    ref = asm.patch.assemble('stiffness', algo='entrywise', to_host=True)
    assert asm.patch.timing()['algo_used'] == 1 and ref.size == data.size
    scale = float(np.abs(ref[::997]).max())
    worst = 0.0
    step = 1 << 26
    for a in range(0, data.size, step):
        worst = max(worst, float(np.abs(data[a:a + step] - ref[a:a + step]).max()))
    assert worst <= RTOL * scale, worst / scale
    # ... and the chain is reproducible run to run, bit for bit (fixed summation order: the only LDS adds have two addends)
    del ref
    again = asm.patch.assemble('stiffness', algo='sumfact', to_host=True)
    for a in range(0, data.size, step):
        assert np.array_equal(data[a:a + step], again[a:a + step])
    asm.patch.close()


def test_full_size_c4_with_repeated_knots_on_the_last_axis_every_entry(iga):
    """C4's patch with double interior knots on the LAST axis (bench.py --config c4l: 128 x 128 x 64 spans, 1.41 G entries) at
    full size: the twin route (k_geoA + k_bf3 on the patch with mid and last axis exchanged, values stored into this patch's CSR
    layout: fused3.hip TR -- 32-bit offsets, 24-bit row constants) against the entry-wise kernels, EVERY entry; exactly the
    path and size the bench line of that config measures."""
    kv = iga.bspline.make_knots(4, 0., 1., 128)
    kvl = iga.bspline.make_knots(4, 0., 1., 64, mult=2)
    patch = iga.assemblers.DevicePatch((kv, kv, kvl), _geo(iga, 'cylinder'))
    data = patch.assemble('stiffness', algo='sumfact', to_host=True)
    assert patch.last_path() == {'geoA', 'fused', 'both', 'bf3', 'twin'} and data.size == 1409243392
    ref = patch.assemble('stiffness', algo='entrywise', to_host=True)
    assert patch.timing()['algo_used'] == 1 and ref.size == data.size
    patch.close()
    scale = float(np.abs(ref[::997]).max())
    worst = 0.0
    step = 1 << 26
    for a in range(0, data.size, step):
        worst = max(worst, float(np.abs(data[a:a + step] - ref[a:a + step]).max()))
    assert worst <= RTOL * scale, worst / scale


def test_fast_variants_match_fixtures(iga, capsys):
    """test/test_assemble.py:187-217 (test_fast_{mass,stiffness}_geo_{2,3}d): the low-rank (ACA) assemblers against the
    bundled fixtures with the reference's tolerance 1e-9; the approximation really is low-rank (few crosses, fewer entries
    evaluated than the matrix has where the matrix is large enough)."""
    kv = iga.bspline.make_knots(3, 0.0, 1.0, 15)
    geo = iga.geometry.bspline_quarter_annulus()
    M_ref = iga.utils.read_sparse_matrix(os.path.join(GOLDEN, 'poisson_neu_d2_p3_n15_mass.mtx.gz'))
    A_ref = iga.utils.read_sparse_matrix(os.path.join(GOLDEN, 'poisson_neu_d2_p3_n15_stiff.mtx.gz'))
    assert abs(iga.assemble.mass_fast((kv, kv), geo, verbose=0) - M_ref).max() < 1e-9
    assert abs(iga.assemble.stiffness_fast((kv, kv), geo, verbose=0) - A_ref).max() < 1e-9
    assert abs(iga.assemble.mass_fast((kv, kv)) - iga.assemble.mass((kv, kv))).max() == 0.0     # no geometry: Kronecker path
    kv3 = iga.bspline.make_knots(2, 0.0, 1.0, 10)
    box = iga.geometry.twisted_box()
    M3_ref = iga.utils.read_sparse_matrix(os.path.join(GOLDEN, 'poisson_neu_d3_p2_n10_mass.mtx.gz'))
    A3_ref = iga.utils.read_sparse_matrix(os.path.join(GOLDEN, 'poisson_neu_d3_p2_n10_stiff.mtx.gz'))
    assert abs(iga.assemble.mass_fast((kv3,) * 3, box, verbose=0) - M3_ref).max() < 1e-9
    assert abs(iga.assemble.stiffness_fast((kv3,) * 3, box, verbose=0) - A3_ref).max() < 1e-9
    # statistics, a looser tolerance, and the progress lines of the reference
    kvb = iga.bspline.make_knots(3, 0.0, 1.0, 40)
    patch = iga.assemblers.DevicePatch((kvb, kvb), iga.geometry.quarter_annulus())
    exact = patch.csr('stiffness')
    A = patch.fast_assemble('stiffness')
    st = patch.aca_stats
    assert abs(A - exact).max() < 1e-9 and 0 < st['rank'] <= 40 and st['entries'] < st['nnz']
    patch.close()                                   # (the annulus is exactly rank 3 in this ordering)
    patch = iga.assemblers.DevicePatch((kv3,) * 3, box)
    exact = patch.csr('stiffness')
    A = patch.fast_assemble('stiffness')
    st = patch.aca_stats
    assert abs(A - exact).max() < 1e-9 and st['entries'] < st['nnz']
    # request granularity: by default a small slice is ONE request (index pairs generated on the device); batch=0 is the
    # reference's access pattern (slices approximated line by line) -- same tolerance, many more launches
    assert st['requests'] < 150, st
    A0 = patch.fast_assemble('stiffness', batch=0)
    st0 = patch.aca_stats
    assert abs(A0 - exact).max() < 1e-9 and st0['requests'] > 2 * st['requests'] and st0['entries'] < st['nnz']
    assert abs(A0 - A3_ref).max() < 1e-9
    B = patch.fast_assemble('stiffness', tol=1e-4, batch=65536)
    assert patch.aca_stats['rank'] < st['rank'] and 1e-12 < abs(B - exact).max() < 1e-2
    capsys.readouterr()
    patch.close()
    # 2D fixture through the line-by-line pattern as well (the default fetches this small matrix in one request, exactly)
    patch = iga.assemblers.DevicePatch((kv, kv), geo)
    assert abs(patch.fast_assemble('stiffness', batch=0) - A_ref).max() < 1e-9 and patch.aca_stats['rank'] > 0
    assert abs(patch.fast_assemble('mass', batch=65536) - M_ref).max() < 1e-14 and patch.aca_stats['requests'] == 1
    patch.close()
    with pytest.raises(AssertionError):
        iga.assemblers.DevicePatch((kvb, kvb), iga.geometry.quarter_annulus(), row0=(0, 10)).fast_assemble('mass')


def test_full_size_c5(iga, monkeypatch):
    """BASELINE config 5 at full size (3D p=5 n=96 convection-diffusion form, 1.26 G nonzeros), memory-light:
    every row sums to zero (a(1, v) = 0), sampled rows agree with the entry-wise kernel, nothing unwritten."""
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')
    kv = iga.bspline.make_knots(5, 0., 1., 96)
    kvs = (kv, kv, kv)
    asm = iga.assemblers.ConvDiffAssembler3D(kvs, _geo(iga, 'cylinder'), lambda x, y, z: 1.0 + x)
    assert asm.patch.nnz == 1263214441
    data = asm.patch.assemble('convdiff', algo='sumfact', to_host=True)
    assert asm.patch.timing()['algo_used'] == 2 and not np.isnan(data).any()
    n = asm.patch.shape[0]
    rows = np.arange(n, dtype=np.int64)
    _, indptr = _positions(kvs, rows, rows)
    scale = np.abs(data).max()
    assert np.abs(np.add.reduceat(data, indptr)).max() <= 1e-10 * scale
    sample = np.unique(np.concatenate(([0, n - 1], np.random.default_rng(11).integers(0, n, 12))))
    S = iga.assemble.assemble_partial_rows(asm, sample)
    for r in sample:
        ref = S.data[S.indptr[r]:S.indptr[r + 1]]
        assert np.abs(data[indptr[r]:indptr[r] + ref.size] - ref).max() <= RTOL * scale


def test_full_size_c5_every_entry_of_a_slab(iga):
    """BASELINE config 5 at full size, EVERY entry of sixteen dof planes (2.0e8 of the 1.26 G entries of the non-symmetric
    convection-diffusion matrix; the coefficient as bench.py passes it, evaluated on the device): sum-factorised chain against
    the entry-wise kernels.  (The whole matrix takes the entry-wise kernels 140 s at p = 5; it was compared once, in round 5,
    with this tolerance: passed.)"""
    kv = iga.bspline.make_knots(5, 0., 1., 96)
    asm = iga.assemblers.ConvDiffAssembler3D((kv, kv, kv), _geo(iga, 'cylinder'), iga.assemblers.AffineCoefficient(1.0, 1.0), row0=(43, 59))
    data = asm.patch.assemble('convdiff', algo='sumfact', to_host=True)
    assert asm.patch.timing()['algo_used'] == 2 and 'bf3' in asm.patch.last_path() and data.size == asm.patch.nnz > 1.9e8
    ref = asm.patch.assemble('convdiff', algo='entrywise', to_host=True)
    assert asm.patch.timing()['algo_used'] == 1 and ref.size == data.size
    scale = float(np.abs(ref).max())
    assert float(np.abs(data - ref).max()) <= RTOL * scale
    asm.patch.close()


def test_full_size_c5_affine_coefficient(iga, golden, oracle, monkeypatch):
    """The coefficient of BASELINE config 5 as bench.py passes it -- AffineCoefficient(1, 1): 1 + x evaluated ON THE DEVICE
    through the geometry map -- pinned (i) at p=5 n=24 to the reference's matrix (golden_fullsize p5n24_convdiff, made with
    the host-sampled lambda) and (ii) at full size to the host-sampled lambda on sampled rows and through the row sums."""
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')
    geo = _geo(iga, 'cylinder')
    g = golden('fullsize')
    kv = iga.bspline.make_knots(5, 0., 1., 24)
    A = iga.assemblers.ConvDiffAssembler3D((kv,) * 3, geo, iga.assemblers.AffineCoefficient(1.0, 1.0)).assemble_csr()
    assert np.abs(_csr_at(A, g['p5n24_idx']) - g['p5n24_convdiff']).max() <= RTOL * abs(A).max()
    del A
    kv = iga.bspline.make_knots(5, 0., 1., 96)
    kvs = (kv, kv, kv)
    aff = iga.assemblers.ConvDiffAssembler3D(kvs, geo, iga.assemblers.AffineCoefficient(1.0, 1.0))
    data = aff.patch.assemble('convdiff', algo='sumfact', to_host=True)
    assert 'fused' in aff.patch.last_path() and not np.isnan(data).any()
    n = aff.patch.shape[0]
    _, indptr = _positions(kvs, np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64))
    scale = np.abs(data).max()
    assert np.abs(np.add.reduceat(data, indptr)).max() <= 1e-10 * scale
    aff.patch.close()
    lam = iga.assemblers.ConvDiffAssembler3D(kvs, geo, lambda x, y, z: 1.0 + x)
    N = kv.numdofs
    # rows of one line of the last axis (every position inside the tiles of the fused stage) + scattered rows
    sample = np.unique(np.concatenate((np.arange(N) + (37 * N + 53) * N, np.random.default_rng(3).integers(0, n, 10))))
    S = iga.assemble.assemble_partial_rows(lam, sample)          # host-sampled coefficient, entry-wise kernel
    for r in sample:
        ref = S.data[S.indptr[r]:S.indptr[r + 1]]
        assert np.abs(data[indptr[r]:indptr[r] + ref.size] - ref).max() <= RTOL * scale
    # (iii) against the CPU oracle at THIS size (oracle.local_entries: the reference's entry sums, fields on the support
    # intersection of each pair only)
    okv = oracle.make_knots(5, 0., 1., 96)
    pr = []
    for r in sample[::8]:
        cols = S.indices[S.indptr[r]:S.indptr[r + 1]]
        pr.append(np.stack([np.full(3, r), cols[[0, cols.size // 2, -1]]], 1))
    pr = np.concatenate(pr)
    ref = oracle.local_entries('convdiff', (okv,) * 3, oracle.geo_cylinder(), pr, coeff=lambda x, y, z: 1.0 + x)
    pos, _ = _positions(kvs, pr[:, 0].astype(np.int64), pr[:, 1].astype(np.int64))
    assert np.abs(data[pos] - ref).max() <= RTOL * scale


def test_repeatability(iga):
    """Race hunt: the final stage waits on its LDS-DMA queue with counted vmcnt and exchanges sums between waves
    through LDS; the halves of a pass of the fused stage ADD into the entry rings (ds_add_f64, two addends: the order must
    not matter); an under-wait or an order dependence would show up as run-to-run differences.  40 repetitions,
    bit-identical values (tools/rowsum_check.py repeats the full C4 size)."""
    import hashlib
    mk = iga.bspline.make_knots
    for kvs, gname, kind in (((mk(4, 0., 1., 14),) * 3, 'cylinder', 'stiffness'),
                             ((mk(2, 0., 1., 30), mk(3, 0., 1., 11), mk(2, 0., 1., 19)), 'twisted_box', 'mass'),
                             ((mk(3, 0., 1., 200), mk(3, 0., 1., 150)), 'quarter_annulus', 'stiffness')):
        patch = iga.assemblers.DevicePatch(kvs, _geo(iga, gname))
        hashes = {hashlib.sha1(patch.assemble(kind, algo='sumfact', to_host=True).tobytes()).hexdigest() for _ in range(40)}
        patch.close()
        assert len(hashes) == 1


def test_both_triangles_from_the_fused_stage(iga, monkeypatch):
    """k_bf3 (fused3.hip) writes the upper triangle of a symmetric 3D form from the same element matrices as the lower one,
    in the same order of addends: the matrix is the one of k_bf2 + mirror pass (IGX_BF=2) BIT FOR BIT, exactly symmetric, every
    value written (NaN poison), for every degree the fused stage is compiled for -- including axes shorter than 2p + 1 dofs
    (every row is an edge row) and unequal sizes per axis.  (pyiga/assemble.py:742-752: assemble_entries(symmetric=True).)"""
    mk = iga.bspline.make_knots
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')
    cases = [((mk(4, 0., 1., 3),) * 3, 'cylinder'), ((mk(4, 0., 1., 9),) * 3, 'cylinder'), ((mk(1, 0., 1., 5),) * 3, 'twisted_box'),
             ((mk(2, 0., 1., 4), mk(2, 0., 1., 11), mk(2, 0., 1., 7)), 'cylinder'), ((mk(3, 0., 1., 6), mk(3, 0., 1., 5), mk(3, 0., 1., 13)), 'twisted_box'),
             ((mk(5, 0., 1., 7), mk(5, 0., 1., 6), mk(5, 0., 1., 8)), 'cylinder'), ((mk(4, 0., 1., 5), mk(4, 0., 1., 40), mk(4, 0., 1., 36)), 'cylinder')]
    for kvs, gname in cases:
        for kind in ('stiffness', 'mass'):
            out = {}
            for bf in ('', '2'):
                if bf:
                    monkeypatch.setenv('IGX_BF', bf)
                else:
                    monkeypatch.delenv('IGX_BF', raising=False)
                patch = iga.assemblers.DevicePatch(kvs, _geo(iga, gname))
                A = patch.csr(kind, algo='sumfact')
                assert patch.last_path() == ({'geoA', 'fused', 'mirror'} if bf else {'geoA', 'fused', 'both', 'bf3'}), (kind, bf, patch.last_path())
                patch.close()
                assert not np.isnan(A.data).any()
                assert abs(A - A.T).max() == 0.0
                out[bf] = A.data
            if kind == 'stiffness':
                assert np.array_equal(out[''], out['2']), (kind, [kv.numdofs for kv in kvs])
            else:
                # round 6: the mass form goes through its per-axis symmetry (k_bf3<SYM = 3>: every block contracted like a diagonal
                # one, a finished row stored to both row blocks) -- the upper lines of an off-diagonal block are no longer swept
                # separately, so the two chains agree to rounding, not bit for bit
                assert np.abs(out[''] - out['2']).max() <= 1e-14 * np.abs(out['2']).max(), (kind, [kv.numdofs for kv in kvs])
    monkeypatch.delenv('IGX_BF', raising=False)


def test_repeated_knots_on_the_last_axis_through_the_twin(iga, monkeypatch):
    """Round 6: k_bf3 contracts an axis of single knots, so a patch whose LAST axis has repeated knots (and
    whose mid axis has not) is assembled through its twin -- mid and last axis exchanged, knot vectors and control net -- whose
    k_bf3 stores into the CSR layout of the caller's patch (fused3.hip, TR; igx_patch::twin).  Mass and stiffness, degrees 2-5 on
    the two axes (any lower degree on axis 0), knots of multiplicity 2 .. p, several tiles of the twin's last axis, NURBS and
    B-spline geometry, row slabs: against the entry-wise kernels (the reference's loop nest, pyiga/assemblers.pyx:1455-1540) and the
    stage kernels (IGX_NO_TWIN: the path such patches took before), exactly symmetric, every value written, slabs bit for bit."""
    mk = iga.bspline.make_knots
    KV = iga.bspline.KnotVector
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')

    def kv_mults(p, mults):
        n = len(mults) + 1
        inner = np.repeat(np.arange(1, n) / n, mults)
        return KV(np.concatenate([np.zeros(p + 1), inner, np.ones(p + 1)]), p)
    cases = [((mk(3, 0., 1., 3), mk(3, 0., 1., 4), mk(3, 0., 1., 5, mult=2)), 'cylinder'),
             ((mk(2, 0., 1., 4), mk(2, 0., 1., 45), mk(2, 0., 1., 6, mult=2)), 'twisted_box'),          # 47 rows: two tiles of the twin's last axis
             ((mk(4, 0., 1., 3), mk(4, 0., 1., 38), kv_mults(4, [1, 2, 4, 1, 3])), 'cylinder'),          # mixed multiplicities, C^0 knot
             ((mk(1, 0., 1., 5), mk(1, 0., 1., 6), mk(1, 0., 1., 4)), 'twisted_box'),                    # (degree 1: nothing to repeat -> no twin)
             ((mk(2, 0., 1., 3), mk(4, 0., 1., 5), kv_mults(4, [2, 2, 1])), 'twisted_box'),              # lower degree on axis 0
             ((mk(5, 0., 1., 3), mk(5, 0., 1., 4), mk(5, 0., 1., 3, mult=3)), 'cylinder'),               # degree 5
             ((mk(3, 0., 1., 4), mk(3, 0., 1., 5), mk(4, 0., 1., 4, mult=2)), 'cylinder'),               # unequal degrees on the two axes: stage kernels
             ((mk(3, 0., 1., 6, mult=2), mk(3, 0., 1., 7), kv_mults(3, [3, 1, 2, 2])), 'cylinder')]      # repeated knots on axis 0 as well
    for kvs, gname in cases:
        geo = _geo(iga, gname)
        twin = kvs[1].p == kvs[2].p and 2 <= kvs[2].p <= 5 and kvs[0].p <= kvs[1].p
        for kind in ('stiffness', 'mass'):
            patch = iga.assemblers.DevicePatch(kvs, geo)
            A = patch.csr(kind, algo='sumfact')
            path = patch.last_path()
            E = patch.csr(kind, algo='entrywise')
            patch.close()
            assert ('twin' in path) == twin, (kind, path, [kv.p for kv in kvs])
            if twin:
                assert path == {'geoA', 'fused', 'both', 'bf3', 'twin'}, path
            assert not np.isnan(A.data).any()
            assert abs(A - A.T).max() == 0.0
            assert np.array_equal(A.indptr, E.indptr) and np.array_equal(A.indices, E.indices)
            assert rel_maxdiff(A, E) <= RTOL, (kind, [kv.numdofs for kv in kvs], rel_maxdiff(A, E))
            if not twin:
                continue
            monkeypatch.setenv('IGX_NO_TWIN', '1')
            patch = iga.assemblers.DevicePatch(kvs, geo)
            S = patch.csr(kind, algo='sumfact')
            assert 'twin' not in patch.last_path() and 'bf3' not in patch.last_path()
            patch.close()
            monkeypatch.delenv('IGX_NO_TWIN')
            assert rel_maxdiff(A, S) <= 1e-13
            # row slabs of axis 0: the rows of the whole patch, bit for bit
            N0 = kvs[0].numdofs
            cuts = [0, 1, N0 // 2, N0]
            parts = []
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                patch = iga.assemblers.DevicePatch(kvs, geo, row0=(lo, hi))
                parts.append(patch.csr(kind, algo='sumfact'))
                assert 'twin' in patch.last_path()
                patch.close()
            V = scipy.sparse.vstack(parts).tocsr()
            assert np.array_equal(V.indptr, A.indptr) and np.array_equal(V.data, A.data), (kind, 'slabs')
        if not twin:
            continue
        # the convection-diffusion form (non-symmetric; pyiga/assemble.py:837-897): its coefficient follows the patch to the twin --
        # an affine one as its numbers, a sampled one with the two last grid axes exchanged
        for coeff in (iga.assemblers.AffineCoefficient(1.5, 0.2, -0.1, 0.3), lambda x, y, z: 1.5 + 0.2 * x * x - 0.1 * y + 0.3 * z):
            asm = iga.assemblers.ConvDiffAssembler3D(kvs, geo, coeff)
            A = asm.assemble_csr(algo='sumfact')
            path = asm.patch.last_path()
            E = asm.assemble_csr(algo='entrywise')
            asm.patch.close()
            assert path == {'geoA', 'fused', 'bf3', 'twin'}, path
            assert not np.isnan(A.data).any()
            assert rel_maxdiff(A, E) <= RTOL, ('convdiff', [kv.numdofs for kv in kvs], rel_maxdiff(A, E))
            N0 = kvs[0].numdofs
            parts = []
            for lo, hi in ((0, N0 // 2), (N0 // 2, N0)):
                sl = iga.assemblers.ConvDiffAssembler3D(kvs, geo, coeff, row0=(lo, hi))
                parts.append(sl.assemble_csr(algo='sumfact'))
                sl.patch.close()
            V = scipy.sparse.vstack(parts).tocsr()
            assert np.array_equal(V.indptr, A.indptr) and np.array_equal(V.data, A.data), 'convdiff slabs'


def test_ablation_variables_have_no_effect(iga, monkeypatch):
    """The switches of the timing experiments (work left out: wrong matrices by construction) exist only in -DIGX_ABLATE
    builds; in the shipped library the variables change nothing, and the chain of a patch is fixed when it is created."""
    kvs = (iga.bspline.make_knots(3, 0., 1., 9),) * 3
    geo = _geo(iga, 'cylinder')
    patch = iga.assemblers.DevicePatch(kvs, geo)
    A = patch.csr('stiffness', algo='sumfact')
    for var in ('IGX_GEOA_DBG', 'IGX_BF_DBG', 'IGX_NO_MIRROR', 'IGX_K1PAD', 'IGX_BF_MCHUNKS', 'IGX_FINALQ_TILE'):
        monkeypatch.setenv(var, '7')
    for var, val in (('IGX_PATH', 'unfused'), ('IGX_GEOA', '0'), ('IGX_FINAL', 'valu')):     # read at creation only
        monkeypatch.setenv(var, val)
    B = patch.csr('stiffness', algo='sumfact')
    assert patch.last_path() == {'geoA', 'fused', 'both', 'bf3'}
    patch.close()
    for var in ('IGX_PATH', 'IGX_GEOA', 'IGX_FINAL'):
        monkeypatch.delenv(var)
    patch = iga.assemblers.DevicePatch(kvs, geo)
    C = patch.csr('stiffness', algo='sumfact')
    patch.close()
    assert np.array_equal(A.data, B.data) and np.array_equal(A.data, C.data)


def test_placement_tries_opt_in(iga, monkeypatch):
    """IGX_PLACEMENT_TRIES (read at patch creation) with the chain of rounds 3-4 (IGX_BF=2: k_bf2 + mirror pass): the first
    assembly times the mirror pass on n candidate buffers for the CSR values and keeps the fastest.  Same matrix, the search is
    reported, and without the variable it does not run.  The default chain (k_bf3) has no mirror pass and never searches."""
    kvs = (iga.bspline.make_knots(3, 0., 1., 12),) * 3
    geo = _geo(iga, 'cylinder')
    monkeypatch.setenv('IGX_PLACEMENT_TRIES', '3')
    patch = iga.assemblers.DevicePatch(kvs, geo)
    monkeypatch.delenv('IGX_PLACEMENT_TRIES')
    patch.csr('stiffness', algo='sumfact')
    assert patch.placement()['tried'] == 0 and 'both' in patch.last_path()
    patch.close()
    monkeypatch.setenv('IGX_BF', '2')
    patch = iga.assemblers.DevicePatch(kvs, geo)
    A = patch.csr('stiffness', algo='sumfact')
    assert patch.placement()['tried'] == 0
    patch.close()
    monkeypatch.setenv('IGX_PLACEMENT_TRIES', '3')
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')
    patch = iga.assemblers.DevicePatch(kvs, geo)
    monkeypatch.delenv('IGX_PLACEMENT_TRIES')
    B = patch.csr('stiffness', algo='sumfact')
    pl = patch.placement()
    assert pl['tried'] == 3 and 0.0 < pl['best_ms'] <= pl['worst_ms']
    C2 = patch.csr('stiffness', algo='sumfact')                            # (the buffer is chosen once)
    assert patch.placement() == pl
    patch.close()
    assert np.array_equal(A.data, B.data) and np.array_equal(A.data, C2.data) and not np.isnan(B.data).any()
    # a form without a mirror pass: nothing to time, plain allocation
    monkeypatch.setenv('IGX_PLACEMENT_TRIES', '3')
    asm = iga.assemblers.ConvDiffAssembler3D(kvs, geo, lambda x, y, z: 1.0 + x)
    monkeypatch.delenv('IGX_PLACEMENT_TRIES')
    asm.assemble_csr(algo='sumfact')
    assert asm.patch.placement()['tried'] == 0
    asm.patch.close()


@pytest.mark.parametrize('d', [2, 3])
def test_stage_events_only_change_the_timing_record(iga, d, monkeypatch):
    """IGX_STAGE_EVENTS (read at patch creation): events between the kernels of a chain.  Off by default for patches whose
    kernels run for microseconds (only total_ms is measured), on request the per-kernel times appear; same matrix."""
    kvs = (iga.bspline.make_knots(3, 0., 1., 40),) * 2 if d == 2 else (iga.bspline.make_knots(2, 0., 1., 9),) * 3
    geo = _geo(iga, 'quarter_annulus' if d == 2 else 'cylinder')
    monkeypatch.setenv('IGX_PATH', 'unfused')
    out = {}
    for ev in (None, '1', '0'):
        if ev is None:
            monkeypatch.delenv('IGX_STAGE_EVENTS', raising=False)
        else:
            monkeypatch.setenv('IGX_STAGE_EVENTS', ev)
        patch = iga.assemblers.DevicePatch(kvs, geo)
        A = patch.csr('stiffness', algo='sumfact')
        tm = patch.timing()
        patch.close()
        staged = tm['stage0_ms'] > 0 and tm['final_ms'] > 0
        assert tm['total_ms'] > 0 and staged == (ev == '1'), (ev, tm)
        out[ev] = A.data
    assert np.array_equal(out[None], out['1']) and np.array_equal(out[None], out['0'])


# ------------------------------------------------------------------------------------------
# Full-size parity pinned to the REFERENCE (tests/golden/golden_fullsize.npz, make_golden.py 'fullsize'):
# multi_entries of the reference at seeded in-pattern pairs of BASELINE configs 2 and 3 at their real sizes and of the
# config-4 / config-5 degrees on 32^3 / 24^3 spans, compared with the device-assembled CSR at those positions.
def _csr_at(A, idx):
    """values of the CSR matrix at the (row, col) pairs (all inside the pattern)."""
    rows, cols = idx[:, 0].astype(np.int64), idx[:, 1].astype(np.int64)
    out = np.empty(len(rows))
    for k in range(len(rows)):
        lo, hi = A.indptr[rows[k]], A.indptr[rows[k] + 1]
        pos = lo + np.searchsorted(A.indices[lo:hi], cols[k])
        assert pos < hi and A.indices[pos] == cols[k]
        out[k] = A.data[pos]
    return out


@pytest.mark.parametrize('path', ['single', 'fused', 'unfused'])
def test_fullsize_vs_reference_c2(iga, golden, path, monkeypatch):
    """BASELINE config 2: 2D p=3 n=256 NURBS quarter annulus, 'CSR vs reference within 1e-12'; 'single' = the single-launch
    kernel (the default of small 2D patches) forced at this size."""
    monkeypatch.setenv('IGX_PATH', path)
    g = golden('fullsize')
    kv = iga.bspline.make_knots(3, 0., 1., 256)
    A = iga.assemble.stiffness((kv, kv), iga.geometry.quarter_annulus())
    assert A.nnz == int(g['c2_nnz'])
    scale = float(g['c2_absmax'])
    assert abs(abs(A).max() - scale) <= 1e-12 * scale
    assert np.abs(_csr_at(A, g['c2_idx']) - g['c2_val']).max() <= RTOL * scale
    # the whole matrix through a fixed vector: every entry takes part
    x = np.sin(0.37 * np.arange(A.shape[0]) + 0.1)
    assert np.abs(A @ x - g['c2_Ax']).max() <= 1e-11 * scale
    assert abs(A - A.T).max() == 0.0


def test_2d_geometry_inside_the_axis0_sweep(iga, oracle, monkeypatch):
    """Round 6: above the single-launch crossover a 2D mass / stiffness patch over a spline map takes TWO launches -- k_geoA (2D
    instantiation: control net -> Jacobian -> fields -> axis-0 sweep -> K1, no field arrays) and the final stage -- instead of field
    kernel + k_stageA + final stage.  `geoA` in last_path(); against the oracle, the entry-wise kernel, row slabs bit for bit;
    degrees 1 .. 4, NURBS / B-spline maps (degree 2 and 1 along axis 0), repeated knots on either axis, unequal degrees.
    (pyiga/assemblers.pyx:86-135, 234-349.)"""
    mk = iga.bspline.make_knots
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')
    cases = [((mk(3, 0., 1., 110), mk(3, 0., 1., 120)), 'quarter_annulus'),                         # (above the single-launch crossover: > 9216 rows)
             ((mk(2, 0., 1., 130), mk(2, 0., 1., 100)), 'bspline_quarter_annulus'),
             ((mk(1, 0., 1., 120), mk(1, 0., 1., 130)), 'quarter_annulus'),
             ((mk(4, 0., 1., 100), mk(4, 0., 1., 110)), 'unit_square'),
             ((mk(3, 0., 1., 60, mult=2), mk(2, 0., 1., 70, mult=2)), 'quarter_annulus'),
             ((mk(2, 0., 1., 128), mk(4, 0., 1., 100)), 'bspline_quarter_annulus')]
    ogeo = {'quarter_annulus': oracle.geo_quarter_annulus, 'bspline_quarter_annulus': oracle.geo_bspline_quarter_annulus,
            'unit_square': lambda: oracle.geo_unit_cube(2)}
    for kvs, gname in cases:
        geo = _geo(iga, gname)
        okvs = tuple(oracle.KnotVector(kv.kv, kv.p) for kv in kvs)
        for kind in ('stiffness', 'mass'):
            patch = iga.assemblers.DevicePatch(kvs, geo)
            A = patch.csr(kind, algo='sumfact')
            path = patch.last_path()
            E = patch.csr(kind, algo='entrywise')
            patch.close()
            tag = (kind, [kv.p for kv in kvs], [kv.numdofs for kv in kvs], gname, sorted(path))
            assert 'geoA' in path and 'single' not in path, tag
            assert not np.isnan(A.data).any() and abs(A - A.T).max() == 0.0, tag
            assert rel_maxdiff(A, E) <= RTOL, (tag, rel_maxdiff(A, E))
            R = oracle.assemble(kind, okvs, ogeo[gname](), nthreads=8)
            assert A.nnz == R.nnz and rel_maxdiff(A, R) <= RTOL, (tag, rel_maxdiff(A, R))
            N0 = kvs[0].numdofs
            parts = []
            for lo, hi in ((0, N0 // 3), (N0 // 3, N0 - 2), (N0 - 2, N0)):
                sl = iga.assemblers.DevicePatch(kvs, geo, row0=(lo, hi))
                parts.append(sl.assemble(kind, algo='sumfact', to_host=True).copy())
                sl.close()
            assert np.array_equal(np.concatenate(parts), A.data), tag


@pytest.mark.parametrize('path', ['fused', 'unfused'])
def test_fullsize_vs_reference_3d(iga, golden, path, monkeypatch):
    """BASELINE config 3 at full size (3D p=2 n=64, mass + stiffness) and the config-4 / config-5 degrees at the largest
    size the reference was run at (p=4 n=32, p=5 n=24; stiffness and the convection-diffusion form)."""
    monkeypatch.setenv('IGX_PATH', path)
    g = golden('fullsize')
    geo = _geo(iga, 'cylinder')
    for tag, p, n, kinds in (('c3', 2, 64, ('stiff', 'mass')), ('p4n32', 4, 32, ('stiff',)), ('p5n24', 5, 24, ('stiff', 'convdiff'))):
        kv = iga.bspline.make_knots(p, 0., 1., n)
        kvs = (kv, kv, kv)
        idx = g[tag + '_idx']
        for kind in kinds:
            if kind == 'convdiff':
                A = iga.assemblers.ConvDiffAssembler3D(kvs, geo, lambda x, y, z: 1.0 + x).assemble_csr()
            else:
                A = (iga.assemble.stiffness if kind == 'stiff' else iga.assemble.mass)(kvs, geo)
            ref = g['%s_%s' % (tag, kind)]
            err = np.abs(_csr_at(A, idx) - ref).max()
            assert err <= RTOL * abs(A).max(), (tag, kind, err / abs(A).max())
            del A


@pytest.mark.parametrize('d,p,n', [(2, 1, 9), (2, 2, 33), (2, 3, 70), (2, 4, 37), (2, 5, 21), (3, 1, 7), (3, 2, 13),
                                   (3, 3, 11), (3, 4, 9), (3, 5, 8)])
def test_fused_equals_unfused(iga, d, p, n, monkeypatch):
    """The fused sweep + final stage against the round-1 kernels (K2 through HBM) for every degree of the fast path, mass and
    stiffness: same matrix to rounding, exactly symmetric, every value written.  Since k_bf3 took over the symmetric forms,
    IGX_PATH=fused runs k_bf3 here in 2D and 3D (it writes both triangles: no mirror pass); the first fused stage k_bf2 and the
    mirror passes are tested in tests/test_bf2_kernels_gpu.py."""
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')
    kv = iga.bspline.make_knots(p, 0., 1., n)
    kvs = (kv,) * d
    geo = iga.geometry.quarter_annulus() if d == 2 else _geo(iga, 'cylinder')
    for kind in ('mass', 'stiffness'):
        monkeypatch.setenv('IGX_PATH', 'fused')
        patch = iga.assemblers.DevicePatch(kvs, geo)
        A = patch.csr(kind, algo='sumfact')
        assert {'fused', 'bf3', 'both'} <= patch.last_path() and 'mirror' not in patch.last_path(), (kind, patch.last_path())
        monkeypatch.setenv('IGX_PATH', 'unfused')
        B = iga.assemblers.DevicePatch(kvs, geo).csr(kind, algo='sumfact')
        assert not np.isnan(A.data).any()
        assert abs(A - A.T).max() == 0.0
        assert rel_maxdiff(A, B) <= RTOL, (kind, rel_maxdiff(A, B))
        if d == 2:                                   # everything in one launch (the default of small 2D patches)
            monkeypatch.setenv('IGX_PATH', 'single')
            patch = iga.assemblers.DevicePatch(kvs, geo)
            C = patch.csr(kind, algo='sumfact')
            assert patch.last_path() == {'single'}
            assert not np.isnan(C.data).any() and abs(C - C.T).max() == 0.0
            assert rel_maxdiff(C, B) <= RTOL, (kind, rel_maxdiff(C, B))


# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d,p,n,G', [(3, 2, 9, 2), (3, 4, 6, 3), (2, 3, 20, 4), (2, 1, 11, 1)])
def test_resident_load_vector(iga, d, p, n, G):
    """igx_load_vector_d on device-resident function values == the host-buffer entry point, bit for bit, per slab."""
    kv = iga.bspline.make_knots(p, 0., 1., n)
    kvs = (kv,) * d
    geo = _geo(iga, 'quarter_annulus' if d == 2 else 'cylinder')
    f = _f2 if d == 2 else _f3
    N0 = kv.numdofs
    bounds = [N0 * k // G for k in range(G + 1)]
    fvals = None
    for k in range(G):
        patch = iga.assemblers.DevicePatch(kvs, geo, row0=(bounds[k], bounds[k + 1]))
        if fvals is None:
            grid = tuple(patch.gauss(a)[0] for a in range(d))
            fvals = iga.utils.grid_eval_transformed(f, grid, geo)
        ref = patch.load_vector(fvals)
        lo, cnt = patch.gauss_slab()
        assert 0 <= lo and lo + cnt <= fvals.shape[0] and (G > 1 or cnt == fvals.shape[0])
        patch.upload_function(fvals)
        assert patch.load_vector_resident() is None          # result stays in HBM
        out = patch.load_vector_resident(to_host=True)
        assert np.array_equal(out, ref)
        assert np.array_equal(patch.load_vector_resident(to_host=True), ref)     # persistent buffers: repeatable
        patch.close()


@pytest.mark.parametrize('d,p,n', [(3, 2, 8), (3, 4, 6), (2, 3, 30), (2, 5, 12), (3, 1, 9)])
def test_entries_wave_vs_thread_and_resident(iga, d, p, n, monkeypatch):
    """Wave-per-entry kernel (default for p >= 2) against the one-thread-per-entry kernel (the reference's summation order)
    and against the assembled matrix; device-resident index pairs give the same bits as the host entry point."""
    kv = iga.bspline.make_knots(p, 0., 1., n)
    kvs = (kv,) * d
    geo = _geo(iga, 'quarter_annulus' if d == 2 else 'cylinder')
    patch = iga.assemblers.DevicePatch(kvs, geo)
    N = patch.shape[0]
    rng = np.random.default_rng(7 + d + p)
    indptr, indices = patch.pattern()
    rows = np.repeat(np.arange(N), np.diff(indptr))
    pick = rng.choice(len(indices), size=min(4000, len(indices)), replace=False)
    idx = np.stack([rows[pick], indices[pick]], axis=1)
    idx = np.concatenate([idx, rng.integers(0, N, size=(500, 2))])          # + arbitrary pairs (mostly outside the pattern)
    kinds = ['mass', 'stiffness'] + (['convdiff'] if d == 3 else [])
    monkeypatch.setenv('IGX_ENTRIES', 'thread')                     # (chain choices are read when a patch is created)
    patch_t = iga.assemblers.DevicePatch(kvs, geo)
    monkeypatch.delenv('IGX_ENTRIES')
    if d == 3:
        patch.set_coeff(1.5)
        patch_t.set_coeff(1.5)
    for kind in kinds:
        e_thread = patch_t.entries(kind, idx)
        e_wave = patch.entries(kind, idx)
        scale = np.abs(e_thread).max()
        assert np.abs(e_wave - e_thread).max() <= RTOL * scale
        assert np.array_equal(e_wave == 0.0, e_thread == 0.0)
        A = patch.csr(kind)
        ref = np.asarray(A[idx[:, 0], idx[:, 1]]).ravel()
        assert np.abs(e_wave - ref).max() <= RTOL * scale
        patch.upload_pairs(idx)
        assert patch.entries_resident(kind) is None
        assert np.array_equal(patch.entries_resident(kind, to_host=True), e_wave)
    patch.close()


# ------------------------------------------------------------------------------------------
def _wavy_box(iga, deg0, spans0, nurbs):
    """3D spline geometry with several knot spans (and degree deg0) along axis 0: a perturbed box."""
    kv0 = iga.bspline.make_knots(deg0, 0., 1., spans0)
    kv1 = iga.bspline.make_knots(2, 0., 1., 2)
    kv2 = iga.bspline.make_knots(1, 0., 1., 3)
    n = (kv0.numdofs, kv1.numdofs, kv2.numdofs)
    z, y, x = np.meshgrid(*(np.linspace(0., 1., k) for k in n), indexing='ij')
    rng = np.random.default_rng(11)
    C = np.stack([x * (1.5 + 0.3 * y), y + 0.2 * np.sin(2. * z), z * (1. + 0.25 * x)], axis=-1)
    C = C + 0.02 * rng.standard_normal(C.shape)
    if nurbs:
        return iga.geometry.NurbsFunc((kv0, kv1, kv2), C, 1.0 + 0.3 * rng.random(n))
    return iga.bspline.BSplineFunc((kv0, kv1, kv2), C)


@pytest.mark.parametrize('deg0,spans0,nurbs', [(1, 3, False), (2, 4, True), (2, 9, False), (1, 1, True)])
@pytest.mark.parametrize('p,n', [(3, 7), (4, 5), (2, 11)])
def test_geometry_in_sweep_multi_span(iga, deg0, spans0, nurbs, p, n, monkeypatch):
    """k_geoA (geometry evaluated inside the axis-0 sweep; batches of planes that straddle span boundaries of the
    geometry's axis 0) against the separate field + sweep kernels, full patch and row slabs, mass and stiffness."""
    geo = _wavy_box(iga, deg0, spans0, nurbs)
    kv = iga.bspline.make_knots(p, 0., 1., n)
    kvs = (kv,) * 3
    for kind in ('stiffness', 'mass'):
        patch = iga.assemblers.DevicePatch(kvs, geo)
        A = patch.csr(kind, algo='sumfact')
        assert 'geoA' in patch.last_path()
        monkeypatch.setenv('IGX_GEOA', '0')                             # (chain choices are read when a patch is created)
        patch0 = iga.assemblers.DevicePatch(kvs, geo)
        monkeypatch.delenv('IGX_GEOA')
        B = patch0.csr(kind, algo='sumfact')
        assert 'geoA' not in patch0.last_path()
        patch0.close()
        E = patch.csr(kind, algo='entrywise')
        patch.close()
        assert rel_maxdiff(A, B) <= RTOL and rel_maxdiff(A, E) <= RTOL
        assert abs(A - A.T).max() == 0.0
        N0 = kv.numdofs
        parts = []
        for lo, hi in ((0, N0 // 3), (N0 // 3, N0 - 2), (N0 - 2, N0)):
            sl = iga.assemblers.DevicePatch(kvs, geo, row0=(lo, hi))
            parts.append(sl.csr(kind, algo='sumfact'))
            sl.close()
        S = scipy.sparse.vstack(parts).tocsr()
        assert np.array_equal(S.indptr, A.indptr) and np.array_equal(S.data, A.data)


@pytest.mark.parametrize('deg0,spans0,nurbs', [(1, 1, True), (2, 4, True), (1, 3, False)])
@pytest.mark.parametrize('p,n', [(4, 7), (3, 9), (4, 13)])
def test_matrix_core_axis0_sweep(iga, deg0, spans0, nurbs, p, n, monkeypatch):
    """IGX_GEOA=mfma (round 4, opt-in: measured slower than the vector form): the axis-0 sweep of
    k_geoA on v_mfma_f64_16x16x4_f64 -- fixed accumulator rows per pair, four planes per instruction, single planes by
    vector multiply-adds.  Same matrix as the default chain to rounding, exactly symmetric, and the row slabs reproduce
    the whole patch bit for bit (the instruction adds its four planes in order, one rounding each: a pair's sum does not
    depend on how the batches of planes cut its spans)."""
    geo = _wavy_box(iga, deg0, spans0, nurbs) if spans0 > 1 or deg0 > 1 else _geo(iga, 'cylinder')
    kv = iga.bspline.make_knots(p, 0., 1., n)
    kvs = (kv, iga.bspline.make_knots(p, 0., 1., n - 2), kv)
    ref = iga.assemblers.DevicePatch(kvs, geo)
    R = ref.csr('stiffness', algo='sumfact')
    ref.close()
    monkeypatch.setenv('IGX_GEOA', 'mfma')
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')
    patch = iga.assemblers.DevicePatch(kvs, geo)
    A = patch.csr('stiffness', algo='sumfact')
    assert 'geoA' in patch.last_path() and not np.isnan(A.data).any()
    A2 = patch.csr('stiffness', algo='sumfact')
    patch.close()
    assert np.array_equal(A.data, A2.data)
    assert rel_maxdiff(A, R) <= 1e-13 and abs(A - A.T).max() == 0.0
    N0 = kv.numdofs
    parts = []
    for lo, hi in ((0, 3), (3, N0 - 4), (N0 - 4, N0)):
        sl = iga.assemblers.DevicePatch(kvs, geo, row0=(lo, hi))
        parts.append(sl.csr('stiffness', algo='sumfact'))
        sl.close()
    S = scipy.sparse.vstack(parts).tocsr()
    assert np.array_equal(S.indptr, A.indptr) and np.array_equal(S.data, A.data)


@pytest.mark.parametrize('deg0,spans0,nurbs', [(1, 1, True), (2, 4, True), (2, 9, False)])
@pytest.mark.parametrize('p,n', [(2, 9), (3, 7), (4, 6), (5, 7)])
def test_convdiff_geometry_in_sweep(iga, oracle, deg0, spans0, nurbs, p, n, monkeypatch):
    """Round 4: the convection-diffusion form with geometry, coefficient and fields evaluated inside the axis-0 sweep
    (k_geoA, non-symmetric: full pair window, two-source slots, geometry waves beside the sweep waves) against the field
    kernel + k_stageA chain (IGX_GEOA=0), the entry-wise kernels and -- on the cylinder -- the CPU oracle; sampled and
    affine coefficient; row slabs bit for bit."""
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')
    cyl = spans0 == 1 and deg0 == 1
    geo = _geo(iga, 'cylinder') if cyl else _wavy_box(iga, deg0, spans0, nurbs)
    kvs = (iga.bspline.make_knots(p, 0., 1., n), iga.bspline.make_knots(p, 0., 1., n + 1), iga.bspline.make_knots(p, 0., 1., n - 1))
    coeff = lambda x, y, z: 1.0 + 0.5 * x - 0.25 * y + 0.125 * z
    asm = iga.assemblers.ConvDiffAssembler3D(kvs, geo, coeff)                # sampled on the host, read per point
    A = asm.assemble_csr(algo='sumfact')
    assert 'geoA' in asm.patch.last_path() and 'fused' in asm.patch.last_path() and not np.isnan(A.data).any()
    E = asm.assemble_csr(algo='entrywise')
    asm.patch.close()
    aff = iga.assemblers.ConvDiffAssembler3D(kvs, geo, iga.assemblers.AffineCoefficient(1.0, 0.5, -0.25, 0.125))
    F = aff.assemble_csr(algo='sumfact')                                     # evaluated in the kernel from the geometry map
    assert 'geoA' in aff.patch.last_path()
    aff.patch.close()
    monkeypatch.setenv('IGX_GEOA', '0')
    old = iga.assemblers.ConvDiffAssembler3D(kvs, geo, coeff)
    monkeypatch.delenv('IGX_GEOA')
    B = old.assemble_csr(algo='sumfact')
    assert 'geoA' not in old.patch.last_path()
    old.patch.close()
    assert rel_maxdiff(A, B) <= RTOL and rel_maxdiff(A, E) <= RTOL and rel_maxdiff(F, A) <= RTOL
    assert abs(A - A.T).max() > 1e-3 * abs(A).max()
    if cyl and p <= 3:
        okvs = tuple(oracle.KnotVector(kv.kv, kv.p) for kv in kvs)
        R = oracle.assemble_nonsymmetric('convdiff', okvs, oracle.geo_cylinder(), coeff=coeff, nthreads=8)
        assert np.array_equal(A.indices, R.indices) and rel_maxdiff(A, R) <= RTOL
    N0 = kvs[0].numdofs
    parts = []
    for lo, hi in ((0, 2), (2, N0 - 3), (N0 - 3, N0)):
        sl = iga.assemblers.ConvDiffAssembler3D(kvs, geo, coeff, row0=(lo, hi))
        parts.append(sl.assemble_csr(algo='sumfact'))
        sl.patch.close()
    S = scipy.sparse.vstack(parts).tocsr()
    assert np.array_equal(S.indptr, A.indptr) and np.array_equal(S.data, A.data)


def test_coefficient_expression_compiled_at_run_time(iga, tmp_path, monkeypatch):
    """igx_patch_set_coeff_expr (round 4, SURVEY 8 f1 "full"): the coefficient of the convection-diffusion form as an
    expression, compiled with hiprtc for the device and cached on disk by source hash, evaluated on the Gauss points from the
    geometry map -- against the same function sampled on the host and shipped (the reference's way), NURBS and B-spline
    geometries, row slabs, the cache (miss, then hit, also from a second patch), a failing expression."""
    monkeypatch.setenv('IGX_CACHE_DIR', str(tmp_path / 'cache'))
    Expr = iga.assemblers.ExprCoefficient
    text = '1 + x**2 + 0.5 * sin(pi * z) - maximum(y, 0.25) / 3'
    fn = lambda x, y, z: 1 + x ** 2 + 0.5 * np.sin(np.pi * z) - np.maximum(y, 0.25) / 3
    kvs = (iga.bspline.make_knots(3, 0., 1., 7), iga.bspline.make_knots(3, 0., 1., 8), iga.bspline.make_knots(3, 0., 1., 6))
    first = True
    for geo in (_geo(iga, 'cylinder'), _wavy_box(iga, 2, 4, False)):
        host = iga.assemblers.ConvDiffAssembler3D(kvs, geo, fn)
        R = host.assemble_csr(algo='sumfact')
        host.patch.close()
        dev = iga.assemblers.ConvDiffAssembler3D(kvs, geo, Expr(text))
        assert dev.coeff_cache_hit == (not first)            # compiled once per source and architecture, then found on disk
        first = False
        A = dev.assemble_csr(algo='sumfact')
        E = dev.assemble_csr(algo='entrywise')
        dev.patch.close()
        assert rel_maxdiff(A, R) <= RTOL and rel_maxdiff(E, R) <= RTOL
        N0 = kvs[0].numdofs
        parts = []
        for lo, hi in ((0, 3), (3, N0)):
            sl = iga.assemblers.ConvDiffAssembler3D(kvs, geo, Expr(text), row0=(lo, hi))
            assert sl.coeff_cache_hit
            parts.append(sl.assemble_csr(algo='sumfact'))
            sl.patch.close()
        assert np.array_equal(scipy.sparse.vstack(parts).tocsr().data, A.data)
    assert len(os.listdir(str(tmp_path / 'cache'))) == 1
    patch = iga.assemblers.DevicePatch(kvs, _geo(iga, 'cylinder'))
    with pytest.raises(iga._lib.IgxError, match='nosuch'):
        patch.set_coeff_expr('1.0 + nosuch(x)')
    patch.close()


@pytest.mark.parametrize('ps,ns,gname', [((3, 3, 3), (5, 6, 7), 'cylinder'), ((4, 2, 3), (4, 7, 5), 'seg3_bspline_annulus'),
                                         ((2, 2, 2), (6, 6, 6), 'unit_cube'), ((1, 3, 2), (5, 4, 6), 'cylinder'),
                                         ((5, 5, 5), (3, 7, 4), 'cylinder')])
def test_separable_geometry_kronecker(iga, oracle, ps, ns, gname, monkeypatch):
    """Round 4 (opt-in, IGX_SEPARABLE=1 / DevicePatch.assemble_kron): a geometry that is separable along axis 0 -- an extruded
    cross-section, like the cylinder of the BASELINE configs -- gives  M = M0 (x) M2D,  K = M0 (x) K2D + K0 (x) M2D  with weighted
    1D matrices of axis 0 and the 2D matrices of the cross-section (the reference's Kronecker path, pyiga/assemble.py:125-190,
    for geo = None, extended to separable maps).  Same pattern, exactly symmetric, equal to the general quadrature chain to
    rounding and to the CPU oracle; row slabs of the expansion reproduce it bit for bit; other geometries are left alone."""
    g = iga.geometry
    geo = {'cylinder': lambda: _geo(iga, 'cylinder'), 'unit_cube': g.unit_cube,
           'seg3_bspline_annulus': lambda: g.tensor_product(g.line_segment(0.5, 2.0, intervals=3), g.bspline_quarter_annulus())}[gname]()
    kvs = tuple(iga.bspline.make_knots(p, 0., 1., n) for p, n in zip(ps, ns))
    assert g.split_axis0(geo) is not None
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')
    for kind in ('mass', 'stiffness'):
        B = getattr(iga.assemble, kind)(kvs, geo)                          # general chain
        monkeypatch.setenv('IGX_SEPARABLE', '1')
        A = getattr(iga.assemble, kind)(kvs, geo)
        monkeypatch.delenv('IGX_SEPARABLE')
        assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices) and not np.isnan(A.data).any()
        assert rel_maxdiff(A, B) <= 1e-14 and abs(A - A.T).max() == 0.0
        if gname == 'cylinder' and max(ps) <= 3:
            okvs = tuple(oracle.make_knots(p, 0., 1., n) for p, n in zip(ps, ns))
            assert rel_maxdiff(A, oracle.assemble(kind, okvs, oracle.geo_cylinder(), nthreads=8)) <= RTOL
        # explicit device API, whole and in slabs
        p3 = iga.assemblers.DevicePatch(kvs, geo)
        geo2, m0, k0 = iga.assemble.separable_terms(kvs, geo, p3)
        p2 = iga.assemblers.DevicePatch(kvs[1:], geo2, nqp=p3.nqp)
        full = p3.assemble_kron(kind, p2, m0, k0)
        assert p3.last_path() == {'kron'} and np.array_equal(full, A.data)
        N0 = kvs[0].numdofs
        parts = []
        for lo, hi in ((0, 2), (2, N0 - 1), (N0 - 1, N0)):
            sl = iga.assemblers.DevicePatch(kvs, geo, row0=(lo, hi))
            parts.append(sl.assemble_kron(kind, p2, m0, k0))
            sl.close()
        assert np.array_equal(np.concatenate(parts), full)
        p2.close(); p3.close()
    # not separable along axis 0: the switch changes nothing
    for other in (g.twisted_box(), g.tensor_product(g.quarter_annulus(), g.line_segment(0.0, 1.0))):
        assert g.split_axis0(other) is None
    kv = iga.bspline.make_knots(2, 0., 1., 4)
    R = iga.assemble.stiffness((kv,) * 3, g.twisted_box())
    monkeypatch.setenv('IGX_SEPARABLE', '1')
    assert np.array_equal(iga.assemble.stiffness((kv,) * 3, g.twisted_box()).data, R.data)


def test_set_form_device_and_failed_call(iga):
    """igx_patch_set_form_d (coefficients already on the device, resident slab) == the host entry point; a call that fails
    validation leaves the previous form in place."""
    import ctypes as C
    lib = iga._lib.load()
    kv = iga.bspline.make_knots(2, 0., 1., 6)
    kvs = (kv,) * 3
    geo = _geo(iga, 'cylinder')
    for row0 in (None, (2, 5)):
        patch = iga.assemblers.DevicePatch(kvs, geo, row0=row0)
        G = tuple(patch.info.ngauss[k] for k in range(3))
        rng = np.random.default_rng(5)
        c00, c12 = 1.0 + rng.random(G), rng.standard_normal(G)
        table = [[None] * 4 for _ in range(4)]
        table[0][0], table[1][2] = c00, c12
        patch.set_form(table)
        ref = patch.assemble('form', algo='sumfact')
        lo, cnt = patch.gauss_slab()
        bufs, ptrs = [], (C.c_void_p * 16)()
        for k, arr in ((0, c00), (4 * 1 + 2, c12)):
            part = np.ascontiguousarray(arr[lo:lo + cnt])
            d = lib.igx_dev_alloc(patch.ctx.handle, part.nbytes)
            assert d
            iga._lib.check(lib.igx_dev_upload(patch.ctx.handle, d, part.ctypes.data, part.nbytes), 'upload')
            bufs.append(d)
            ptrs[k] = d
        # a failing call first: a coefficient of the 4th jet slot row and column is fine in 3D, so break it with an empty table
        empty = (C.c_void_p * 16)()
        assert lib.igx_patch_set_form_d(patch.handle, empty) != 0
        assert np.array_equal(patch.assemble('form', algo='sumfact'), ref)         # previous form still in place
        iga._lib.check(lib.igx_patch_set_form_d(patch.handle, ptrs), 'igx_patch_set_form_d')
        for d in bufs:
            lib.igx_dev_free(patch.ctx.handle, d)                                   # the patch keeps its own copy
        assert np.array_equal(patch.assemble('form', algo='sumfact'), ref)
        patch.close()


def test_reference_signature_kwargs(iga):
    """assemble(..., layout=, symmetric=) as in pyiga/assemble.py:837; get/set_max_threads; the zero functional."""
    kv = iga.bspline.make_knots(2, 0., 1., 5)
    kvs = (kv,) * 3
    geo = _geo(iga, 'cylinder')
    A = iga.assemble.assemble('inner(grad(u), grad(v)) * dx', kvs, geo=geo, layout='blocked')
    assert rel_maxdiff(A, iga.assemble.stiffness(kvs, geo)) <= RTOL
    with pytest.raises(ValueError):
        iga.assemble.assemble('u * v * dx', kvs, geo=geo, layout='packed')
    # symmetric=True on a non-symmetric form: lower triangle mirrored, as the reference does
    form = 'inner((x[2], 0.0, -x[0]), grad(u)) * v * dx'
    N = iga.assemble.assemble(form, kvs, geo=geo)
    S = iga.assemble.assemble(form, kvs, geo=geo, symmetric=True)
    assert abs(N - N.T).max() > 0.0
    L = scipy.sparse.tril(N)
    assert abs(S - (L + scipy.sparse.tril(N, k=-1).T)).max() == 0.0
    z = iga.assemble.assemble('0 * v * dx', kvs, geo=geo)
    assert z.shape == (kv.numdofs,) * 3 and not z.any()
    iga.set_max_threads(3)
    assert iga.get_max_threads() == 3


def test_inner_products_1d_with_geometry(iga):
    """1D load vector over a curve parametrisation: weights times |x'(t)| (pyiga/assemble.py:326-333)."""
    kv = iga.bspline.make_knots(3, 0., 1., 7)
    geo = iga.geometry.line_segment(1.0, 3.0, intervals=2)         # x(t) = 1 + 2 t
    ref0 = iga.assemble.inner_products(kv, lambda x: np.ones_like(x))
    out = iga.assemble.inner_products(kv, lambda x: np.ones_like(x), geo=geo)
    assert np.abs(out - 2.0 * ref0).max() <= 1e-14
    assert abs(out.sum() - 2.0) <= 1e-14                          # length of the segment
    phys = iga.assemble.inner_products(kv, lambda x: x, f_physical=True, geo=geo)
    assert abs(phys.sum() - 4.0) <= 1e-13                         # int_1^3 x dx


def test_entry_func_ptr_capsule(iga):
    """The "entryfunc" capsule of the reference's plugin interface (pyiga/genericasm.pxi:780-786): a C function pointer that
    returns single entries."""
    import ctypes as C
    kv = iga.bspline.make_knots(2, 0., 1., 5)
    asm = iga.assemblers.StiffnessAssembler2D((kv, kv), _geo(iga, 'quarter_annulus'))
    cap = asm.entry_func_ptr()
    get = C.pythonapi.PyCapsule_GetPointer
    get.restype, get.argtypes = C.c_void_p, [C.py_object, C.c_char_p]
    fn = C.CFUNCTYPE(C.c_double, C.c_size_t, C.c_size_t, C.c_void_p)(get(cap, b'entryfunc'))
    for i, j in ((0, 0), (8, 9), (20, 13), (3, 40)):
        assert fn(i, j, None) == asm.entry(i, j)
    assert fn(3, 40, None) == 0.0


def test_affine_coefficient_on_device(iga):
    """igx_patch_set_coeff_affine: the coefficient of the convection-diffusion form evaluated on the device through the
    geometry map == the host-sampled callable (full patch and a row slab), to rounding."""
    kv = iga.bspline.make_knots(2, 0., 1., 6)
    kvs = (kv,) * 3
    geo = _geo(iga, 'cylinder')
    aff = iga.assemblers.AffineCoefficient(1.0, 0.5, -0.25, 2.0)
    for row0 in (None, (2, 6)):
        A = iga.assemblers.ConvDiffAssembler3D(kvs, geo, aff, row0=row0).assemble_csr()
        B = iga.assemblers.ConvDiffAssembler3D(kvs, geo, lambda x, y, z: 1.0 + 0.5 * x - 0.25 * y + 2.0 * z, row0=row0).assemble_csr()
        assert rel_maxdiff(A, B) <= RTOL
    assert aff(1.0, 2.0, 3.0) == 1.0 + 0.5 - 0.5 + 6.0


# ------------------------------------------------------------------------------------------
# On-demand assemblers with a bounding box (pyiga/codegen/cython.py:541-559, pyiga/_hdiscr.py:5-11,37-56)
def _ondemand_cases(iga):
    mk = iga.bspline.make_knots
    kvs3 = (mk(2, 0., 1., 6), mk(3, 0., 1., 5), mk(2, 0., 1., 7, mult=2))
    kvs2 = (mk(3, 0., 1., 9), mk(2, 0., 1., 12))
    A = iga.assemblers
    cyl, ann = _geo(iga, 'cylinder'), _geo(iga, 'quarter_annulus')
    return [('stiff3d', kvs3, lambda **kw: A.StiffnessAssembler3D(kvs3, cyl, **kw)),
            ('mass3d', kvs3, lambda **kw: A.MassAssembler3D(kvs3, cyl, **kw)),
            ('convdiff3d', kvs3, lambda **kw: A.ConvDiffAssembler3D(kvs3, cyl, lambda x, y, z: 1.0 + x, **kw)),
            ('stiff2d', kvs2, lambda **kw: A.StiffnessAssembler2D(kvs2, ann, **kw)),
            ('mass2d', kvs2, lambda **kw: A.MassAssembler2D(kvs2, ann, **kw))]


def test_ondemand_bbox_vs_reference(iga, golden):
    """Rows assembled by an assembler that only holds the bounding box of their supports = what the reference's
    compile_vform(..., on_demand=True) class with the same bbox gives through _assemble_partial_rows."""
    g = golden('ondemand')
    for name, kvs, make in _ondemand_cases(iga):
        rows = g[name + '_rows']
        bbox = iga.assemble.bbox_for_rows(kvs, rows)
        assert np.array_equal(np.array(bbox), g[name + '_bbox'])
        asm = make(bbox=bbox)
        S = iga.assemble.assemble_partial_rows(asm, rows)
        sub = S[rows]
        assert np.array_equal(sub.indptr, g[name + '_indptr']) and np.array_equal(sub.indices, g[name + '_indices'])
        ref = g[name + '_data']
        assert np.abs(sub.data - ref).max() <= RTOL * np.abs(ref).max(), name
        # the whole-patch assembler agrees; a pair whose common support leaves the box is refused (NaN), not wrong
        full = make()
        I, J = iga.assemble._nonzeros_for_rows(kvs, kvs, rows)
        pairs = np.column_stack((I, J)).astype(np.uintp)
        assert np.abs(asm.multi_entries(pairs) - full.multi_entries(pairs)).max() <= RTOL * np.abs(ref).max()
        n = int(np.prod([kv.numdofs for kv in kvs]))
        far = np.array([[n - 1, n - 1], [0, 0]], dtype=np.uintp)
        out = asm.multi_entries(far)
        assert np.isnan(out).all(), (name, out)
        assert asm.multi_entries(np.array([[0, n - 1]], dtype=np.uintp))[0] == 0.0      # disjoint supports: still exact 0
        with pytest.raises(iga._lib.IgxError):
            asm.patch.assemble(asm._kind)                     # a boxed patch serves batched entries only


def test_ondemand_bbox_other_geometries_and_forms(iga):
    """Bounding boxes with a Jacobian-array geometry (sampled on the box only), a general form string with sampled
    coefficients and the device-evaluated affine coefficient: equal to the whole-patch assemblers on the rows of the box."""
    mk = iga.bspline.make_knots
    kvs = (mk(3, 0., 1., 6), mk(2, 0., 1., 8), mk(2, 0., 1., 7))
    nd = [kv.numdofs for kv in kvs]
    rows = np.ravel_multi_index(np.array([(4, 5, 3), (5, 5, 4), (4, 6, 4)]).T, nd)
    bbox = iga.assemble.bbox_for_rows(kvs, rows)
    I, J = iga.assemble._nonzeros_for_rows(kvs, kvs, rows)
    pairs = np.column_stack((I, J)).astype(np.uintp)
    cyl = _geo(iga, 'cylinder')
    A = iga.assemblers
    form = '(inner(dot(K, grad(u)), grad(v)) + inner(b, grad(u)) * v + c * u * v) * dx'
    inputs = {'K': lambda x, y, z: np.stack([np.stack([2.0 + x, 0.1 * y, 0 * x], -1), np.stack([0.1 * y, 1.0 + z, 0 * x], -1),
                                             np.stack([0 * x, 0 * x, 1.5 + 0 * x], -1)], -2),
              'b': lambda x, y, z: np.stack([y, -x, 1.0 + 0 * x], -1), 'c': lambda x, y, z: 1.0 + x * y}
    makers = [lambda **kw: A.StiffnessAssembler3D(kvs, _OpaqueGeo(cyl), **kw),
              lambda **kw: A.ConvDiffAssembler3D(kvs, cyl, A.AffineCoefficient(1.0, 1.0, 0.5, -0.25), **kw),
              lambda **kw: A.GeneralFormAssembler3D(kvs, cyl, form, inputs=inputs, **kw)]
    for make in makers:
        full, boxed = make(), make(bbox=bbox)
        ref = full.multi_entries(pairs)
        out = boxed.multi_entries(pairs)
        assert np.isfinite(out).all()
        assert np.abs(out - ref).max() <= RTOL * np.abs(ref).max()
    # the opaque geometry was asked for its Jacobians on the box only
    boxed = makers[0](bbox=bbox)
    assert boxed.patch.fields('stiffness').shape[1:] == tuple((hi - lo) * boxed.nqp for lo, hi in bbox)


def _device_free_bytes():
    import ctypes
    hip = ctypes.CDLL('libamdhip64.so')
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def test_ondemand_bbox_at_c4_size(iga):
    """A 60-row request on the 3D p=4 128^3 patch through a boxed assembler: < 100 MB of device memory (the whole patch keeps
    12.6 GB of fields for the same request), same values as the whole-patch assembler."""
    kv = iga.bspline.make_knots(4, 0., 1., 128)
    kvs = (kv, kv, kv)
    cyl = _geo(iga, 'cylinder')
    N = kv.numdofs
    rows = np.ravel_multi_index((np.full(60, 70), np.full(60, 41), 30 + np.arange(60)), (N, N, N))
    bbox = iga.assemble.bbox_for_rows(kvs, rows)
    iga._lib.context().sync()
    before = _device_free_bytes()
    asm = iga.assemblers.StiffnessAssembler3D(kvs, cyl, bbox=bbox)
    S = iga.assemble.assemble_partial_rows(asm, rows)
    used = before - _device_free_bytes()
    assert used < 100e6, used
    assert S.nnz == S[rows].nnz and S.nnz > 60 * 5 ** 3
    full = iga.assemblers.StiffnessAssembler3D(kvs, cyl)
    I, J = iga.assemble._nonzeros_for_rows(kvs, kvs, rows[::7])
    pairs = np.column_stack((I, J)).astype(np.uintp)
    ref = full.multi_entries(pairs)
    got = np.asarray(S[I, J]).ravel()
    assert np.abs(got - ref).max() <= RTOL * np.abs(ref).max()
    full.patch.close()


# ------------------------------------------------------------------------------------------
# Form strings with vector-valued basis functions and boundary integrals (SURVEY section 8 f1 "full";
# test/test_assemble.py:314-400,452-476).  Goldens: the reference's assemble() on the same strings (make_golden.py vecforms).
def _vec_inputs():
    return {'c': lambda x, y: 1.0 + x * y, 'K': lambda x, y: np.stack([np.stack([1.0 + x, 0.5 * y], -1), np.stack([0 * x, 2.0 - y], -1)], -2),
            'f': lambda x, y: x * y ** 2, 'gv': lambda x, y: (y, -x)}


_VEC_FORMS = {
    'nonsym': ('inner(as_matrix([[2,1],[0,0]]).dot(u), v) * dx', [('u', 2), ('v', 2)]),
    'graddiv': ('(inner(grad(u), grad(v)) + div(u) * div(v)) * dx', [('u', 2), ('v', 2)]),
    'divp': ('div(u) * v * dx', [('u', 2), ('v', 1)]),
    'weighted': ('(c * inner(grad(u), grad(v)) + inner(dot(K, u), v)) * dx', [('u', 2), ('v', 2)]),
}


def test_vector_valued_forms_vs_reference(iga, golden):
    g = golden('vecforms')
    mk = iga.bspline.make_knots
    ann, cyl = _geo(iga, 'quarter_annulus'), _geo(iga, 'cylinder')
    kvs2 = (mk(2, 0., 1., 5), mk(3, 0., 1., 4))
    inp = _vec_inputs()
    for name, (form, bfuns) in _VEC_FORMS.items():
        args = {k: v for k, v in inp.items() if k in form}
        for layout in ('blocked', 'packed'):
            A = iga.assemble.assemble(form, kvs2, geo=ann, bfuns=bfuns, layout=layout, **args)
            ref = golden_csr(g, '%s_%s' % (name, layout))
            assert A.shape == ref.shape and rel_maxdiff(A, ref) <= RTOL, (name, layout)
        asm = iga.assemble.instantiate_assembler(form, kvs2, dict(args, geo=ann), bfuns)
        assert tuple(asm.num_components()) == tuple(g[name + '_numcomp']) and asm.arity == 2
        blocks = np.asarray(asm.multi_blocks(g[name + '_idx']))
        refb = g[name + '_blocks']
        assert blocks.shape == refb.shape and np.abs(blocks - refb).max() <= RTOL * np.abs(refb).max()
    A = iga.assemble.assemble('inner(as_matrix([[2,1],[0,0]]).dot(u), v) * dx', kvs2, geo=ann, bfuns=[('u', 2), ('v', 2)], layout='packed', format='bsr')
    assert A.format == 'bsr' and A.blocksize == (2, 2) and rel_maxdiff(A.tocsr(), golden_csr(g, 'nonsym_packed')) <= RTOL
    kvs3 = (mk(2, 0., 1., 3), mk(2, 0., 1., 2), mk(3, 0., 1., 2))
    A = iga.assemble.assemble('(inner(curl(u), curl(v)) + inner(u, v)) * dx', kvs3, geo=cyl, bfuns=[('u', 3), ('v', 3)])
    assert rel_maxdiff(A, golden_csr(g, 'curlcurl_blocked')) <= RTOL
    for name, form in (('fdiv', 'f * div(v) * dx'), ('gdotv', 'inner(gv, v) * dx')):
        args = {k: v for k, v in inp.items() if k in form}
        for layout in ('blocked', 'packed'):
            out = iga.assemble.assemble(form, kvs2, geo=ann, bfuns=[('v', 2)], layout=layout, **args)
            ref = g['%s_%s' % (name, layout)]
            assert out.shape == ref.shape and np.abs(out - ref).max() <= RTOL * np.abs(ref).max(), (name, layout)


def test_boundary_integrals_vs_reference(iga, golden):
    g = golden('vecforms')
    mk = iga.bspline.make_knots
    ann, cyl = _geo(iga, 'quarter_annulus'), _geo(iga, 'cylinder')
    kvb = (mk(3, 0., 1., 3), mk(2, 0., 1., 4), mk(3, 0., 1., 5))
    g3 = lambda x, y, z: 1.0 + x + 2 * y * z
    asm = iga.assemble.assemble

    def close(a, ref, what):
        assert a.shape == ref.shape, what
        assert np.abs(a - ref).max() <= RTOL * max(np.abs(ref).max(), 1e-300), what
    for side in ('left', 'right', 'bottom', 'top', 'front', 'back'):
        close(asm('v * ds', kvb, geo=cyl, boundary=side), g['bd3_v_' + side], side)
        close(asm('(g * v + inner(n, grad(v))) * ds', kvb, geo=cyl, boundary=side, g=g3), g['bd3_gv_' + side], side)
        close(asm('inner(v, n) * ds', kvb, bfuns=[('v', 3)], geo=cyl, boundary=side, layout='packed'), g['bd3_vn_' + side], side)
    # the literal checks of test/test_assemble.py:331-372
    assert np.allclose(asm('v * ds', kvb, geo=cyl, boundary='right').sum(), (2 * 2 * np.pi) / 4)
    assert np.allclose(asm('inner(v, n) * ds', kvb, bfuns=[('v', 3)], geo=cyl, boundary='left', layout='packed').sum(axis=(0, 1, 2)), [-1, -1, 0])
    for name, form, side in (('gradgrad_left', 'inner(grad(u), grad(v)) * ds', 'left'), ('gradgrad_top', 'inner(grad(u), grad(v)) * ds', 'top'),
                             ('tang_front', 'inner(cross(n, grad(u)), cross(n, grad(v))) * ds', 'front'), ('mass_right', 'u * v * ds', 'right'),
                             ('robin_back', '(g * u * v + inner(n, grad(u)) * v) * ds', 'back')):
        args = {'g': g3} if 'g *' in form else {}
        A = asm(form, kvb, geo=cyl, boundary=side, **args)
        ref = golden_csr(g, 'bd3_' + name)
        assert A.shape == ref.shape and rel_maxdiff(A, ref) <= RTOL, name
    # tangential part on the plane face 'front' = the 2D Laplacian of the quarter annulus (test/test_assemble.py:395-400)
    A = asm('inner(cross(n, grad(u)), cross(n, grad(v))) * ds', kvb, geo=cyl, boundary='front')
    assert rel_maxdiff(A, iga.assemble.stiffness(kvb[1:], geo=ann)) < 1e-11
    # 2D patches: the faces are 1D
    kvs2 = (mk(2, 0., 1., 5), mk(3, 0., 1., 4))
    g2 = lambda x, y: 1.0 + x * y
    for side in ('left', 'right', 'bottom', 'top'):
        close(asm('g * v * ds', kvs2, geo=ann, boundary=side, g=g2), g['bd2_v_' + side], side)
        close(asm('inner(v, n) * ds', kvs2, bfuns=[('v', 2)], geo=ann, boundary=side, layout='packed'), g['bd2_vn_' + side], side)
    for name, form, side in (('mass_left', 'u * v * ds', 'left'), ('mass_top', 'u * v * ds', 'top'), ('gradgrad_right', 'inner(grad(u), grad(v)) * ds', 'right'),
                             ('nitsche_bottom', '(inner(n, grad(u)) * v + g * u * v) * ds', 'bottom')):
        args = {'g': g2} if 'g *' in form else {}
        A = asm(form, kvs2, geo=ann, boundary=side, **args)
        ref = golden_csr(g, 'bd2_' + name)
        assert A.shape == ref.shape and rel_maxdiff(A, ref) <= RTOL, name
    sq = iga.geometry.unit_square()
    kq = 2 * (mk(3, 0., 1., 3),)
    for side, nv in (('left', [-1, 0]), ('right', [1, 0]), ('bottom', [0, -1]), ('top', [0, 1])):
        assert np.allclose(asm('inner(v, n) * ds', kq, bfuns=[('v', 2)], geo=sq, boundary=side, layout='packed').sum(axis=(0, 1)), nv)
    with pytest.raises(ValueError):
        asm('v * ds', kq, geo=sq, boundary='front')
    with pytest.raises(ValueError):
        asm('v * ds', kq, geo=sq)


def test_surface_integrals_vs_reference(iga, golden):
    """Integrals over a patch that is mapped into a space of one dimension more (test/test_assemble.py:314-330): faces of the
    quarter-annulus cylinder as 2D -> 3D NURBS surfaces, sides of the quarter annulus as curves.  Goldens: the reference's
    assemble() on the same strings with geo.boundary(side)."""
    g = golden('surface')
    mk = iga.bspline.make_knots
    cyl, ann = _geo(iga, 'cylinder'), _geo(iga, 'quarter_annulus')
    asm = iga.assemble.assemble
    kvs2 = (mk(3, 0., 1., 4), mk(2, 0., 1., 6))

    def close(a, ref, what):
        assert a.shape == ref.shape, what
        assert np.abs(a - ref).max() <= RTOL * np.abs(ref).max(), what
    for side in ('left', 'right', 'top', 'back'):
        geo = cyl.boundary(side)
        assert geo.sdim == 2 and geo.dim == 3
        close(asm('v * ds', kvs2, geo=geo), g['s3_v_' + side], side)
        close(asm('(1.0 + x[0] + 2 * x[1] * x[2]) * v * ds', kvs2, geo=geo), g['s3_xv_' + side], side)
        close(asm('inner(v, n) * ds', kvs2, geo=geo, bfuns=[('v', 3)], layout='packed'), g['s3_vn_' + side], side)
        A = asm('(2.5 + x[0]) * u * v * ds', kvs2, geo=geo)
        assert rel_maxdiff(A, golden_csr(g, 's3_mass_' + side)) <= RTOL, side
    # inner and outer mantle: r = 1 and r = 2, a quarter of the circle, height 1 (test/test_assemble.py:327-330)
    assert np.allclose(asm('v * ds', kvs2, geo=cyl.boundary('left')).sum(), 2 * np.pi / 4)
    assert np.allclose(asm('v * ds', kvs2, geo=cyl.boundary('right')).sum(), 2 * 2 * np.pi / 4)
    kv1 = (mk(3, 0., 1., 7),)
    for side in ('left', 'right', 'bottom', 'top'):
        geo = ann.boundary(side)
        close(asm('(1.0 + x[0] * x[1]) * v * ds', kv1, geo=geo), g['s2_v_' + side], side)
        close(asm('inner(v, n) * ds', kv1, geo=geo, bfuns=[('v', 2)], layout='packed'), g['s2_vn_' + side], side)
        assert rel_maxdiff(asm('u * v * ds', kv1, geo=geo), golden_csr(g, 's2_mass_' + side)) <= RTOL, side
    with pytest.raises(NotImplementedError):
        asm('inner(grad(u), grad(v)) * ds', kvs2, geo=cyl.boundary('left'))


@pytest.mark.parametrize('p,n', [(4, 7), (5, 6)])
def test_general_form_high_degree(iga, p, n):
    """Non-symmetric sweeps of degree >= 4 run with one type per group (k_stageA<..., ONE>, two-type groups split on the host):
    a full general form (diffusion tensor, convection, adjoint convection, reaction) equals the entry-wise kernel and its
    row slabs reproduce it bit for bit."""
    form = '(inner(dot(K, grad(u)), grad(v)) + inner(b, grad(u)) * v + u * inner(b, grad(v)) + c * u * v) * dx'
    inp = form_inputs()
    kv = iga.bspline.make_knots(p, 0., 1., n)
    kvs = (kv, kv, kv)
    cyl = _geo(iga, 'cylinder')
    asm = iga.assemblers.GeneralFormAssembler3D(kvs, cyl, form, inputs=inp)
    A = asm.patch.csr('form', algo='sumfact')
    E = asm.patch.csr('form', algo='entrywise')
    assert rel_maxdiff(A, E) <= RTOL
    N0 = kv.numdofs
    parts = [iga.assemblers.GeneralFormAssembler3D(kvs, cyl, form, inputs=inp, row0=r).patch.csr('form', algo='sumfact')
             for r in ((0, N0 // 2), (N0 // 2, N0))]
    assert abs(scipy.sparse.vstack(parts).tocsr() - A).max() == 0.0


def test_assembler_class_with_updatable_inputs(iga):
    """The high-level Assembler object (pyiga/assemble.py:958-1003; test/test_assemble.py:417-426)."""
    kvs = 2 * (iga.bspline.make_knots(2, 0., 1., 10),)
    geo = iga.geometry.quarter_annulus()
    A2 = iga.assemble.stiffness(kvs, geo)
    asm = iga.assemble.Assembler('inner(grad(u), grad(v)) * dx', kvs, geo=geo, symmetric=True, updatable=['geo'])
    assert rel_maxdiff(asm.assemble(), A2) <= RTOL
    with pytest.raises(RuntimeError):
        asm.assemble(f=geo)                                   # not an updatable field
    with pytest.raises(ValueError):
        iga.assemble.Assembler('inner(grad(u), grad(v)) * dx', kvs, geo=geo, updatable=['f'])   # f is not an input
    geo2 = iga.geometry.bspline_quarter_annulus()
    assert rel_maxdiff(asm.assemble(geo=geo2), iga.assemble.stiffness(kvs, geo2)) <= RTOL
    asm = iga.assemble.Assembler('c * u * v * dx', kvs, geo=geo, c=lambda x, y: 1.0 + x, updatable=['c'])
    M1 = asm.assemble()
    M2 = asm.assemble(c=lambda x, y: 2.0 + 2.0 * x)
    assert rel_maxdiff(M2, 2.0 * M1) <= RTOL


def test_ondemand_bbox_random_cases(iga):
    """Bounding-box assemblers on random spaces (degrees 1..4, repeated interior knots, 2D and 3D, NURBS / B-spline geometry): the
    rows of a random cluster of functions from a boxed assembler equal the whole-patch assembler's."""
    rng = np.random.default_rng(17)
    g = iga.geometry
    for case in range(12):
        d = 3 if case % 3 else 2
        kvs = []
        for k in range(d):
            p = int(rng.integers(1, 5))
            kv = iga.bspline.make_knots(p, 0.0, 1.0, int(rng.integers(3, 9)), mult=int(rng.integers(1, max(2, p))))
            kvs.append(kv)
        kvs = tuple(kvs)
        geo = (g.quarter_annulus() if case % 2 else g.bspline_quarter_annulus()) if d == 2 else (_geo(iga, 'cylinder') if case % 2 else g.twisted_box())
        cls = {2: (iga.assemblers.MassAssembler2D, iga.assemblers.StiffnessAssembler2D),
               3: (iga.assemblers.MassAssembler3D, iga.assemblers.StiffnessAssembler3D)}[d][case % 2]
        nd = [kv.numdofs for kv in kvs]
        centre = [int(rng.integers(0, n)) for n in nd]
        multi = np.stack([np.clip(c + rng.integers(-1, 2, 6), 0, n - 1) for c, n in zip(centre, nd)], 1)
        rows = np.unique(np.ravel_multi_index(multi.T, nd))
        bbox = iga.assemble.bbox_for_rows(kvs, rows)
        full, boxed = cls(kvs, geo), cls(kvs, geo, bbox=bbox)
        A = iga.assemble.assemble_partial_rows(full, rows)
        B = iga.assemble.assemble_partial_rows(boxed, rows)
        assert np.array_equal(A.indices, B.indices) and np.array_equal(A.indptr, B.indptr)
        assert np.isfinite(B.data).all()
        assert np.abs(A.data - B.data).max() <= RTOL * np.abs(A.data).max(), (case, d)


def test_boundary_integrals_divergence_theorem(iga):
    """Normals, surface measures and orientation of every face at once: sum over the faces of  F . n  against the volume
    integral of  div F  (the basis functions sum to one, so summing a load vector integrates its coefficient).  The two sides
    agree to the accuracy of the Gauss rule on the rational integrands of a NURBS map (1e-9 here); a wrong sign, normal or
    measure on any face is an O(1) error."""
    mk = iga.bspline.make_knots
    asm = iga.assemble.assemble
    kvs3 = (mk(2, 0., 1., 3), mk(3, 0., 1., 4), mk(2, 0., 1., 5))
    cyl = _geo(iga, 'cylinder')
    F3 = lambda x, y, z: (x * z, y * y, z * x + y)
    vol = asm('d * v * dx', kvs3, geo=cyl, d=lambda x, y, z: z + 2 * y + x).sum()
    sur = sum(asm('inner(F, n) * v * ds', kvs3, geo=cyl, boundary=s, F=F3).sum() for s in ('left', 'right', 'bottom', 'top', 'front', 'back'))
    assert abs(vol - sur) <= 1e-7 * abs(vol)
    for geo in (_geo(iga, 'quarter_annulus'), iga.geometry.bspline_quarter_annulus()):
        kvs2 = (mk(3, 0., 1., 6), mk(2, 0., 1., 7))
        F2 = lambda x, y: (x * y, y * y - x)
        vol = asm('d * v * dx', kvs2, geo=geo, d=lambda x, y: 3 * y).sum()
        sur = sum(asm('inner(F, n) * v * ds', kvs2, geo=geo, boundary=s, F=F2).sum() for s in ('left', 'right', 'bottom', 'top'))
        # (the B-spline annulus is an approximate circle: the theorem holds on whatever domain the map describes)
        assert abs(vol - sur) <= 1e-7 * abs(vol)


# ---------------------------------------------------------------------------------------------
# forms with second derivatives and parametric derivatives (pyiga_amd/pforms.py -> igx_patch_set_pform in passes)
def test_spline_hessians_vs_reference(iga, golden):
    """grid_hessian of B-spline and NURBS geometry maps against the reference's (pyiga/bspline.py:923-975,
    pyiga/geometry.py:125-150)."""
    g = golden('pforms')
    g2 = (g['hess_grid2_0'], g['hess_grid2_1'])
    g3 = (g['hess_grid3_0'], g['hess_grid3_1'], g['hess_grid3_2'])
    for key, gname, grid in (('hess_ann', 'quarter_annulus', g2), ('hess_bann', 'bspline_quarter_annulus', g2),
                             ('hess_cyl', 'cylinder', g3), ('hess_tbox', 'twisted_box', g3)):
        H = _geo(iga, gname).grid_hessian(grid)
        assert H.shape == g[key].shape
        assert np.abs(H - g[key]).max() <= 1e-12 * max(1.0, np.abs(g[key]).max()), key
    # scalar functions drop the component axis
    kv = iga.bspline.make_knots(3, 0.0, 1.0, 4)
    f = iga.bspline.BSplineFunc((kv, kv), np.arange(49.0).reshape(7, 7) ** 1.5)
    assert f.grid_hessian(g2).shape == (7, 5, 3)


@pytest.mark.parametrize('algo', ['sumfact', 'entrywise'])
def test_second_derivative_forms_vs_reference(iga, golden, algo, monkeypatch):
    """hess / Dx(times=2) / div(grad) / parametric derivatives through pyiga_amd.pforms and the device passes, against the
    matrices the reference compiled from the same strings (2D NURBS + B-spline annulus, 3D NURBS cylinder + twisted box)."""
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')
    g = golden('pforms')
    mk = iga.bspline.make_knots
    in2, in3 = pform_inputs2(), form_inputs()
    spaces2 = {'ann': ((mk(3, 0.0, 1.0, 4), mk(2, 0.0, 1.0, 5, mult=2)), 'quarter_annulus'),
               'bann': ((mk(4, 0.0, 1.0, 3), mk(4, 0.0, 1.0, 6)), 'bspline_quarter_annulus')}
    spaces3 = {'cyl_p2': ((mk(2, 0.0, 1.0, 3),) * 3, 'cylinder'),
               'tbox_mixed': ((mk(3, 0.0, 1.0, 2), mk(2, 0.0, 1.0, 4, mult=2), mk(2, 0.0, 1.0, 3)), 'twisted_box')}
    for dim, spaces, FS, inp in ((2, spaces2, PFORMS2, in2), (3, spaces3, PFORMS3, in3)):
        for sname, (kvs, gname) in spaces.items():
            geo = _geo(iga, gname)
            for fname, (form, names) in FS.items():
                R = golden_csr(g, 'd%d_%s_%s' % (dim, sname, fname))
                asm = iga.assemble.instantiate_assembler(form, kvs, dict(geo=geo, **{k: inp[k] for k in names}))
                assert isinstance(asm, iga.assemblers._ParametricFormAssembler)
                A = asm.assemble_csr(algo=algo)
                assert A.nnz == R.nnz and np.array_equal(A.indices, R.indices) and not np.isnan(A.data).any()
                assert rel_maxdiff(A, R) <= RTOL, (sname, fname, algo, rel_maxdiff(A, R))
                if algo == 'entrywise':
                    rng = np.random.default_rng(6)
                    idx = rng.integers(0, R.shape[0], (50, 2)).astype(np.uintp)
                    assert np.abs(asm.multi_entries(idx) - np.asarray(R[idx[:, 0], idx[:, 1]]).ravel()).max() <= RTOL * np.abs(R.data).max()
                # the default tables are back: the built-in forms still work on the same patch
                assert asm.patch.assemble('mass').shape == (R.nnz,)
    kv = mk(3, 0.0, 1.0, 4)
    A = iga.assemble.assemble(PFORMS2['biharm'][0], (kv, mk(2, 0.0, 1.0, 5, mult=2)), geo=_geo(iga, 'quarter_annulus'))
    assert rel_maxdiff(A, golden_csr(g, 'd2_ann_biharm')) <= RTOL and abs(A - A.T).max() <= 1e-12 * abs(A).max()
    for bad in ('Dx(u, 0, times=3) * v * dx', 'Dx(c * u, 0) * v * dx', 'Dx(Dx(u, 0, parametric=True), 1) * v * dx', 'hess(u) * v * dx'):
        with pytest.raises(NotImplementedError):
            iga.assemble.assemble(bad, (kv, kv), geo=_geo(iga, 'quarter_annulus'), c=lambda x, y: x)


def test_basis_orders_guard(iga):
    """With derivative orders other than (value, first derivative) in the basis tables only a parametric jet form assembles."""
    kv = iga.bspline.make_knots(3, 0.0, 1.0, 5)
    asm = iga.assemblers.MassAssembler2D((kv, kv), _geo(iga, 'quarter_annulus'))
    M = asm.patch.assemble('mass')
    asm.patch.set_basis_orders((0, 1), (2, 2))
    with pytest.raises(RuntimeError):
        asm.patch.assemble('mass')
    with pytest.raises(RuntimeError):
        asm.patch.set_basis_orders((1, 0), (1, 2))
    asm.patch.set_basis_orders()
    assert np.array_equal(asm.patch.assemble('mass'), M)


def test_forms_compiled_at_run_time(iga, golden, tmp_path, monkeypatch):
    """The coefficients of a form string -- and of the callables it names -- are traced into C, ONE kernel per form is generated,
    compiled with hiprtc and cached on disk (igx_patch_set_form_expr; the reference: one compiled module per form,
    pyiga/compile.py:58-73,120-132); the matrices are the reference's, the host-sampled path (IGX_FORM_RTC=0, or an input the
    tracer cannot follow) gives the same ones; a plain callable as the convection-diffusion coefficient goes the same way."""
    monkeypatch.setenv('IGX_CACHE_DIR', str(tmp_path / 'cache'))
    g = golden('forms')
    inp = form_inputs()
    kvs, gname = _form_spaces(iga)['tbox_mixed']
    geo = _geo(iga, gname)
    for n, (fname, (form, names)) in enumerate(FORMS.items()):
        R = golden_csr(g, 'tbox_mixed_%s' % fname)
        kw = dict(geo=geo, **{k: inp[k] for k in names})
        asm = iga.assemble.instantiate_assembler(form, kvs, kw)
        assert asm.compiled and asm.coeff_cache_hit is False
        # the expressions live INSIDE the generated field kernel: no coefficient arrays on the device
        assert asm.patch.form_generated()
        A = asm.assemble_csr()
        assert rel_maxdiff(A, R) <= RTOL, (fname, rel_maxdiff(A, R))
        again = iga.assemble.instantiate_assembler(form, kvs, kw)
        assert again.compiled and again.coeff_cache_hit is True and np.array_equal(again.assemble_csr().data, A.data)
        monkeypatch.setenv('IGX_FORM_RTC', '0')
        sampled = iga.assemble.instantiate_assembler(form, kvs, kw)
        monkeypatch.delenv('IGX_FORM_RTC')
        assert not sampled.compiled and not sampled.patch.form_generated() and rel_maxdiff(sampled.assemble_csr(), A) <= 1e-13
    assert len(os.listdir(tmp_path / 'cache')) == len(FORMS)
    # an input the tracer cannot follow: sampled on the host, same interface
    step = lambda x, y, z: np.where(x + y > 1.0, 2.0, 1.0)
    asm = iga.assemble.instantiate_assembler('c * u * v * dx', kvs, dict(geo=geo, c=step))
    assert not asm.compiled
    M = asm.assemble_csr()
    assert abs(M - M.T).max() <= 1e-14 * abs(M).max() and M.sum() > 0
    # transcendental coefficients: device libm against numpy
    w = lambda x, y, z: np.exp(-((x - 0.5) ** 2 + y ** 3) / 0.7) * np.sqrt(1.0 + z * z) + np.cos(x * y) / (2.0 + np.sin(z))
    form = '(w * inner(grad(u), grad(v)) + w**2 * u * v) * dx'
    a1 = iga.assemble.instantiate_assembler(form, kvs, dict(geo=geo, w=w))
    monkeypatch.setenv('IGX_FORM_RTC', '0')
    a0 = iga.assemble.instantiate_assembler(form, kvs, dict(geo=geo, w=w))
    assert a1.compiled and not a0.compiled and rel_maxdiff(a1.assemble_csr(), a0.assemble_csr()) <= 1e-13
    # convection-diffusion: a plain callable is traced and compiled like an ExprCoefficient
    kv = iga.bspline.make_knots(3, 0.0, 1.0, 6)
    cyl = _geo(iga, 'cylinder')
    dc = lambda x, y, z: 2.0 + np.sin(x + z)
    C0 = iga.assemblers.ConvDiffAssembler3D((kv, kv, kv), cyl, dc).assemble_csr()
    monkeypatch.delenv('IGX_FORM_RTC')
    c1 = iga.assemblers.ConvDiffAssembler3D((kv, kv, kv), cyl, dc)
    assert getattr(c1, 'coeff_traced', False) and rel_maxdiff(c1.assemble_csr(), C0) <= 1e-13


@pytest.mark.parametrize('p', [6, 7])
def test_high_degree_sum_factorisation(iga, oracle, p):
    """Degrees 6 and 7 run through the sum-factorised stage kernels (IGX_MAX_SF_DEGREE = 7): against the oracle and the
    entry-wise kernels, 2D and 3D, symmetric forms, convection-diffusion, unequal degrees and repeated knots."""
    mk = iga.bspline.make_knots
    cyl, ann = _geo(iga, 'cylinder'), _geo(iga, 'quarter_annulus')
    for dim, kvs, geo, ogeo in ((2, (mk(p, 0.0, 1.0, 9), mk(p, 0.0, 1.0, 12)), ann, oracle.geo_quarter_annulus()),
                                (3, (mk(p, 0.0, 1.0, 4), mk(p, 0.0, 1.0, 5), mk(p, 0.0, 1.0, 3)), cyl, oracle.geo_cylinder()),
                                (3, (mk(p, 0.0, 1.0, 3), mk(2, 0.0, 1.0, 6, mult=2), mk(p - 1, 0.0, 1.0, 4)), cyl, oracle.geo_cylinder())):
        okvs = tuple(oracle.KnotVector(kv.kv, kv.p) for kv in kvs)
        for kind in ('mass', 'stiffness'):
            asm = {('mass', 2): iga.assemblers.MassAssembler2D, ('stiffness', 2): iga.assemblers.StiffnessAssembler2D,
                   ('mass', 3): iga.assemblers.MassAssembler3D, ('stiffness', 3): iga.assemblers.StiffnessAssembler3D}[(kind, dim)](kvs, geo)
            A = asm.assemble_csr(algo='sumfact')
            assert asm.patch.timing()['algo_used'] == 2
            R = oracle.assemble(kind, okvs, ogeo, nthreads=8)
            assert np.array_equal(A.indices, R.indices) and rel_maxdiff(A, R) <= RTOL, (p, dim, kind, rel_maxdiff(A, R))
            assert abs(A - A.T).max() == 0.0
            assert rel_maxdiff(asm.assemble_csr(algo='entrywise'), R) <= RTOL
        if dim == 3:
            coeff = lambda x, y, z: 1.0 + x * y
            C = iga.assemblers.ConvDiffAssembler3D(kvs, geo, coeff).assemble_csr(algo='sumfact')
            R = oracle.assemble_nonsymmetric('convdiff', okvs, ogeo, coeff=coeff, nthreads=8)
            assert rel_maxdiff(C, R) <= RTOL, (p, 'convdiff', rel_maxdiff(C, R))


def test_load_vector_function_compiled(iga, tmp_path, monkeypatch):
    """inner_products / the L2 functional assemblers with a plain callable: the function is traced into C and evaluated at
    the Gauss points on the device (igx_patch_eval_expr_d) -- physical and parametric coordinates, 2D and 3D, row slabs --
    and gives what sampling on the host gives; spline functions and untraceable callables are sampled as before."""
    monkeypatch.setenv('IGX_CACHE_DIR', str(tmp_path / 'cache'))
    mk = iga.bspline.make_knots
    f3 = lambda x, y, z: np.cos(x) * np.exp(y) * np.sin(z) + 0.25 * x * y * z
    f2 = lambda x, y: np.exp(-x) * np.sin(3.0 * y) + x ** 2
    cases = [((mk(3, 0.0, 1.0, 6), mk(2, 0.0, 1.0, 5), mk(4, 0.0, 1.0, 4)), _geo(iga, 'cylinder'), f3),
             ((mk(3, 0.0, 1.0, 9), mk(2, 0.0, 1.0, 7, mult=2)), _geo(iga, 'quarter_annulus'), f2)]
    for kvs, geo, f in cases:
        for physical in (True, False):
            got = iga.assemble.inner_products(kvs, f, f_physical=physical, geo=geo)
            monkeypatch.setenv('IGX_FORM_RTC', '0')
            ref = iga.assemble.inner_products(kvs, f, f_physical=physical, geo=geo)
            monkeypatch.delenv('IGX_FORM_RTC')
            assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max(), (len(kvs), physical)
        got = iga.assemble.inner_products(kvs, f)                     # parameter domain, no geometry
        monkeypatch.setenv('IGX_FORM_RTC', '0')
        ref = iga.assemble.inner_products(kvs, f)
        monkeypatch.delenv('IGX_FORM_RTC')
        assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()
    # the one-kernel path (geometry + weight + function: igx_load_vector_expr) against the two-array path (function values by a
    # generated kernel, weight field by the library, both read back: igx_patch_eval_expr_d + igx_load_vector_d), slabs included
    # (the first two cases are refused by the one-kernel path -- unequal degrees of the last two axes, 2D -- and
    # load_vector_expr falls back to the two arrays: only the third, with equal mid and last degrees, runs igx_lv12_expr)
    import ctypes
    fused = ((mk(2, 0.0, 1.0, 5), mk(3, 0.0, 1.0, 6), mk(3, 0.0, 1.0, 4)), _geo(iga, 'cylinder'), f3)
    for kvs, geo, f in cases + [fused]:
        from pyiga_amd import symbolic
        src = symbolic.trace_function(f, len(kvs))
        N0 = kvs[0].numdofs
        for row0 in (None, (1, N0 - 2)):
            patch = iga.assemblers.DevicePatch(kvs, geo, row0=row0)
            for par in (False, True):
                if kvs is fused[0]:
                    direct = np.empty(patch.row_range[1] - patch.row_range[0])
                    rc = iga._lib.load().igx_load_vector_expr(patch.handle, src.encode(), 1 if par else 0, iga._lib.dptr(direct), ctypes.byref(ctypes.c_int(0)))
                    assert rc == iga._lib.IGX_OK, (row0, par, rc)
                    assert patch.timing()['n_launches'] == 2
                one = patch.load_vector_expr(src, parametric=par)
                if kvs is fused[0]:
                    assert np.array_equal(one.ravel(), direct)
                patch.eval_function_expr(src, parametric=par)
                two = patch.load_vector_resident(to_host=True)
                assert one.shape == two.shape and np.abs(one - two).max() <= 1e-13 * np.abs(two).max(), (len(kvs), row0, par)
            patch.close()
    kvs, geo, f = cases[0]
    cls = iga.assemblers.L2FunctionalAssemblerPhys3D
    whole = cls(kvs, geo, f)
    assert whole._fexpr is not None
    v = whole.assemble_vector()
    N0 = kvs[0].numdofs
    parts = [cls(kvs, geo, f, row0=(a, b)).assemble_vector() for a, b in ((0, N0 // 2), (N0 // 2, N0))]
    assert np.array_equal(np.concatenate(parts, axis=0), v)
    step = lambda x, y, z: np.where(x > 1.2, 1.0, 0.5 + 0.0 * y * z)
    assert cls(kvs, geo, step)._fexpr is None and np.isfinite(cls(kvs, geo, step).assemble_vector()).all()
    spline = iga.bspline.BSplineFunc(kvs, np.arange(float(np.prod([kv.numdofs for kv in kvs]))))
    assert iga.assemblers.L2FunctionalAssembler3D(kvs, geo, spline)._fexpr is None


def test_auto_falls_back_to_entry_kernels(iga):
    """A shape the stage kernels refuse (here: more outer pairs than a launch grid has rows) is assembled by the entry-wise
    kernels when the caller leaves the algorithm to the library; an explicit request for the sum-factorised path keeps the error."""
    mk = iga.bspline.make_knots
    kvs = (mk(4, 0.0, 1.0, 14000), mk(1, 0.0, 1.0, 2), mk(2, 0.0, 1.0, 2))
    geo = iga.geometry.unit_cube()
    asm = iga.assemblers.MassAssembler3D(kvs, geo)
    with pytest.raises(RuntimeError):
        asm.assemble_csr(algo='sumfact')
    A = asm.assemble_csr()
    assert asm.patch.timing()['algo_used'] == 1
    E = asm.assemble_csr(algo='entrywise')
    assert np.array_equal(A.data, E.data) and abs(A - A.T).max() == 0.0
    assert abs(A.sum() - 1.0) <= 1e-12                    # the mass matrix of a partition of unity on the unit cube


def test_functional_form_strings_compiled(iga, golden, monkeypatch):
    """Arity-1 form strings with traceable inputs: the coefficients of v and grad(v) are compiled for the device
    (igx_load_vector_jet_expr) -- the reference's vectors, and the host-sampled path gives the same ones."""
    g = golden('forms')
    mk = iga.bspline.make_knots
    kv2 = (mk(3, 0.0, 1.0, 6), mk(2, 0.0, 1.0, 5))
    ann = _geo(iga, 'quarter_annulus')
    b2 = lambda x, y: (y * np.ones_like(x * y), (1.0 - x) * np.ones_like(x * y))
    form, kw = '(f * v + inner(b, grad(v))) * dx', dict(f=lambda x, y: x * y ** 2, b=b2)
    asm = iga.assemble.instantiate_assembler(form, kv2, dict(geo=ann, **kw))
    assert asm._jet_exprs is not None
    got = asm.assemble_vector()
    assert _close(got, g['funcgrad_d2'], 1e-13)
    monkeypatch.setenv('IGX_FORM_RTC', '0')
    ref = iga.assemble.instantiate_assembler(form, kv2, dict(geo=ann, **kw))
    assert ref._jet_exprs is None and np.abs(ref.assemble_vector() - got).max() <= 1e-13 * np.abs(got).max()
    monkeypatch.delenv('IGX_FORM_RTC')
    inp = form_inputs()
    kvs, gname = _form_spaces(iga)['tbox_mixed']
    v3 = iga.assemble.assemble('inner(b, grad(v)) * dx', kvs, geo=_geo(iga, gname), b=inp['b'])
    assert _close(v3, g['funcgrad_d3'], 1e-13)
    step = iga.assemble.instantiate_assembler('c * v * dx', kv2, dict(geo=ann, c=lambda x, y: np.where(x > 1.0, 1.0, 2.0 + 0.0 * y)))
    assert step._jet_exprs is None and np.isfinite(step.assemble_vector()).all()


def test_without_the_run_time_compiler_everything_still_assembles(iga, monkeypatch, tmp_path):
    """run-time compilation is the default for form strings, traced callables and functionals; on a box without
    libhiprtc (IGX_NO_HIPRTC, an empty cache) every one of those calls must fall through to host sampling -- same results."""
    mk = iga.bspline.make_knots
    kvs = (mk(2, 0., 1., 5), mk(2, 0., 1., 4), mk(2, 0., 1., 6))
    geo = _geo(iga, 'cylinder')

    def coef(x, y, z):
        return 1.0 + x * y + np.sin(z)

    def run():
        A = iga.assemble.assemble('(c * inner(grad(u), grad(v)) + u * v) * dx', kvs, geo=geo, c=coef)
        b = iga.assemble.inner_products(kvs, coef, f_physical=True, geo=geo)
        f = iga.assemble.assemble('(c * v + inner(b, grad(v))) * dx', kvs, geo=geo, c=coef, b=lambda x, y, z: (1.0 + 0 * x, x, y * z))
        C = iga.assemblers.ConvDiffAssembler3D(kvs, geo, coef).assemble_csr()
        return A, b, f, C
    ref = run()
    monkeypatch.setenv('IGX_NO_HIPRTC', '1')
    monkeypatch.setenv('IGX_CACHE_DIR', str(tmp_path / 'empty_cache'))
    out = run()
    for r, o in zip(ref, out):
        r = r.toarray() if hasattr(r, 'toarray') else np.asarray(r)
        o = o.toarray() if hasattr(o, 'toarray') else np.asarray(o)
        assert r.shape == o.shape and np.abs(r - o).max() <= 1e-13 * np.abs(r).max()


def test_run_time_compiler_errors_are_told_apart(iga, monkeypatch, tmp_path):
    """(1) 'no run-time compiler' (IGX_ERR_NORTC), 'the expression does not compile' (IGX_ERR_COMPILE) and 'the kernel
    does not serve this patch' (IGX_ERR_UNSUPPORTED) are different codes -- the Python side falls back to host sampling for these
    and for nothing else (a device failure must surface); (2) igx_load_vector_expr asks whether it applies BEFORE it touches the
    weight field; (3) an expression that could end the construct it is pasted into is refused (IGX_ERR_ARG) before anything is
    generated."""
    from pyiga_amd import _lib
    mk = iga.bspline.make_knots
    kvs = (mk(2, 0., 1., 5), mk(2, 0., 1., 4), mk(2, 0., 1., 6))
    patch = iga.assemblers.DevicePatch(kvs, _geo(iga, 'cylinder'))
    good = patch.load_vector_expr('x + y * z')
    for bad in ('x + y\n+ z', 'x // y', 'x + \\\ny', 'x; y', 'x /* y */', '1) ; } void f() { (0'):
        with pytest.raises(_lib.IgxError) as ei:
            patch.load_vector_expr(bad)
        assert ei.value.code == _lib.IGX_ERR_ARG, (bad, ei.value.code)
        with pytest.raises(_lib.IgxError) as ei:
            patch.set_coeff_expr(bad)
        assert ei.value.code == _lib.IGX_ERR_ARG, (bad, ei.value.code)
    with pytest.raises(_lib.IgxError) as ei:
        patch.load_vector_expr('x + undefined_name')
    assert ei.value.code == _lib.IGX_ERR_COMPILE
    assert np.array_equal(patch.load_vector_expr('x + y * z'), good)           # the patch is intact after the refusals
    patch.close()
    monkeypatch.setenv('IGX_NO_HIPRTC', '1')
    monkeypatch.setenv('IGX_CACHE_DIR', str(tmp_path / 'empty_cache'))
    patch = iga.assemblers.DevicePatch(kvs, _geo(iga, 'cylinder'))
    with pytest.raises(_lib.IgxError) as ei:
        patch.load_vector_expr('x + y * z + 1')
    assert ei.value.code == _lib.IGX_ERR_NORTC
    patch.close()
    # what may fall back and what may not
    ok, dev = _lib.IgxError('x'), _lib.IgxError('y')
    ok.code, dev.code = _lib.IGX_ERR_NORTC, _lib.IGX_ERR_HIP
    with pytest.warns(RuntimeWarning):
        assert _lib.sampled_fallback(ok, 'test input %d' % id(ok))
    assert not _lib.sampled_fallback(dev, 'test input')
    dev.code = _lib.IGX_ERR_NOMEM
    assert not _lib.sampled_fallback(dev, 'test input')


def test_kronecker_shortcut_refuses_degrees_beyond_its_row_buffers(iga, monkeypatch):
    """k_kron3 stages one 2D row of at most 128 entries per wave; degree 6 on the cross-section axes (13 * 13 = 169)
    must be refused by the library and the opt-in path must fall back to the general chain (same matrix)."""
    mk = iga.bspline.make_knots
    kvs = (mk(2, 0., 1., 3), mk(6, 0., 1., 2), mk(6, 0., 1., 2))
    geo = _geo(iga, 'cylinder')
    A = iga.assemble.stiffness(kvs, geo)
    monkeypatch.setenv('IGX_SEPARABLE', '1')
    B = iga.assemble.stiffness(kvs, geo)
    assert (A != B).nnz == 0 or abs(A - B).max() <= 1e-13 * abs(A).max()


def test_fused_stage_with_unequal_degrees_and_repeated_knots(iga, monkeypatch):
    """Round 5: k_bf3 serves every symmetric 3D patch with single knots on the LAST axis -- degrees of the swept and the last
    axis one below nqp = max degree + 1 (pyiga/assemblers.pyx:1338), repeated knots on the swept axis (equal degrees) and on
    axis 0.  Against the entry-wise kernels (the reference's loop nest), exactly symmetric, every value written, the fused
    stage really ran, and row slabs reproduce the patch bit for bit.  (Every instantiation of k_bf3, one case each:
    tests/_bf3_cases.py, test_every_bf3_instantiation_vs_oracle.)"""
    mk = iga.bspline.make_knots
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')

    def rep(p, n, m, at=None):                 # make_knots with the interior knots of index `at` repeated m times in all
        kv = mk(p, 0., 1., n)
        inner = np.unique(kv.kv)[1:-1]
        extra = np.repeat(inner if at is None else inner[list(at)], m - 1)
        return iga.bspline.KnotVector(np.sort(np.concatenate([kv.kv, extra])), p)
    cases = [((mk(3, 0., 1., 4), mk(2, 0., 1., 9), mk(3, 0., 1., 7)), 'twisted_box', True),          # (P1, P2, Q) = (3, 4, 4)
             ((mk(4, 0., 1., 3), mk(4, 0., 1., 6), mk(3, 0., 1., 11)), 'cylinder', True),            # (5, 4, 5)
             ((mk(4, 0., 1., 3), mk(3, 0., 1., 8), mk(3, 0., 1., 9)), 'cylinder', True),             # (4, 4, 5)
             ((mk(2, 0., 1., 5), mk(1, 0., 1., 6), mk(2, 0., 1., 4)), 'twisted_box', True),          # (2, 3, 3)
             ((mk(3, 0., 1., 4), rep(3, 7, 2), mk(3, 0., 1., 9)), 'cylinder', True),                 # double knots on the swept axis
             ((mk(4, 0., 1., 3), rep(4, 6, 3, at=(1, 3)), mk(4, 0., 1., 40)), 'cylinder', True),     # triple knots, four tiles
             ((rep(2, 5, 2), rep(2, 6, 2, at=(0, 4)), mk(2, 0., 1., 8)), 'twisted_box', True),       # repeated knots on axes 0 and 1
             ((mk(3, 0., 1., 4), mk(3, 0., 1., 5), rep(3, 6, 2)), 'cylinder', True),                 # repeated knots on the LAST axis only: through the twin (round 6)
             ((mk(3, 0., 1., 4), rep(3, 5, 2, at=(1,)), rep(3, 6, 2)), 'cylinder', False),           # ... on the mid AND the last axis: stage kernels
             ((mk(4, 0., 1., 3), mk(2, 0., 1., 5), mk(4, 0., 1., 6)), 'cylinder', True),             # two degrees below nqp on the swept axis (round 6): (3, 5, 5)
             ((mk(4, 0., 1., 3), mk(4, 0., 1., 5), mk(2, 0., 1., 14)), 'cylinder', True),            # ... on the last axis: (5, 3, 5)
             ((mk(3, 0., 1., 4), mk(1, 0., 1., 6), mk(2, 0., 1., 9)), 'twisted_box', True)]          # (2, 3, 4)
    for kvs, gname, fused3 in cases:
        for kind in ('stiffness', 'mass'):
            patch = iga.assemblers.DevicePatch(kvs, _geo(iga, gname))
            A = patch.csr(kind, algo='sumfact')
            path = patch.last_path()
            E = patch.csr(kind, algo='entrywise')
            patch.close()
            tag = (kind, [kv.p for kv in kvs], [kv.numdofs for kv in kvs], sorted(path))
            assert ('bf3' in path and 'both' in path) == fused3, tag
            assert ('twin' in path) == (fused3 and kvs[2].numdofs > kvs[2].numspans + kvs[2].p), tag
            assert not np.isnan(A.data).any(), tag
            assert abs(A - A.T).max() == 0.0, tag
            assert rel_maxdiff(A, E) <= RTOL, (tag, rel_maxdiff(A, E))
            # ... and against the CPU oracle (the reference's loop nest restated, pinned to reference-made matrices of these very
            # shapes: golden_matrices.npz d3_midmult / d3_p443 / d3_p433 / d3_lastmult / d3_p424), not only HIP against HIP
            from oracle import iga_oracle as orc
            okvs = tuple(orc.KnotVector(np.asarray(kv.kv), kv.p) for kv in kvs)
            R = orc.assemble(kind, okvs, orc.geo_cylinder() if gname == 'cylinder' else orc.geo_twisted_box())
            assert A.nnz == R.nnz and rel_maxdiff(A, R) <= RTOL, (tag, rel_maxdiff(A, R))
            N0 = kvs[0].numdofs
            parts = []
            for lo, hi in ((0, N0 // 3), (N0 // 3, N0 - 1), (N0 - 1, N0)):
                if hi > lo:
                    sl = iga.assemblers.DevicePatch(kvs, _geo(iga, gname), row0=(lo, hi))
                    parts.append(sl.assemble(kind, algo='sumfact', to_host=True).copy())
                    sl.close()
            assert np.array_equal(np.concatenate(parts), A.data), tag


# ---------------------------------------------------------------------------------------------
# every compiled k_bf3 instantiation (tests/_bf3_cases.py; tests/test_bf3_coverage_cpu.py ties the table to fused3.hip)
def _bf3_coeff(x, y, z):
    return 1.0 + x * x + 0.5 * z


def _bf3_patch_kvs(iga, axes):
    return tuple(iga.bspline.KnotVector(bc.axis_knots(a), a[0]) for a in axes)


def _bf3_oracle(kind, kvs, gname):
    from oracle import iga_oracle as orc
    okvs = tuple(orc.KnotVector(np.asarray(kv.kv), kv.p) for kv in kvs)
    geo = orc.geo_cylinder() if gname == 'cylinder' else orc.geo_twisted_box()
    if kind == 'convdiff':
        return orc.assemble_nonsymmetric('convdiff', okvs, geo, coeff=_bf3_coeff, nthreads=8)
    return orc.assemble(kind, okvs, geo, nthreads=8)


def _bf3_assemble(iga, kind, kvs, gname, algo, row0=None):
    """(CSR matrix, last_path) of one patch or row slab."""
    geo = _geo(iga, gname)
    if kind == 'convdiff':
        asm = iga.assemblers.ConvDiffAssembler3D(kvs, geo, _bf3_coeff, row0=row0)
        A = asm.assemble_csr(algo=algo)
        path = asm.patch.last_path()
        asm.patch.close()
        return A, path
    patch = iga.assemblers.DevicePatch(kvs, geo, row0=row0)
    A = patch.csr(kind, algo=algo)
    path = patch.last_path()
    patch.close()
    return A, path


def _bf3_check_vs_oracle(A, R, kvs, kind, tag, symmetric=None):
    """Every value written, exact symmetry, the reference's pattern, the oracle's values.  The pattern is the structural one
    (MLStructure, oracle.full_pattern): the oracle's matrix is a sum of two scipy matrices, which drops entries that are
    exactly zero -- those of two functions whose supports share only an empty-width span, as make_knots makes for some n
    (bspline.make_knots: n = 49 gives a last interior knot of 1 - 1e-16)."""
    from oracle import iga_oracle as orc
    assert not np.isnan(A.data).any(), tag                    # every value written (IGX_DEBUG_POISON)
    if (kind != 'convdiff') if symmetric is None else symmetric:
        assert abs(A - A.T).max() == 0.0, tag
    I, J = orc.full_pattern(tuple(orc.KnotVector(np.asarray(kv.kv), kv.p) for kv in kvs))
    P = scipy.sparse.csr_matrix((np.ones(len(I)), (I, J)), shape=R.shape)
    P.sort_indices()
    assert A.shape == R.shape and np.array_equal(A.indptr, P.indptr) and np.array_equal(A.indices, P.indices), tag
    assert rel_maxdiff(A, R) <= RTOL, (tag, rel_maxdiff(A, R))


@pytest.mark.parametrize('case', bc.BF3_CASES, ids=[c.id for c in bc.BF3_CASES])
def test_every_bf3_instantiation_vs_oracle(iga, case, monkeypatch):
    """Every k_bf3 instantiation launch_bf3 can pick -- 27 (P1, P2, Q) x {mass, stiffness}, the convection-diffusion form at
    equal degrees, repeated knots on the swept axis (MULT) and on the last axis (TR, the twin) for the three forms -- on a small
    patch shaped for the edges (tests/_bf3_cases.py): the intended kernel ran (not a fallback), every value written, exact
    symmetry, the pattern and the values of the CPU oracle (the reference's loop nest), the entry-wise kernels, and -- one case
    per (P1, P2, Q) -- row slabs of axis 0 bit for bit."""
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')
    kind, key = case.kind, case.key
    kvs = _bf3_patch_kvs(iga, case.axes)
    A, path = _bf3_assemble(iga, kind, kvs, case.geo, 'sumfact')
    tag = (case.id, key, sorted(path))
    assert 'bf3' in path and ('twin' in path) == key.tr, tag
    if kind != 'convdiff':
        assert 'both' in path, tag
    _bf3_check_vs_oracle(A, _bf3_oracle(kind, kvs, case.geo), kvs, kind, tag)
    E, _ = _bf3_assemble(iga, kind, kvs, case.geo, 'entrywise')
    assert rel_maxdiff(A, E) <= RTOL, (tag, rel_maxdiff(A, E))
    if not case.slabs:
        return
    N0 = kvs[0].numdofs
    cuts = sorted(set([0, 1, N0 // 2, N0]))
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        S, spath = _bf3_assemble(iga, kind, kvs, case.geo, 'sumfact', row0=(lo, hi))
        assert 'bf3' in spath and ('twin' in spath) == key.tr, (tag, lo, hi, sorted(spath))
        parts.append(S)
    V = scipy.sparse.vstack(parts).tocsr()
    assert np.array_equal(V.indptr, A.indptr) and np.array_equal(V.indices, A.indices) and np.array_equal(V.data, A.data), (tag, 'slabs')


@pytest.mark.parametrize('axes01,p2,gname,kind', bc.EDGE_SWEEPS, ids=['%s-p%d%d%d' % (s[3], s[0][0][0], s[0][1][0], s[1]) for s in bc.EDGE_SWEEPS])
def test_bf3_tile_edges_along_the_last_axis(iga, axes01, p2, gname, kind, monkeypatch):
    """k_bf3 cuts the last axis into tiles of RMAX rows (BF3Geom::rmax, fused3.hip): the dof count of the last axis runs over
    2 p + 1 .. 2 RMAX + 2 -- one, two and three tiles, every position of the last tile's edge -- against the CPU oracle, every
    value written."""
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')
    spans, rmax = bc.edge_sweep_sizes(axes01, p2, kind)
    keys = set()
    for n2 in spans:
        axes = tuple(axes01) + ((p2, n2, 1),)
        key = bc.bf3_key(axes, kind)
        keys.add(key)
        kvs = _bf3_patch_kvs(iga, axes)
        A, path = _bf3_assemble(iga, kind, kvs, gname, 'sumfact')
        tag = (kind, key, kvs[2].numdofs, rmax, sorted(path))
        assert key is not None and 'bf3' in path and 'twin' not in path, tag
        _bf3_check_vs_oracle(A, _bf3_oracle(kind, kvs, gname), kvs, kind, tag)
    assert len(keys) == 1 and kvs[2].numdofs >= 2 * rmax + 2


@pytest.mark.parametrize('last_rep', [1, 2], ids=['single-knots', 'twin'])
def test_failed_set_form_expr_keeps_the_previous_form(iga, last_rep, monkeypatch, tmp_path):
    """A call of igx_patch_set_form_expr that fails (the expressions do not compile: IGX_ERR_COMPILE; no run-time compiler:
    IGX_ERR_NORTC) leaves the previous form in place for EVERY algorithm: the fast chain's coefficient table (of the patch and
    of its axis-exchanged twin) as well as the field kernel of the entry-wise path."""
    import ctypes
    from pyiga_amd import _lib
    mk = iga.bspline.make_knots
    kvs = (mk(2, 0., 1., 3), mk(3, 0., 1., 4), iga.bspline.KnotVector(bc.axis_knots((3, 5, last_rep)), 3))
    patch = iga.assemblers.DevicePatch(kvs, _geo(iga, 'cylinder'))

    def table(c0, c1, bad=None):
        t = [[None] * 4 for _ in range(4)]
        t[0][0] = c0
        for k in range(1, 4):
            t[k][k] = c1
        if bad:
            t[1][1] = bad
        return t

    def set_raw(t):
        exprs = (ctypes.c_char_p * 16)()
        for r in range(4):
            for s in range(4):
                if t[r][s] is not None:
                    exprs[4 * r + s] = t[r][s].encode()
        hit = ctypes.c_int(0)
        return _lib.load().igx_patch_set_form_expr(patch.handle, exprs, ctypes.byref(hit))

    def both():
        A = patch.csr('form', algo='sumfact')
        path = patch.last_path()
        assert 'bf3' in path and ('twin' in path) == (last_rep > 1), sorted(path)
        return A, patch.csr('form', algo='entrywise')

    patch.set_form_expr(table('1.0', '2.0'))
    A_old, E_old = both()
    assert rel_maxdiff(A_old, E_old) <= RTOL
    # no run-time compiler: a table of constants the fast chain could take without compiling anything
    monkeypatch.setenv('IGX_NO_HIPRTC', '1')
    monkeypatch.setenv('IGX_CACHE_DIR', str(tmp_path / 'empty_cache'))
    assert set_raw(table('3.25', '0.5')) == _lib.IGX_ERR_NORTC
    A, E = both()
    assert rel_maxdiff(A, A_old) <= RTOL and rel_maxdiff(E, A_old) <= RTOL, (rel_maxdiff(A, A_old), rel_maxdiff(E, A_old))
    monkeypatch.delenv('IGX_NO_HIPRTC')
    # an expression that does not compile
    assert set_raw(table('3.25', '0.5', bad='x + undefined_name')) == _lib.IGX_ERR_COMPILE
    A, E = both()
    assert rel_maxdiff(A, A_old) <= RTOL and rel_maxdiff(E, A_old) <= RTOL, (rel_maxdiff(A, A_old), rel_maxdiff(E, A_old))
    # ... and the next call that succeeds takes effect for both algorithms
    assert set_raw(table('3.25', '0.5')) == _lib.IGX_OK
    A, E = both()
    assert rel_maxdiff(A, E) <= RTOL and rel_maxdiff(A, A_old) > 1e-3
    patch.close()


# ---------------------------------------------------------------------------------------------
# every compiled k_geoA instantiation (tests/_geoa_cases.py; tests/test_geoa_coverage_cpu.py ties the table to geoa.hip)
def _geoa_coeff(x, y, z):
    return 1.0 + x * x + 0.5 * z


_GEOA_AFFINE = (1.0, 0.5, -0.25, 0.125)


def _geoa_assemble(iga, axes, geo, kind, table, coeff, algo, monkeypatch, row0=None):
    """(CSR matrix, last_path) of one patch or row slab of a case."""
    kvs = _bf3_patch_kvs(iga, axes)
    g = gc.product_geo(iga, geo, len(axes))
    if kind == 'convdiff':
        if coeff == 'affine':
            asm = iga.assemblers.ConvDiffAssembler3D(kvs, g, iga.assemblers.AffineCoefficient(*_GEOA_AFFINE), row0=row0)
        else:
            with monkeypatch.context() as m:
                if coeff == 'sampled':
                    m.setenv('IGX_FORM_RTC', '0')                  # sampled on the host, read per point
                asm = iga.assemblers.ConvDiffAssembler3D(kvs, g, _geoa_coeff, row0=row0)
        A = asm.assemble_csr(algo=algo)
        path = asm.patch.last_path()
        asm.patch.close()
        return A, path
    patch = iga.assemblers.DevicePatch(kvs, g, row0=row0)
    if table is not None:
        patch.set_form_expr(gc.TABLES[table])
    A = patch.csr('form' if table is not None else kind, algo=algo)
    path = patch.last_path()
    patch.close()
    return A, path


def _geoa_oracle(axes, geo, kind, table, coeff):
    from oracle import iga_oracle as orc
    okvs = tuple(orc.KnotVector(bc.axis_knots(a), a[0]) for a in axes)
    ogeo = gc.oracle_geo(orc, geo, len(axes))
    if kind == 'convdiff':
        c = _geoa_coeff if coeff != 'affine' else (lambda x, y, z: _GEOA_AFFINE[0] + _GEOA_AFFINE[1] * x + _GEOA_AFFINE[2] * y + _GEOA_AFFINE[3] * z)
        return orc.assemble_nonsymmetric('convdiff', okvs, ogeo, coeff=c, nthreads=8)
    if table is not None:
        return orc.assemble_nonsymmetric('form', okvs, ogeo, table=gc.table_oracle(gc.TABLES[table]), nthreads=8)
    return orc.assemble(kind, okvs, ogeo, nthreads=8)


def _geoa_slabs(iga, axes, geo, kind, table, coeff, cuts, monkeypatch, key, twin):
    """The row slabs [cuts[k], cuts[k + 1]) of axis 0, stacked; each ran k_geoA (and the twin) like the whole patch."""
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        S, spath = _geoa_assemble(iga, axes, geo, kind, table, coeff, 'sumfact', monkeypatch, row0=(lo, hi))
        assert ('geoA' in spath) == (key is not None) and ('twin' in spath) == twin, (lo, hi, sorted(spath))
        parts.append(S)
    return scipy.sparse.vstack(parts).tocsr()


def _geoa_check(iga, axes, geo, kind, table, coeff, key, twin, bf3, tag, monkeypatch):
    """The whole patch: the intended chain ran, against the oracle and the entry-wise kernels; returns it."""
    A, path = _geoa_assemble(iga, axes, geo, kind, table, coeff, 'sumfact', monkeypatch)
    tag = (tag, key, sorted(path))
    assert ('geoA' in path) == (key is not None) and ('twin' in path) == twin, tag
    if bf3 is not None:
        assert ('bf3' in path) == bf3, tag
    sym = kind in ('mass', 'stiffness', 'form_sym')
    R = _geoa_oracle(axes, geo, kind, table, coeff)
    _bf3_check_vs_oracle(A, R, _bf3_patch_kvs(iga, axes), kind, tag, symmetric=sym)
    E, _ = _geoa_assemble(iga, axes, geo, kind, table, coeff, 'entrywise', monkeypatch)
    assert rel_maxdiff(A, E) <= RTOL, (tag, rel_maxdiff(A, E))
    return A


@pytest.mark.parametrize('case', gc.GEOA_CASES, ids=[c.id for c in gc.GEOA_CASES])
def test_every_geoa_instantiation_vs_oracle(iga, case, monkeypatch):
    """Every (k_geoA instantiation, form) launch_geoA can pick -- mass and stiffness at P = 2 .. 6 (one sweep wave for the mass
    form at P = 6), the matrix-core sweep, the convection-diffusion form, symmetric and non-symmetric coefficient tables, the 2D
    chain; geometry maps of degree 1 and 2 along axis 0 with spans not nested in the space mesh, B-spline and NURBS -- on a patch
    shaped for the edges (tests/_geoa_cases.py), and the decision edges where k_geoA must not run: the intended kernels ran
    (k_geoA, k_bf3, the twin, as restated), every value written, exact symmetry for the symmetric forms, the pattern and the values
    of the CPU oracle from the same control net, the entry-wise kernels, and -- one case per (P, P0G, NC, FORM, D2) -- row slabs
    of axis 0 bit for bit."""
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')
    if case.mfma:
        monkeypatch.setenv('IGX_GEOA', 'mfma')                 # (knobs are read when a patch is created)
    bf3 = None if case.key is None else case.bf3
    A = _geoa_check(iga, case.axes, case.geo, case.kind, case.table, case.coeff, case.key, case.twin, bf3, case.id, monkeypatch)
    if not case.slabs:
        return
    N0 = bc.numdofs(case.axes[0])
    cuts = sorted(set([0, 1, N0 // 2, N0]))
    V = _geoa_slabs(iga, case.axes, case.geo, case.kind, case.table, case.coeff, cuts, monkeypatch, case.key, case.twin)
    assert np.array_equal(V.indptr, A.indptr) and np.array_equal(V.indices, A.indices) and np.array_equal(V.data, A.data), (case.id, 'slabs')


@pytest.mark.parametrize('sweep', gc.CHUNK_SWEEPS, ids=[s[0] for s in gc.CHUNK_SWEEPS])
def test_geoa_axis0_chunks(iga, sweep, monkeypatch):
    """k_geoA splits the axis-0 sweep of a patch with a small cross-section into blockIdx.y chunks (sumfact.hip: sweep_chunks,
    geoa2d_min_chunk); each chunk re-walks P - 1 warm-up spans.  Axis 0 runs over sizes that give 1, 2, 3 and 4 chunks and every
    remainder of the last chunk, with a C^0 knot and a geometry span boundary inside the warm-up spans before a chunk start:
    against the oracle and the entry-wise kernels, and -- for the sizes of 3 and 4 chunks with no remainder -- row slabs cut just
    before, at and after a chunk boundary reproduce the whole patch bit for bit (a slab has fewer spans and a chunking of its
    own)."""
    name, ml, p0, (deg0, nurbs), kind, extra = sweep
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')
    table = extra if kind.startswith('form') else None
    coeff = extra if kind == 'convdiff' else None
    seen = set()
    for n0 in gc.chunk_sweep_sizes(ml, p0):
        a0, gk, length, nch = gc.chunk_axis0(ml, p0, n0)
        axes = (a0,) + tuple(ml)
        geo = gc.Geo(deg0, gk, nurbs, 300 + n0)
        key, twin = gc.geoa_route(axes, geo, kind, gc.TABLES[table] if table else None)
        tag = (name, n0, length, nch)
        assert key is not None and not twin, tag
        A = _geoa_check(iga, axes, geo, kind, table, coeff, key, False, gc.expect_bf3(axes, kind, key), tag, monkeypatch)
        if nch in (3, 4) and n0 % nch == 0 and nch not in seen:
            seen.add(nch)
            b = length * (1 if nch == 3 else 2)                # a chunk start (in spans = in dofs of its first function)
            cuts = [0, b - 1, b, b + 1, bc.numdofs(a0)]
            V = _geoa_slabs(iga, axes, geo, kind, table, coeff, cuts, monkeypatch, key, False)
            assert np.array_equal(V.indptr, A.indptr) and np.array_equal(V.indices, A.indices) and np.array_equal(V.data, A.data), (tag, 'slabs')
    assert seen == {3, 4}

"""Every instantiation, path and edge of the geometry-field kernels (k_geo_fields, k_geo_fields_lines), of k_grid_geo and
k_coeff_affine, and every tile shape of the single-launch 2D kernel k_single2d (csrc/kern_basis.hip) against a long-double
model: the cases of tests/_fields_cases.py, which tests/test_fields_coverage_cpu.py ties to the source.

Reference (tests/_fields_model.py): plain numpy in long double; no oracle library, no golden file.

Fields and k_grid_geo: the device may deviate from the long-double model by MARGIN = 8 times D, D being what the float64 run of
the same model deviates by on the same case (floor 16 * 2**-53), relative to the largest magnitude of the field over the case.
Before that, the planning query must equal the restatement: which kernel ran, its lines per block and its LDS bytes.

k_single2d: last_path() == {'single'}, the planning query equals the restatement (tile shape, LDS extents, bytes, blocks), every
entry of the matrix within (npts + c) 2**-53 mag + (the fields' tolerance carried through the sum) of the long-double assembly
(basis tables as the device holds them: bspline.active_deriv is the kernel that fills them), A == A.T bit for bit, every row
slab bit for bit the rows of the whole patch, no NaN under IGX_DEBUG_POISON.  Every test prints the figures it asserts on.
"""
import numpy as np
import pytest
import scipy.sparse

import pyiga_amd
from pyiga_amd import assemblers, bspline

import _entries_model as em
import _fields_cases as fc
import _fields_model as fm

pytestmark = pytest.mark.gpu

LD = np.longdouble


@pytest.fixture(autouse=True)
def _poison(monkeypatch):
    assert np.finfo(np.longdouble).eps < 2e-19
    monkeypatch.setenv('IGX_DEBUG_POISON', '1')          # an unwritten field or matrix value shows up as NaN


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _report(tag, dev, FLD, F64):
    """Asserts the tolerance field by field; returns (err / tolerance, err / D) -- the worst over the fields."""
    tol, D, mag = fm.tolerance(F64, FLD)
    assert not np.isnan(dev).any(), tag
    ax = tuple(range(1, FLD.ndim))
    err = abs(np.asarray(dev).astype(LD) - FLD).max(axis=ax)
    r_tol = float((err / tol).max())
    r_D = float((err / np.maximum(D * mag, fm.FLOOR / fm.MARGIN * fm.U * mag)).max())
    print('%s: err / tolerance %.3f, err / max(D, 2 u) %.2f, D %.2f u, err %.2f u' % (
        tag, r_tol, r_D, float(D.max() / fm.U), float((err / mag).max() / fm.U)))
    assert r_tol <= 1.0, (tag, r_tol, [float(v) for v in err / tol])
    return r_tol, r_D


# ---------------------------------------------------------------------------------------------
def _field_patch(case, sp, inp):
    geo = None if case.geo == 'jac' else fc.product_geo(pyiga_amd, case.geo)
    row0 = case.win[1] if case.win[0] == 'slab' else None
    bbox = case.win[1] if case.win[0] == 'box' else None
    return assemblers.DevicePatch(sp.kvs, geo, row0=row0, jacobian=inp['jac_full'], bbox=bbox, nqp=case.nqp)


@pytest.mark.parametrize('cid', [c.id for c in fc.FIELD_CASES])
def test_fields_against_long_double(cid):
    case = next(c for c in fc.FIELD_CASES if c.id == cid)
    sp, w, plan = fc.field_case_plan(case)
    inp = fc.field_inputs(case, sp, w)
    patch = _field_patch(case, sp, inp)
    try:
        kind = 'form' if case.kind.startswith('form') else case.kind
        assert patch.nqp == sp.q and patch.gauss_slab() == (w.g0, w.G0)
        for k in range(case.dim):
            lo, n = fm.window_axes(w, case.dim)[k] if case.win[0] == 'box' else (0, sp.G[k])
            nodes, wts = patch.gauss(k)
            assert np.array_equal(nodes, sp.gauss[k][0][lo:lo + n]) and np.array_equal(wts, sp.gauss[k][1][lo:lo + n])
        if case.kind == 'convdiff':
            if case.extra == 'affine':
                patch.set_coeff_affine(inp['coeff'][1])
            else:
                patch.set_coeff(inp['coeff_full'])
        elif case.kind == 'form_phys':
            patch.set_form(inp['table'])
        elif case.kind == 'form_par':
            patch.set_pform(inp['pterms'])
        # which kernel runs, its lines per block and its LDS bytes: the launcher's own decision
        assert patch.fields_plan(kind) == plan, (patch.fields_plan(kind), plan)
        F = patch.fields(kind)
    finally:
        patch.close()
    FLD = fc.model_fields(case, LD, sp, w, inp)
    F64 = fc.model_fields(case, np.float64, sp, w, inp)
    assert F.shape == FLD.shape, (F.shape, FLD.shape)
    inst = fc.fields_instantiation(case.dim, plan, case.kind.startswith('form'))
    _report('fields %s %s%s' % (cid, inst[0], inst[1]), F, FLD, F64)
    if case.extra == 'affine':
        # k_coeff_affine through the first six fields: c W J^-1 J^-T over the model's W J^-1 J^-T
        kw = dict(geo=fc.model_map(case.geo))
        B = fm.fields('stiffness', 3, w, sp.gauss, LD, **kw)
        ev = fm.eval_map(kw['geo'], [sp.gauss[k][0][lo:lo + n] for k, (lo, n) in enumerate(fm.window_axes(w, 3))], LD)[0]
        c = [LD(v) for v in inp['coeff'][1]]
        cm = c[0] + c[1] * ev[..., 0] + c[2] * ev[..., 1] + c[3] * ev[..., 2]
        tol = fm.tolerance(F64, FLD)[0]
        for k in range(6):
            ok = abs(B[k]) > 0.05 * abs(B[k]).max()
            dev = abs(F[k].astype(LD) / np.where(ok, B[k], 1) - cm)[ok]
            assert (dev <= (tol[k] / abs(B[k]))[ok]).all(), (k, float(dev.max()))
        print('k_coeff_affine<3> %s: coefficient from the fields within the fields\' tolerance, %d..%d points per field' % (
            cid, min(int((abs(B[k]) > 0.05 * abs(B[k]).max()).sum()) for k in range(6)), B[0].size))


@pytest.mark.parametrize('cid', [c.id for c in fc.GRID_CASES])
def test_grid_geo_against_long_double(cid):
    case = next(c for c in fc.GRID_CASES if c.id == cid)
    m = fc.grid_map(case)
    kvs = tuple(bspline.KnotVector(k, p) for k, p in m.kvs)
    J = bspline._device_grid_eval(kvs, m.ctrl, m.nurbs, case.ncomp, case.grid, want_jac=True)
    E = bspline._device_grid_eval(kvs, m.ctrl, m.nurbs, case.ncomp, case.grid, want_jac=False)
    eLD, jLD = fm.eval_map(m, case.grid, LD)
    e64, j64 = fm.eval_map(m, case.grid, np.float64)
    dim = m.dim
    assert J.shape == jLD.shape == tuple(len(g) for g in case.grid) + (case.ncomp, dim) and E.shape == eLD.shape
    fields_first = lambda a, n: np.moveaxis(a.reshape(a.shape[:dim] + (n,)), -1, 0)
    _report('k_grid_geo<%d> %s values' % (dim, cid), fields_first(E, case.ncomp), fields_first(eLD, case.ncomp), fields_first(e64, case.ncomp))
    n = case.ncomp * dim
    _report('k_grid_geo<%d> %s jacobian' % (dim, cid), fields_first(J, n), fields_first(jLD, n), fields_first(j64, n))


# ---------------------------------------------------------------------------------------------
def _device_tables(sp):
    """Per-axis tables with the basis values the device holds (bspline.active_deriv: the kernel that fills them)."""
    return em.tables_from_active_deriv(sp.kvs, sp.q, [bspline.active_deriv(kv, g[0], 1) for kv, g in zip(sp.kvs, sp.gauss)])


@pytest.mark.parametrize('kind', fc.S2D_KINDS)
@pytest.mark.parametrize('cid', [c.id for c in fc.S2D_CASES])
def test_single2d_against_long_double(cid, kind, monkeypatch):
    case = next(c for c in fc.S2D_CASES if c.id == cid)
    if case.path == 'single':
        monkeypatch.setenv('IGX_PATH', 'single')
    sp = fc.Space(case.axes, case.nqp)
    jac = fc.s2d_jac(case, sp) if case.geo == 'jac' else None
    geo = None if jac is not None else fc.product_geo(pyiga_amd, case.geo)
    N1 = sp.tables[1].N
    if fc.s2d_refused(case):
        # degree 0: sumfact_supported wants 1 <= p, so the assembly refuses the patch and k_single2d is never launched
        patch = assemblers.DevicePatch(sp.kvs, geo, nqp=case.nqp)
        try:
            assert not patch.info.sumfact_ok
            with pytest.raises(pyiga_amd._lib.IgxError, match='sum factorisation does not support this patch'):
                patch.assemble(kind, algo='sumfact')
        finally:
            patch.close()
        return

    def run(row0):
        patch = assemblers.DevicePatch(sp.kvs, geo, row0=row0, jacobian=jac, nqp=case.nqp)
        try:
            want = fc.single2d_plan(sp, case.geo, kind, case.path, row0=row0)
            assert patch.single2d_plan(kind) == want, (row0, patch.single2d_plan(kind), want)
            whole = fc.single2d_plan(sp, case.geo, kind, case.path, row0=row0, whole_patch=True)
            assert patch.single2d_plan(kind, whole_patch=True) == whole, (row0, patch.single2d_plan(kind, whole_patch=True), whole)
            data = patch.assemble(kind, algo='sumfact')
            assert patch.last_path() == {'single'}, (row0, patch.last_path())
            return data, patch.pattern(), want
        finally:
            patch.close()
    data, (indptr, indices), plan = run(None)
    assert not np.isnan(data).any()
    n = sp.tables[0].N * N1
    A = scipy.sparse.csr_matrix((data, indices, indptr), shape=(n, n))
    A.sort_indices()
    At = A.T.tocsr()
    At.sort_indices()
    assert np.array_equal(A.indptr, At.indptr) and np.array_equal(A.indices, At.indices)
    assert np.array_equal(_bits(A.data), _bits(At.data)), 'A != A.T bit for bit'
    for row0 in case.slabs:
        d, (ip, _), pl = run(row0)
        lo, hi = indptr[row0[0] * N1], indptr[row0[1] * N1]
        assert d.shape == (hi - lo,) and np.array_equal(ip, indptr[row0[0] * N1:row0[1] * N1 + 1] - lo)
        assert np.array_equal(_bits(d), _bits(data[lo:hi])), ('slab', row0, (pl['R0'], pl['R1']))
    # every entry against the long-double assembly
    tables = _device_tables(sp)
    w = em.whole_window(tables)
    kw = dict(jac=jac) if jac is not None else dict(geo=fc.model_map(case.geo))
    FLD = fm.fields(kind, 2, w, sp.gauss, LD, **kw)
    F64 = fm.fields(kind, 2, w, sp.gauss, np.float64, **kw)
    tol = fm.tolerance(F64, FLD)[0]
    val, mag, npts = fm.assemble2d(tables, FLD, kind)
    magF = fm.assemble2d(tables, FLD, kind, Fmag=np.broadcast_to(tol.reshape(-1, 1, 1), FLD.shape))[1]
    idx = fm.csr_order(tables)
    mi, mj = em.pattern(tables)
    assert np.array_equal(mi, indptr) and np.array_equal(mj, indices)
    bound = fm.single2d_bound(kind, mag, npts, magF)[idx]
    err = abs(data.astype(LD) - val[idx])
    worst = int(np.argmax(err / bound))
    r_round = float((err / ((npts[idx] + fm.C_SINGLE2D[kind]) * fm.U * mag[idx])).max())
    print('k_single2d<%s> %s tile %d x %d (%d blocks, %d bytes, NCOL %d): %d entries, err / bound %.3f (err / rounding part alone %.3f)' % (
        kind, cid, plan['R0'], plan['R1'], plan['blocks'], plan['lds'], plan['NCOL'], data.size, float((err / bound).max()), r_round))
    assert (err <= bound).all(), (worst, float(data[worst]), float(val[idx][worst]), float(err[worst] / bound[worst]))

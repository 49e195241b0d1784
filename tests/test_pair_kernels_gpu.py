"""The kernels of csrc/pair.hip (k_pair_pattern, k_pair_entries_csr, k_pair_entries_list; 2D and 3D, IGX_MASS and IGX_FORM)
through ``DevicePair``, for every case of tests/_pair_cases.py.

Reference (tests/_pair_model.py ``slot_matrix``): every entry summed in long double from the patch's own quadrature fields
(``DevicePatch.fields``) and the basis tables of BOTH spaces at the patch's Gauss nodes (``bspline.active_deriv``, the kernel
that fills the resident tables), so that only the pair kernels are under test.  Acceptance, entry by entry:
|dev - ref| <= (npts + C_KIND) 2**-53 mag, mag the same sum over absolute values, npts the Gauss points of the support
intersection, C_KIND counted from pair_entry_value (see the model; the expressions are entry_value's).  No measured factor.
entries() has the bits of the corresponding csr() values; pairs with disjoint supports or an index at or past the row or
column count give exactly 0.0.  Every test prints the largest |dev - ref| / bound.
"""
import numpy as np
import pytest

from pyiga_amd import assemblers, bspline, geometry

import _entries_cases as ec
import _entries_model as em
import _pair_cases as pc
import _pair_model as pm

pytestmark = pytest.mark.gpu

LD = np.longdouble


@pytest.fixture(autouse=True)
def _wide_long_double():
    assert np.finfo(np.longdouble).eps < 2e-19


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Dev:
    """Patch, pair and long-double tables of one case."""

    def __init__(self, case):
        self.case = case
        self.ku, self.kv = case.kvs(bspline)
        geo = geometry.quarter_annulus() if case.geo == 'quarter_annulus' else geometry.twisted_box()
        self.patch = assemblers.DevicePatch(self.ku, geo, nqp=case.q())
        self.pair = assemblers.DevicePair(self.patch, self.kv)
        self.nodes = [self.patch.gauss(k)[0] for k in range(case.dim)]
        for kv, g in zip(self.ku, self.nodes):
            assert np.array_equal(g, em.gauss_nodes(kv, case.q()))
        self.Bu = [pm.dense_colloc(kv, bspline.findspans(kv, g) - kv.p, bspline.active_deriv(kv, g, 1), LD) for kv, g in zip(self.ku, self.nodes)]
        self.Bv = [pm.dense_colloc(kv, bspline.findspans(kv, g) - kv.p, bspline.active_deriv(kv, g, 1), LD) for kv, g in zip(self.kv, self.nodes)]
        self.npts = pm.npts_matrix(self.ku, self.kv, case.q())

    def close(self):
        self.pair.close()
        self.patch.close()

    def kinds(self):
        """(kind, terms of the model, C_KIND), the patch set up for the kind."""
        d = self.case.dim
        yield 'mass', em.terms_of(d, 'mass'), em.c_kind(d, 'mass')
        self.patch.set_form(ec.phys_table(d, self.nodes))
        form = ('phys', em.physical_form_ab(d, ec.phys_present(d)))
        yield 'form', em.terms_of(d, 'form', form), em.c_kind(d, 'form', form)


@pytest.mark.parametrize('cid', [c.id for c in pc.CASES])
def test_pair_kernels_against_long_double(cid):
    case = pc.BY_ID[cid]
    dev = Dev(case)
    try:
        pair = dev.pair
        rows, cols = case.shape
        assert pair.shape == case.shape and pair.nnz == case.nnz
        assert tuple(pair.info.ndofs_trial)[:case.dim] == tuple(k.numdofs for k in dev.ku)
        assert tuple(pair.info.ndofs_test)[:case.dim] == tuple(k.numdofs for k in dev.kv)
        # k_pair_pattern
        indptr, indices = pair.pattern()
        ip, ind, maxrow = pm.pattern(dev.ku, dev.kv)
        assert indptr.dtype == np.int32 and indices.dtype == np.int32
        assert np.array_equal(indptr, ip) and np.array_equal(indices, ind) and indptr[-1] == pair.nnz == len(indices)
        nblocks, last = pc.csr_blocks(rows, maxrow)
        R = np.repeat(np.arange(rows), np.diff(indptr))
        idx, kinds = pc.picks(case, rows, cols, indptr, indices)
        for kind, terms, ck in dev.kinds():
            F = dev.patch.fields(kind)
            val, mag = pm.slot_matrix(dev.Bu, dev.Bv, F, terms)
            # k_pair_entries_csr: every value, entry by entry
            data = pair.assemble(kind, to_host=True)
            assert data.shape == (pair.nnz,) and not np.isnan(data).any()
            n = dev.npts[R, indices]
            assert (n > 0).all()
            err = abs(data.astype(LD) - val[R, indices])
            bound = (n + ck) * em.U * mag[R, indices]
            ratio = np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)
            assert (err <= bound).all(), (cid, kind, float(ratio.max()))
            worst_csr = float(ratio.max())
            # k_pair_entries_list: the bits of the csr values, exact zeros outside the pattern and past the ends
            got = pair.entries(kind, idx)
            worst_list = 0.0
            for k, ((I, J), cls) in enumerate(zip(idx.tolist(), kinds)):
                if cls == 'zero':
                    assert got[k] == 0.0 and not np.signbit(got[k]), (cid, kind, k, I, J)
                else:
                    pos = indptr[I] + int(np.searchsorted(indices[indptr[I]:indptr[I + 1]], J))
                    assert indices[pos] == J and _bits(got[k]) == _bits(data[pos]), (cid, kind, k, I, J)
                    worst_list = max(worst_list, float(ratio[pos]))
            for m in pc.request_lengths(len(idx))[1:]:
                assert np.array_equal(_bits(pair.entries(kind, idx[:m])), _bits(got[:m])), (cid, kind, m)
            print('%s %s: k_pair_entries_csr<%d> %d values in %d blocks (last: %d threads), max |dev - ref| / bound = %.3f; '
                  'k_pair_entries_list M = %d: %.3f' % (cid, kind, case.dim, len(data), nblocks, last, worst_csr, len(idx), worst_list))
    finally:
        dev.close()


def test_pair_create_refusals():
    """igx_pair_create names the failing condition: dimension, degree, breakpoints, boxed patch, row slab."""
    from pyiga_amd import _lib
    mk = bspline.make_knots
    ku = (mk(3, 0., 1., 4, mult=2), mk(3, 0., 1., 3, mult=2))
    geo = geometry.quarter_annulus()
    patch = assemblers.DevicePatch(ku, geo)
    try:
        for kvs, msg in (((mk(2, 0., 1., 4),), 'dimension'), ((mk(2, 0., 1., 4), mk(2, 0., 1., 4)), 'breakpoints'),
                         ((mk(16, 0., 1., 4), mk(2, 0., 1., 3)), 'degree'),
                         ((mk(2, 0., 1., 4), bspline.KnotVector(np.array([0., 0., 0., 0.3, 2. / 3, 1., 1., 1.]), 2)), 'breakpoints')):
            with pytest.raises(_lib.IgxError, match=msg):
                assemblers.DevicePair(patch, kvs)
    finally:
        patch.close()
    for kw, msg in ((dict(bbox=((0, 2), (0, 2))), 'span box'), (dict(row0=(0, 4)), 'row slab')):
        patch = assemblers.DevicePatch(ku, geo, **kw)
        try:
            with pytest.raises(_lib.IgxError, match=msg):
                assemblers.DevicePair(patch, (mk(2, 0., 1., 4), mk(2, 0., 1., 3)))
        finally:
            patch.close()

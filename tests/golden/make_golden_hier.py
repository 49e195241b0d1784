#!/usr/bin/env python3
"""Golden vectors for hierarchical (HB / THB) spline spaces, from the REAL reference (c-f-h/pyiga).

Run where an unmodified build of the reference is importable (see the header of make_golden.py):

    PYTHONPATH=/path/to/built/reference python3 tests/golden/make_golden_hier.py

Writes tests/golden/golden_hier.npz -- data only.  The cases are those of tests/_hier_cases.py (the table is shared: it is
written against the interface the reference and this package have in common).  Per case `id`:

    <id>_nlev, <id>_kv, <id>_kvlen        number of levels; the knots of all levels and axes (level-major) in one array, their lengths
    <id>_ac, _dc, _af, _df                active / deactivated cells and functions: rows (level, multi-index), sorted
    <id>_numactive, <id>_dirichlet
    <id>_ref                              the cells every refine_region call reported as refined: rows (round, level, multi-index)
    <id>_rfhb, _rfthb                     represent_fine(truncate=False / True): CSR triples (_data, _indices, _indptr, _shape) for
                                          the basis of the case (and RF_THB_CASES; not RF_PROBE_ONLY); otherwise _pat (packed bits of the
                                          dense pattern), _probe (transposed products with two seeded vectors) and _shape: the
                                          size limit of a committed file does not hold all of them entry by entry
    <id>_rf1hb, _rf1thb, _rf1rows, _rf1restr  (RF_LV1_CASES) the same for lv=1, and with rows=active_indices()[1], restrict False / True
    <id>_t2h                              thb_to_hb()
    <id>_A, <id>_rhs                      assemble.assemble(form, hs, geo=geo), assemble.assemble('f * v * dx', hs, geo=geo, f=f)
    <id>_M, <id>_C                        mass and the form with a coefficient (EXTRA_FORM_CASES)
    <id>_thb_amp                          THB cases, see below

Symmetric matrices are stored by their upper triangle (name + 'u'), to stay under the size limit of a committed file.

thb_amp: how strongly T' A T reacts to the rounding of A_hb -- the stored values of the HB matrix (the reference's, assembled
with truncate=False on a copy of the space) are multiplied by 1 + 1e-13 N(0, 1) (seeded), and the largest relative change of
T' A T over five seeds is divided by 1e-13.  solve_amp, proj_amp: the same for the solution of the Poisson problem and of the
L2 projection of the solve case when the values of the THB matrix are perturbed.
"""
import os
import sys

import numpy as np
import scipy.sparse
import scipy.sparse.linalg

import pyiga
from pyiga import approx, assemble, bspline, geometry
from pyiga.hierarchical import HSpace

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import _hier_cases as hc                                          # noqa: E402

pyiga.set_max_threads(1)
OUT = os.path.dirname(os.path.abspath(__file__))


def put_csr(out, name, A, upper=False):
    A = scipy.sparse.csr_matrix(A)
    A.sort_indices()
    if upper:
        A = scipy.sparse.triu(A, format='csr')
        A.sort_indices()
        name += 'u'
    small = max(A.shape) < 2 ** 16
    out[name + '_data'] = A.data
    out[name + '_indices'], out[name + '_indptr'] = A.indices.astype(np.uint16 if small else np.int32), A.indptr.astype(np.int32)
    out[name + '_shape'] = np.array(A.shape)


def put_probe(out, name, R):
    """A representation matrix by its pattern (entries above 1e-14 in magnitude, as packed bits of the dense 0/1 array) and its
    transposed products with the seeded vectors of _hier_cases.probe_vectors: every entry takes part in them with a weight of
    magnitude up to one, and they are a few kilobytes where the entries are tens."""
    R = scipy.sparse.csr_matrix(R)
    out[name + '_pat'] = np.packbits((abs(R.toarray()) > 1e-14).ravel())
    out[name + '_probe'] = R.T @ hc.probe_vectors(R.shape[0])
    out[name + '_shape'] = np.array(R.shape)


def sorted_tuples(s, dim):
    return np.array(sorted(s), dtype=np.int32).reshape(-1, dim)


def rel(A, B):
    return abs(A - B).max() / abs(B).max()


def amp_of(values, recompute, base, seeds=5):
    amp = 0.0
    for seed in range(seeds):
        rng = np.random.default_rng(seed)
        amp = max(amp, rel(recompute(values * (1 + 1e-13 * rng.standard_normal(values.size))), base) / 1e-13)
    return amp


def ref_form(form, dim):
    """The reference's own form objects for stiffness and mass (the nnz column of the case table was taken with them: in the THB
    cases scipy drops products that cancel exactly, so the count follows the last bit of the values), strings otherwise."""
    from pyiga import vform
    return {hc.STIFF: vform.stiffness_vf, hc.MASS: vform.mass_vf}[form](dim) if form in (hc.STIFF, hc.MASS) else form


def main():
    out = {}
    for name, (spec, tr, disp, rounds, reg, form, numactive, nnz) in hc.CASES.items():
        hs, refined = hc.build(bspline, HSpace, name)
        dim = hs.dim
        assert hs.numactive == numactive, (name, hs.numactive)
        out[name + '_nlev'] = np.array(hs.numlevels)
        # (one array per kind and case, the level -- and the round -- as leading columns: an archive member costs ~200 bytes)
        kvs_all = [kv.kv for lv in range(hs.numlevels) for kv in hs.knotvectors(lv)]
        out[name + '_kv'], out[name + '_kvlen'] = np.concatenate(kvs_all), np.array([k.size for k in kvs_all])
        for key, sets in (('_ac', [hs.active_cells(lv) for lv in range(hs.numlevels)]), ('_dc', [hs.deactivated_cells(lv) for lv in range(hs.numlevels)]),
                          ('_af', hs.actfun), ('_df', hs.deactfun)):
            out[name + key] = np.concatenate([np.column_stack((np.full(len(c), lv, dtype=np.int32), sorted_tuples(c, dim))) for lv, c in enumerate(sets)])
        out[name + '_numactive'] = np.array(hs.numactive)
        out[name + '_dirichlet'] = np.asarray(hs.dirichlet_dofs())
        out[name + '_ref'] = np.concatenate([np.column_stack((np.full(len(cells), r, dtype=np.int32), np.full(len(cells), lv, dtype=np.int32), sorted_tuples(set(cells), dim)))
                                             for r, marked in enumerate(refined) for lv, cells in sorted(marked.items()) if len(cells)])
        # both bases for every case: entry by entry where the size limit of a committed file allows, else pattern + probes
        (put_csr if not tr and name not in hc.RF_PROBE_ONLY else put_probe)(out, name + '_rfhb', hs.represent_fine(truncate=False))
        (put_csr if tr or name in hc.RF_THB_CASES else put_probe)(out, name + '_rfthb', hs.represent_fine(truncate=True))
        if name in hc.RF_LV1_CASES:
            put_csr(out, name + '_rf1hb', hs.represent_fine(lv=1, truncate=False))
            put_csr(out, name + '_rf1thb', hs.represent_fine(lv=1, truncate=True))
            rows = hs.active_indices()[1]
            put_csr(out, name + '_rf1rows', hs.represent_fine(lv=1, truncate=False, rows=rows))
            put_csr(out, name + '_rf1restr', hs.represent_fine(lv=1, truncate=False, rows=rows, restrict=True))
        T = hs.thb_to_hb()
        put_csr(out, name + '_t2h', T)
        geo = hc.geometry_of(geometry, dim)
        A = assemble.assemble(ref_form(form, dim), hs, geo=geo)
        if nnz is not None:
            assert A.nnz == nnz, (name, A.nnz)
        sym = form != hc.NONSYM
        put_csr(out, name + '_A', A, upper=sym)
        out[name + '_rhs'] = assemble.assemble('f * v * dx', hs, geo=geo, f=hc.f_rhs)
        if name in hc.EXTRA_FORM_CASES:
            put_csr(out, name + '_M', assemble.assemble(ref_form(hc.MASS, dim), hs, geo=geo), upper=True)
            put_csr(out, name + '_C', assemble.assemble(hc.COEFF, hs, geo=geo, c=hc.c_coeff), upper=True)
        if tr:
            hb, _ = hc.build(bspline, HSpace, name, truncate=False)
            Ahb = scipy.sparse.csr_matrix(assemble.assemble(ref_form(form, dim), hb, geo=geo))
            base = (T.T @ Ahb @ T).toarray()
            assert rel(base, A.toarray()) < 1e-13

            def again(v):
                P = Ahb.copy()
                P.data = v
                return (T.T @ P @ T).toarray()
            out[name + '_thb_amp'] = np.array(amp_of(Ahb.data, again, base))
        if name == hc.SOLVE_CASE:
            free = np.array(hs.non_dirichlet_dofs())
            A = scipy.sparse.csr_matrix(A)
            b = out[name + '_rhs']
            Aff = A[free][:, free].tocsr()
            u = scipy.sparse.linalg.spsolve(Aff.tocsc(), b[free])
            out[name + '_free'] = free
            out[name + '_u'] = u

            def solve_again(v):
                P = Aff.copy()
                P.data = v
                return scipy.sparse.linalg.spsolve(P.tocsc(), b[free])
            out[name + '_solve_amp'] = np.array(amp_of(Aff.data, solve_again, u))
            proj = approx.project_L2(hs, hc.f_rhs, f_physical=True, geo=geo)
            out[name + '_proj'] = proj
            M = scipy.sparse.csr_matrix(assemble.assemble(ref_form(hc.MASS, dim), hs, geo=geo))
            assert rel(scipy.sparse.linalg.spsolve(M.tocsc(), b), proj) < 1e-9

            def proj_again(v):
                P = M.copy()
                P.data = v
                return scipy.sparse.linalg.spsolve(P.tocsc(), b)
            out[name + '_proj_amp'] = np.array(amp_of(M.data, proj_again, scipy.sparse.linalg.spsolve(M.tocsc(), b)))
        print(name, hs.numactive, 'nnz', A.nnz, 'thb_amp', out.get(name + '_thb_amp'))
    path = os.path.join(OUT, 'golden_hier.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()

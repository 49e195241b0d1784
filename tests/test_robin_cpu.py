"""Boundary terms (Robin / Neumann), CPU tier: the position arithmetic of k_face_add restated in numpy (tests/_robin_model.py)
against scipy index lookups in E R E^T, the golden sums of tests/golden/golden_robin.npz reproduced in term order, the shifted
Kronecker preconditioner of the pure-Robin problem against Jacobi, and the validation of BoundaryTerm / boundary_terms= --
every ValueError raised before any device call.  No GPU."""
import os
import re

import numpy as np
import pytest
import scipy.sparse

import _robin_cases as rc
import _robin_model as rm
from conftest import ROOT, golden_csr


def _volume_lookup(kvs):
    """The canonical CSR pattern of the volume as a scipy matrix whose value at (I, J) is the entry's position + 1."""
    indptr, indices = rm.canonical_pattern(kvs)
    n = indptr.size - 1
    return scipy.sparse.csr_matrix((np.arange(1, indices.size + 1, dtype=np.float64), indices, indptr), shape=(n, n))


@pytest.mark.parametrize('name', sorted(rc.KERNEL_CASES))
def test_position_arithmetic_matches_index_lookup(name):
    from pyiga_amd.multipatch import boundary_dofs
    kvs = rc.kernel_kvs(name)
    V = _volume_lookup(kvs)
    for axis, side in rc.sides(len(kvs)):
        tkvs = rm.face_kvs(kvs, axis)
        fptr, find = rm.canonical_pattern(tkvs)
        assert find.size == rm.face_nnz(kvs, axis)
        dofs = boundary_dofs(kvs, (axis, side), ravel=True)
        assert dofs.size == fptr.size - 1
        It = np.repeat(np.arange(fptr.size - 1), np.diff(fptr))
        want = np.asarray(V[dofs[It], dofs[find]]).ravel()
        assert want.min() >= 1, (name, axis, side, 'a face entry outside the volume pattern')
        pos = rm.face_positions(kvs, axis, side)
        assert np.array_equal(pos, want.astype(np.int64) - 1), (name, axis, side)
        assert np.unique(pos).size == pos.size          # no two entries of one face share a position: no atomics needed


def test_model_axis_tables_are_the_library_tables():
    """jlo / jhi / rp of the model against the closed form for single interior knots: S = N (2p + 1) - p (p + 1) pairs."""
    from pyiga_amd import bspline
    for p, n in ((1, 2), (2, 5), (3, 4)):
        kv = bspline.make_knots(p, 0.0, 1.0, n)
        jlo, jhi, rp = rm.axis_tables(kv)
        N = kv.numdofs
        assert rp[-1] == N * (2 * p + 1) - p * (p + 1)
        assert np.array_equal(jlo, np.maximum(np.arange(N) - p, 0)) and np.array_equal(jhi, np.minimum(np.arange(N) + p + 1, N))


# ---- golden data
def _face_csr_values(R_dense, tkvs):
    from pyiga_amd import boundary_terms as bt
    return bt.face_values(scipy.sparse.csr_matrix(R_dense), tkvs)


def _model_sum(g, prefix, kvs, nterms):
    """A0 + sum E R E^T formed by the model in term order on the canonical values; b0 + sum E r."""
    from pyiga_amd.form_assemblers import parse_bdspec
    A0 = golden_csr(g, prefix + 'A0')
    indptr, indices = rm.canonical_pattern(kvs)
    lookup = scipy.sparse.csr_matrix((np.arange(indices.size, dtype=np.float64) + 1, indices, indptr), shape=A0.shape)
    vals = np.zeros(indices.size)
    A0 = A0.tocoo()
    where = np.asarray(lookup[A0.row, A0.col]).ravel().astype(np.int64) - 1
    assert where.min() >= 0
    vals[where] = A0.data
    b = g[prefix + 'b0'].copy()
    return vals, b, (indptr, indices), parse_bdspec


@pytest.mark.parametrize('prefix,terms', [('robin2_', rc.TERMS2), ('robin2n_', rc.TERMS2), ('robin3_', rc.TERMS3), ('cd2_', rc.TERMSC),
                                          ('heat2_', rc.TERMS2)])
def test_golden_sums_reproduced_in_term_order(golden, prefix, terms):
    g = golden('robin')
    kvs = rc.golden_patch_case(prefix)[0]
    vals, b, (indptr, indices), parse = _model_sum(g, prefix, kvs, len(terms))
    for k, (bd, mform, lform, _) in enumerate(terms):
        axis, side = parse(bd, len(kvs))
        if mform is not None:
            r = _face_csr_values(g['%sR%d' % (prefix, k)], rm.face_kvs(kvs, axis))
            rm.add_face(vals, kvs, axis, side, r)
        if lform is not None:
            b[g['%sR%d_dofs' % (prefix, k)]] += g['%sr%d' % (prefix, k)]
    A = scipy.sparse.csr_matrix((vals, indices, indptr), shape=(indptr.size - 1,) * 2)
    W = golden_csr(g, prefix + 'A')
    D = (A - W).tocsr()
    D.eliminate_zeros()
    assert D.nnz == 0, (prefix, abs(D).max())                # the same additions in the same order: exact
    assert np.array_equal(b, g[prefix + 'b']), prefix


def test_golden_multipatch_terms_share_an_interface_dof(golden):
    g = golden('robin')
    p2g = [g['mp_p2g%d' % p] for p in range(3)]
    dofs0 = p2g[0][g['mp_R0_dofs']]
    assert int(g['mp_R0_patch']) == 0 and int(g['mp_R1_patch']) == 2
    assert np.intersect1d(dofs0, p2g[1]).size == 1            # the corner of patch 0 'bottom' lies on the interface to patch 1
    # the stored sum is A0 + X E R E^T X^T, the stored load b0 + X E r
    A = golden_csr(g, 'mp_A0').tolil()
    b = g['mp_b0'].copy()
    for k in range(2):
        d = p2g[int(g['mp_R%d_patch' % k])][g['mp_R%d_dofs' % k]]
        A[np.ix_(d, d)] = A[np.ix_(d, d)] + g['mp_R%d' % k]
    b[dofs0] += g['mp_r0']
    assert abs(A.tocsr() - golden_csr(g, 'mp_A')).max() <= 1e-15 * abs(golden_csr(g, 'mp_A')).max()
    assert np.allclose(b, g['mp_b'], rtol=0, atol=1e-15)


def test_shifted_kron_beats_jacobi_on_pure_robin(golden):
    """robin2n_: no fixed dof.  The unshifted fast-diagonalization preconditioner is singular (sum lam_k = 0 on the constant);
    with lam_k + sigma / (d |domain|), sigma = 1^T R 1, PCG converges and needs fewer iterations than Jacobi."""
    from pyiga_amd import boundary_terms as bt
    g = golden('robin')
    kvs = rc.kvs2()
    A = golden_csr(g, 'robin2n_A').toarray()
    b = g['robin2n_b']
    sigma = float(g['robin2n_R0'].sum() + g['robin2n_R1'].sum())
    shift = bt.kron_shift(kvs, sigma)
    assert shift > 0
    # 1D parametric stiffness and mass matrices of the axes, on the host (the test oracle's quadrature)
    from oracle import iga_oracle as orc
    okv = orc.make_knots(3, 0.0, 1.0, 8)
    K1 = 2 * [orc.bsp_mixed_deriv_biform_1d(okv, 1, 1).toarray()]
    M1 = 2 * [orc.bsp_mixed_deriv_biform_1d(okv, 0, 0).toarray()]
    assert K1[0].shape == (kvs[0].numdofs,) * 2 and abs(K1[0].sum()) < 1e-10 and abs(M1[0].sum() - 1.0) < 1e-13
    x_k, it_k = rm.shifted_kron_pcg(A, b, kvs, K1, M1, shift, tol=1e-10)
    x_j, it_j = rm.shifted_kron_pcg(A, b, kvs, None, None, 0.0, tol=1e-10)
    u = g['robin2n_u']
    print('pure Robin, 2D p=3 n=8: PCG iterations shifted kron %d, jacobi %d' % (it_k, it_j))
    assert np.abs(x_k - u).max() <= 1e-7 * np.abs(u).max() and np.abs(x_j - u).max() <= 1e-7 * np.abs(u).max()
    assert it_k < it_j, (it_k, it_j)


# ---- validation: every ValueError before any device call
@pytest.fixture
def no_device(monkeypatch):
    from pyiga_amd import _lib

    def refuse(*a, **k):
        raise AssertionError('device call before the boundary terms were validated')
    monkeypatch.setattr(_lib, 'load', refuse)
    monkeypatch.setattr(_lib, 'context', refuse)


def test_boundary_term_rejects_bad_forms():
    from pyiga_amd import solvers
    BT = solvers.BoundaryTerm
    with pytest.raises(ValueError, match='neither'):
        BT('right')
    with pytest.raises(ValueError, match='dx'):
        BT('right', matrix='u*v*dx')
    with pytest.raises(ValueError, match='dx'):
        BT('right', rhs='g*v*dx', g=1.0)
    with pytest.raises(ValueError, match='bfuns'):
        BT('right', matrix='inner(u,v)*ds', bfuns=[('u', 2), ('v', 2)])
    with pytest.raises(ValueError, match='bilinear'):
        BT('right', matrix='g*v*ds')
    with pytest.raises(ValueError, match='linear'):
        BT('right', rhs='u*v*ds')
    t = BT('top', matrix='alpha*u*v*ds', rhs='g*v*ds', alpha=2.0, g=1.0)
    assert t.patch is None and set(t.inputs) == {'alpha', 'g'}


def test_systems_validate_terms_before_any_device_work(no_device):
    from pyiga_amd import solvers
    BT = solvers.BoundaryTerm
    kvs, geo = rc.kvs2(), rc.geo2()
    n = int(np.prod([kv.numdofs for kv in kvs]))
    b = np.ones(n)
    nonsym = BT('right', matrix='inner((1.0, 2.0), grad(u)) * v * ds')
    cases = [
        ([BT('nowhere', matrix='u*v*ds')], 'bdspec'),
        ([BT((2, 0), matrix='u*v*ds')], 'bdspec'),
        ([BT('right', matrix='u*v*ds', patch=0)], 'patch'),
        (['u*v*ds'], 'BoundaryTerm'),
        ([nonsym], 'symmetric'),
    ]
    for terms, word in cases:
        with pytest.raises(ValueError, match=word):
            solvers.PatchSystem(kvs, geo, b, boundary_terms=terms)
        with pytest.raises(ValueError, match=word):
            solvers.ParabolicSystem(kvs, geo, b, method='cg', boundary_terms=terms)
    with pytest.raises(ValueError, match='symmetric'):
        solvers.FormSystem('inner(grad(u),grad(v))*dx', kvs, b, geo=geo, method='cg', boundary_terms=[nonsym])
    with pytest.raises(ValueError, match='bdspec'):
        solvers.FormSystem(rc.CD2_FORM, kvs, b, geo=geo, diff_coeff=rc.kappa2, boundary_terms=[BT('nowhere', matrix='u*v*ds')])
    # 3D: the symmetry check runs on the face's Gauss grid without creating the face patch
    kvs3, g3 = rc.kvs3(), rc.geo3()
    with pytest.raises(ValueError, match='symmetric'):
        solvers.PatchSystem(kvs3, g3, np.ones(216), boundary_terms=[BT('top', matrix='inner((1.0, 2.0, 0.5), grad(u)) * v * ds')])


def test_multipatch_validates_terms_before_any_device_work(no_device):
    from pyiga_amd import solvers
    BT = solvers.BoundaryTerm
    MP = rc.lshape()
    f = 'f*v*dx'
    K = 'inner(grad(u),grad(v))*dx'
    with pytest.raises(ValueError, match='patch'):
        solvers.MultipatchSystem(MP, K, f, f=rc.fmp, boundary_terms=[BT('right', matrix='u*v*ds')])
    with pytest.raises(ValueError, match='patch'):
        solvers.MultipatchSystem(MP, K, f, f=rc.fmp, boundary_terms=[BT('right', matrix='u*v*ds', patch=3)])
    with pytest.raises(ValueError, match='bdspec'):
        MP.assemble_system(K, f, f=rc.fmp, boundary_terms=[BT('front', matrix='u*v*ds', patch=0)])
    with pytest.raises(ValueError, match='right-hand side'):
        MP.assemble_system(K, None, boundary_terms=[BT('right', rhs='g*v*ds', patch=0, g=rc.g2)])
    with pytest.raises(ValueError, match='symmetric'):
        solvers.MultipatchSystem(MP, K, f, f=rc.fmp, boundary_terms=[BT('right', matrix='inner((1.0, 2.0), grad(u)) * v * ds', patch=0)])


def test_new_symbols_declared_and_bound():
    from pyiga_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'igx.h')).read()
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    for name in ('igx_patch_add_face', 'igx_patch_add_face_host', 'igx_multipatch_add_face', 'igx_multipatch_add_face_host'):
        assert re.search(r'\bint\s+%s\s*\(' % name, hdr), name
        assert name in bound and len(bound[name][1]) == (6 if 'multipatch' in name and 'host' in name else
                                                         5 if 'multipatch' in name or 'host' in name else 4)
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in ('igx_patch_add_face', 'igx_patch_add_face_host', 'igx_multipatch_add_face', 'igx_multipatch_add_face_host'):
        assert name in doc, name

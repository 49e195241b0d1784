"""Vector-valued Dirichlet problems on a multipatch (solvers.MultipatchVectorSystem, igx_solver_create_multipatch_block): what
can be checked without a GPU.

- The dispatch table of k_csr_block_spmv names exactly the ten (GW, U, NC) instantiations, none is written outside it, and the
  GPU cases (tests/_mpvec_model.py) reach every group width past one grid of scalar rows at 2 and 3 components.
- ``glue`` of symmetric patch matrices is symmetric; ``BlockSchwarzModel.dense()`` is symmetric positive definite on the free dofs
  of a 2-component L-shape; the model's preconditioned CG agrees with scipy's.
- The argument refusals raise ValueError before any device call.
- The new ABI names are declared, bound and exported.
"""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.linalg

from pyiga_amd import _lib, assemble, bspline, solvers

import _mpsolve_model as M
import _mpvec_model as MV
import _solver_cases as sc
import _vecsolve_model as V
from test_vecsolve_cpu import _HostGeo, _HostPatch, _no_device

from conftest import ROOT

NEW_NAMES = ('igx_solver_create_multipatch_block', 'igx_solver_take_multipatch_block', 'igx_solver_download_multipatch_block',
             'igx_solver_set_block_schwarz')
MU_LAM = dict(mu=1.0, lam=2.0)


@pytest.fixture(scope='module')
def src():
    return sc.read_source()


def test_csr_block_dispatch_table_names_exactly_the_ten_instantiations(src):
    lines = MV.parse_csr_block_dispatch(src)
    assert len(lines) == 10, sorted(lines, key=str)
    assert {(gw, u, nc) for _, gw, u, nc in lines} == MV.CSR_BLOCK_SPMV_INSTANCES
    assert {(gw, nc) for _, gw, _, nc in lines} == {(gw, nc) for gw in sc.GWS for nc in (2, 3)}
    for label, gw, _, _ in lines:
        assert label == gw or (label is None and gw == 4), (label, gw)


def test_no_csr_block_instance_outside_the_table(src):
    assert MV.csr_block_instances_outside_table(src) == []
    # the scans of the three older families do not match the new kernel's name, and still find nothing outside their tables
    assert sc.instances_outside_tables(src) == []
    assert V.block_instances_outside_table(src) == []
    assert len(V.parse_block_dispatch(src)) == 10


def test_cases_reach_every_width_past_one_grid():
    past = set()
    patterns = {}
    for c in MV.MPVEC_CASES:
        if c.mp.id not in patterns:
            MP = c.build()
            patterns[c.mp.id] = (MP.numdofs, sc.max_row(sc.multipatch_pattern(MP)))
        rows, longest = patterns[c.mp.id]
        assert sc.spmv_gw(longest) == c.gw, (c.id, longest)
        if rows > sc.spmv_pass_rows(c.gw):
            past.add((c.gw, c.nc))
    assert past == {(gw, nc) for gw in sc.GWS for nc in (2, 3)}, sorted(past)
    assert all(len(MV.PRESENT[nc]) == k for nc, k in ((2, 4), (3, 5)))
    assert all((c, c) in MV.PRESENT[nc] for nc in (2, 3) for c in range(nc))


# ---------------------------------------------------------------------------------------------
def _lshape_blocked(oracle, p=2, n=6):
    """The 2-component L-shape with the per-patch blocked matrices [[K + M, M / 2], [M / 2, K + 2 M]] from the oracle's 1D
    matrices (every patch a unit square up to a rigid motion: K and M are sums of Kronecker products of the 1D ones)."""
    MP = M.lshape(p=p, n=n)
    mats1d = M.mats1d_oracle(oracle)
    kvs = tuple(MP.patches[0][0])
    K1, M1 = mats1d(kvs[0])
    K1, M1 = scipy.sparse.csr_matrix(K1), scipy.sparse.csr_matrix(M1)
    K = scipy.sparse.kron(K1, M1) + scipy.sparse.kron(M1, K1)
    Mm = scipy.sparse.kron(M1, M1)
    Ap = scipy.sparse.bmat([[K + Mm, 0.5 * Mm], [0.5 * Mm, K + 2 * Mm]], format='csr')
    return MP, [Ap] * MP.numpatches, mats1d


def _schwarz_model(MP, fixed, nc, mats1d):
    shapes, maps = M.shapes_maps(MP)
    n = MP.numdofs
    kvs_list = [tuple(kvs) for kvs, _ in MP.patches]
    setups = []
    for c in range(nc):
        fc = fixed[(fixed >= c * n) & (fixed < (c + 1) * n)] - c * n
        boxes = solvers.schwarz_boxes(shapes, maps, fc)
        setups.append((boxes,) + solvers.schwarz_factors(kvs_list, boxes, 'stiffness', mats1d))
    return MV.BlockSchwarzModel(n, shapes, maps, fixed, setups), setups


def test_glue_of_symmetric_patch_matrices_is_symmetric(oracle):
    MP, mats, _ = _lshape_blocked(oracle)
    A = MV.glue(MP, mats, 2)
    n = MP.numdofs
    assert A.shape == (2 * n, 2 * n)
    assert abs(A - A.T).max() <= 1e-15 * abs(A).max()
    # block (0, 1) is the scalar glue of M / 2, and every interface row is longer than the patch rows it sums
    B01 = A[:n, n:]
    S = sc.multipatch_pattern(MP)
    assert np.array_equal(np.diff(B01.indptr), np.diff(S.indptr))
    assert len(MP.shared_dofs) > 0 and MV.interface_rows_gain(MP, S).min() > 0


def test_block_schwarz_model_is_spd_and_its_pcg_agrees_with_scipy(oracle):
    MP, mats, mats1d = _lshape_blocked(oracle)
    n = MP.numdofs
    A = MV.glue(MP, mats, 2)
    fixed = MV.blocked_fixed(MP, [[(0, 'left')], []], 2)             # component 0 clamped on one side, component 1 floating
    assert fixed.size and fixed.max() < n
    P, setups = _schwarz_model(MP, fixed, 2, mats1d)
    free = np.setdiff1d(np.arange(2 * n), fixed)
    # patch 0 of component 0 lost its first index on axis 1 ('left'); every patch of component 1 is floating
    assert setups[0][0][0][0][1] == 1 and all(lo == (0, 0) for lo, _ in setups[1][0])
    D = P.dense()
    assert np.allclose(D, D.T, atol=1e-12 * abs(D).max())
    assert not D[fixed].any() and not D[:, fixed].any()
    Df = D[np.ix_(free, free)]
    assert np.linalg.eigvalsh(0.5 * (Df + Df.T)).min() > 0
    r = np.random.default_rng(3).standard_normal(2 * n)
    assert np.allclose(P.apply(r), D @ np.where(np.isin(np.arange(2 * n), fixed), 0.0, r), atol=1e-12 * abs(D).max() * abs(r).max())

    def Mfree(v):
        full = np.zeros(2 * n)
        full[free] = v
        return P.apply(full)[free]
    b = np.random.default_rng(7).standard_normal(2 * n)
    Aff, bf = A[free][:, free], b[free]
    x, it, conv = V.pcg(Aff, bf, Mfree, tol=1e-10)
    it_sp, x_sp, info = M.cg_iterations(Aff, bf, Mfree, 1e-10)
    assert conv and info == 0 and abs(it - it_sp) <= 1, (it, it_sp)
    xs = scipy.sparse.linalg.spsolve(Aff.tocsc(), bf)
    assert np.linalg.norm(x - xs) <= 1e-8 * np.linalg.norm(xs)
    assert np.linalg.norm(x_sp - xs) <= 1e-8 * np.linalg.norm(xs)


# ---------------------------------------------------------------------------------------------
def _host_multipatch():
    """Two unit squares side by side with a geometry evaluated on the host: no device is needed to number or inspect them."""
    kvs = 2 * (bspline.make_knots(2, 0.0, 1.0, 4),)
    MP = assemble.Multipatch([(kvs, _HostGeo()), (kvs, _HostGeo())])
    MP.join_boundaries(0, 'right', 1, 'left')
    MP.finalize()
    return MP


@pytest.mark.parametrize('problem, kwargs, match', [
    ('inner(u, v) * dx', dict(bfuns=[('u', 2), ('v', 3)]), 'components'),                           # mixed
    ('inner(u, v) * ds', dict(bfuns=V.bfuns(2)), 'boundary'),
    ('inner(f, v) * dx', dict(bfuns=[('v', 2)], f=(1.0, 0.0)), 'bilinear'),                         # a functional
    ('u * v * dx', {}, 'scalar form'),
    ('inner(u, v) * dx', dict(bfuns=V.bfuns(4)), '2 or 3'),
    (V.ELASTICITY, dict(bfuns=V.bfuns(2), method='gmres', **MU_LAM), 'method'),
])
def test_refusals_before_any_device_work(monkeypatch, problem, kwargs, match):
    _no_device(monkeypatch)
    MP = _host_multipatch()
    monkeypatch.setattr(MP, '_device', lambda: pytest.fail('device multipatch created'))
    with pytest.raises(ValueError, match=match):
        solvers.MultipatchVectorSystem(MP, problem, 0.0, **kwargs)
    if 'method' not in kwargs:
        kw = {k: v for k, v in kwargs.items() if k != 'bfuns'}
        with pytest.raises(ValueError, match=match):
            MP.assemble_vector_system(problem, 0.0, kwargs.get('bfuns'), **kw)


def test_refuses_a_form_object(monkeypatch):
    _no_device(monkeypatch)
    from pyiga_amd import form_assemblers
    with pytest.raises(ValueError, match='form string'):
        solvers.MultipatchVectorSystem(_host_multipatch(), form_assemblers.FormAssembler, 0.0)


class _ClosableHostPatch(_HostPatch):
    """The host stand-in of DevicePatch, which the system may close (the only call besides the Gauss grid)."""

    def close(self):
        pass


def test_cg_on_a_non_symmetric_form_refused_before_any_assembly(monkeypatch):
    from pyiga_amd import form_assemblers
    _no_device(monkeypatch)
    monkeypatch.setattr(form_assemblers, 'DevicePatch', _ClosableHostPatch)
    MP = _host_multipatch()
    monkeypatch.setattr(MP, '_device', lambda: pytest.fail('device multipatch created'))
    with pytest.raises(ValueError, match='not symmetric'):
        solvers.MultipatchVectorSystem(MP, V.NONSYM, 0.0, bfuns=V.bfuns(2), method='cg')


def test_assemble_system_keeps_refusing_bfuns():
    with pytest.raises(NotImplementedError):
        _host_multipatch().assemble_system(V.ELASTICITY, None, bfuns=V.bfuns(2), **MU_LAM)


def test_new_abi_names_declared_bound_exported():
    hdr = open(os.path.join(ROOT, 'include', 'igx.h')).read()
    declared = set(re.findall(r'\b(igx_[a-z_0-9]+)\s*\(', hdr))
    bound = {name for name, _, _ in _lib.SYMBOLS}
    nm = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in NEW_NAMES:
        assert name in declared and name in bound, name
        assert re.search(r'\bT %s\b' % name, nm), name

"""Vector-valued Dirichlet problems on the device (solvers.VectorFormSystem, igx_solver_create_block): what can be checked
without a GPU.

- Every refusal happens before any device work, and CG on a non-symmetric form before any assembly.
- Symmetry of the block coefficient tables: elasticity and grad-div are symmetric, a one-way coupling is not.
- The numpy model of block-Kronecker-preconditioned CG (tests/_vecsolve_model.py) agrees with scipy on a blocked matrix
  assembled on the host.
- The dispatch table of k_block_spmv has one case line per group width and number of components, no instantiation is named
  outside it, and the GPU cases reach every width past one grid of scalar rows at 2 and 3 components.
"""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.linalg

from pyiga_amd import _lib, bspline, geometry, solvers, tforms
from pyiga_amd.quadrature import make_tensor_quadrature

import _mpsolve_model as M
import _solver_cases as sc
import _vecsolve_model as V

from conftest import ROOT

NEW_NAMES = ('igx_solver_create_block', 'igx_solver_take_block', 'igx_solver_set_block_kron')
MU_LAM = dict(mu=1.0, lam=2.0)


def _kvs(d, p=2, n=4):
    return (bspline.make_knots(p, 0.0, 1.0, n),) * d


def _geo(d):
    return geometry.quarter_annulus() if d == 2 else geometry.tensor_product(geometry.line_segment(0.0, 1.0),
                                                                             geometry.quarter_annulus())


class _HostPatch:
    """Stands in for DevicePatch: the Gauss grid from the host, and no device work at all (an assembly fails the test)."""

    def __init__(self, kvs, geo, device=None, **kw):
        self.kvs = tuple(kvs)
        self.nqp = max(kv.p for kv in self.kvs) + 1
        self.ndofs = tuple(kv.numdofs for kv in self.kvs)

    def gauss(self, axis):
        nodes, weights = make_tensor_quadrature([self.kvs[axis].mesh], self.nqp)
        return nodes[0], weights[0]

    def __getattr__(self, name):
        raise AssertionError('device work: DevicePatch.%s' % name)


class _HostGeo:
    """The identity map of the unit square, evaluated on the host."""
    dim = sdim = 2

    def grid_eval(self, grid):
        return np.stack(np.meshgrid(*grid, indexing='ij')[::-1], axis=-1)


def _no_device(monkeypatch, host_patch=False):
    from pyiga_amd import assemblers, form_assemblers

    def no_device(*a, **k):
        raise AssertionError('device patch created')
    monkeypatch.setattr(assemblers, 'DevicePatch', no_device)
    monkeypatch.setattr(form_assemblers, 'DevicePatch', _HostPatch if host_patch else no_device)


@pytest.mark.parametrize('problem, kvs_dim, kwargs, match', [
    (V.ELASTICITY, 2, dict(bfuns=V.bfuns(2), **MU_LAM), 'geo'),                                      # no geo
    ('inner(u, v) * dx', 2, dict(bfuns=[('u', 2), ('v', 3)]), 'components'),                        # mixed
    ('inner(u, v) * ds', 2, dict(bfuns=V.bfuns(2)), 'boundary'),
    ('inner(u, v) * dx', 1, dict(bfuns=V.bfuns(2)), 'surface'),                                      # a surface patch
    ('inner(f, v) * dx', 2, dict(bfuns=[('v', 2)], f=(1.0, 0.0)), 'bilinear'),                      # a functional
    ('u * v * dx', 2, {}, 'FormSystem'),                                                             # a scalar form
    ('inner(u, v) * dx', 2, dict(bfuns=V.bfuns(4)), '2 or 3'),
    (V.ELASTICITY, 2, dict(bfuns=V.bfuns(2), method='gmres', **MU_LAM), 'method'),
])
def test_refusals_before_any_device_work(monkeypatch, problem, kvs_dim, kwargs, match):
    _no_device(monkeypatch)
    kw = dict(kwargs)
    if match != 'geo':
        kw['geo'] = geometry.unit_square()
    with pytest.raises(ValueError, match=match):
        solvers.VectorFormSystem(problem, _kvs(kvs_dim), 0.0, **kw)


def test_refuses_a_form_object(monkeypatch):
    _no_device(monkeypatch)
    from pyiga_amd import form_assemblers
    with pytest.raises(ValueError, match='form string'):
        solvers.VectorFormSystem(form_assemblers.FormAssembler, _kvs(2), 0.0, geo=geometry.unit_square())


def test_cg_on_a_non_symmetric_form_refused_before_any_assembly(monkeypatch):
    _no_device(monkeypatch, host_patch=True)
    with pytest.raises(ValueError, match='not symmetric'):
        solvers.VectorFormSystem(V.NONSYM, _kvs(2), 0.0, bfuns=V.bfuns(2), method='cg', geo=_HostGeo())


def _tables(form, d, nc, inputs=None):
    rng = np.random.default_rng(d * 10 + nc)
    G = (3,) * d
    X = rng.uniform(0.1, 1.0, G + (d,))
    arity, measure, table, ncs = tforms.evaluate(form, G, X, dict(inputs or {}), V.bfuns(nc))
    assert arity == 2 and measure == 'dx' and ncs == (nc, nc)
    return table


@pytest.mark.parametrize('d', [2, 3])
def test_symmetry_of_the_block_tables(d):
    assert solvers.symmetric_block_tables(_tables(V.ELASTICITY, d, d, MU_LAM))
    assert solvers.symmetric_block_tables(_tables(V.GRAD_DIV, d, d))
    assert solvers.symmetric_block_tables(_tables('(inner(grad(u), grad(v)) + inner(u, v)) * dx', d, 3))
    # an x-dependent coefficient keeps the symmetry of its jets
    assert solvers.symmetric_block_tables(_tables('(1 + x[0]*x[1]) * div(u) * div(v) * dx', d, d))
    assert not solvers.symmetric_block_tables(_tables(V.NONSYM, d, 2))
    assert not solvers.symmetric_block_tables(_tables(V.COUPLED[2], d, 2))
    assert not solvers.symmetric_block_tables(_tables(V.COUPLED[3], d, 3))
    # a None opposite an array of zeros is not symmetric; values within 1e-13 of the largest entry are
    t = _tables(V.GRAD_DIV, d, d)
    t[0][1][1][2], t[1][0][2][1] = None, np.zeros(3)
    assert not solvers.symmetric_block_tables(t)
    t = _tables(V.ELASTICITY, d, d, MU_LAM)
    big = max(float(np.max(np.abs(e))) for row in t for tab in row for trow in tab for e in trow if e is not None)
    t[0][1][1][2] = t[0][1][1][2] + 0.5e-13 * big
    assert solvers.symmetric_block_tables(t)
    t[0][1][1][2] = t[0][1][1][2] + 2e-13 * big
    assert not solvers.symmetric_block_tables(t)


def test_block_kron_cg_model_agrees_with_scipy(oracle):
    """Blocked matrix [[K + M, M / 2], [M / 2, K + 2 M]] of the 2D stiffness K and mass M on the unit square (the oracle's 1D
    matrices), the first component clamped on one side, the second floating (the sigma / d shift); the model's CG with the
    block-Kronecker preconditioner against scipy's CG with the same preconditioner: iterations and solution."""
    p, n = 2, 10
    kvs = _kvs(2, p, n)
    mats = M.mats1d_oracle(oracle)
    K1, M1 = mats(kvs[0])
    K1, M1 = scipy.sparse.csr_matrix(K1), scipy.sparse.csr_matrix(M1)
    K = scipy.sparse.kron(K1, M1) + scipy.sparse.kron(M1, K1)      # (the unit square: sums of Kronecker products of 1D matrices)
    Mm = scipy.sparse.kron(M1, M1)
    A = scipy.sparse.bmat([[K + Mm, 0.5 * Mm], [0.5 * Mm, K + 2 * Mm]], format='csr')
    ndofs = tuple(kv.numdofs for kv in kvs)
    N = int(np.prod(ndofs))
    from pyiga_amd import assemble
    fixed = assemble.boundary_dofs(kvs, (0, 0), ravel=True)     # component 0 only
    free = np.setdiff1d(np.arange(2 * N), fixed)
    boxes = [solvers.dirichlet_box(ndofs, fixed), solvers.dirichlet_box(ndofs, [])]
    assert boxes[0] == ((1, 0), (ndofs[0], ndofs[1])) and boxes[1] == ((0, 0), ndofs)
    factors = []
    for c, (lo, hi) in enumerate(boxes):
        U, lam, mode = solvers.fastdiag_factors(kvs, lo, hi, True, mats)
        if c == 1:
            sigma = min(l[1] for l in lam)
            lam = [l + sigma / 2 for l in lam]
        factors.append((lo, hi, U, lam, mode))
    P = V.BlockKronModel(ndofs, factors)

    def Mfree(r):
        full = np.zeros(2 * N)
        full[free] = r
        return P.apply(full)[free]
    rng = np.random.default_rng(7)
    b = rng.standard_normal(2 * N)
    Aff = A[free][:, free]
    bf = b[free]
    x, it, conv = V.pcg(Aff, bf, Mfree, tol=1e-10)
    it_sp, x_sp, info = M.cg_iterations(Aff, bf, Mfree, 1e-10)
    assert conv and info == 0
    assert abs(it - it_sp) <= 1, (it, it_sp)
    xs = scipy.sparse.linalg.spsolve(Aff.tocsc(), bf)
    assert np.linalg.norm(x - xs) <= 1e-8 * np.linalg.norm(xs)
    assert np.linalg.norm(x_sp - xs) <= 1e-8 * np.linalg.norm(xs)
    # the preconditioner is symmetric positive definite on the free dofs, and much better than none
    Pd = np.column_stack([Mfree(e) for e in np.eye(free.size)])
    assert np.allclose(Pd, Pd.T, atol=1e-12 * abs(Pd).max())
    assert np.linalg.eigvalsh(0.5 * (Pd + Pd.T)).min() > 0
    assert it < V.pcg(Aff, bf, None, tol=1e-10)[1] / 2


# ---------------------------------------------------------------------------------------------
# the dispatch table of k_block_spmv and the cases that run it
@pytest.fixture(scope='module')
def src():
    return sc.read_source()


def test_block_dispatch_table_case_lines(src):
    lines = V.parse_block_dispatch(src)
    assert len(lines) == 2 * len(sc.GWS), sorted(lines, key=str)
    assert {(gw, u, nc) for _, gw, u, nc in lines} == V.BLOCK_SPMV_INSTANCES
    for label, gw, _, _ in lines:
        assert label == gw or (label is None and gw == 4), (label, gw)


def test_no_block_instance_outside_the_table(src):
    assert V.block_instances_outside_table(src) == []
    # (the names of the two scalar families do not match the new one)
    assert sc.instances_outside_tables(src) == []


def test_vector_cases_reach_every_width_past_one_grid():
    past = set()
    for c in V.VEC_CASES:
        kvs = c.kvs()
        rows = int(np.prod([kv.numdofs for kv in kvs]))
        assert sc.spmv_gw(sc.patch_maxlen(kvs)) == c.gw, c.id
        if rows > sc.spmv_pass_rows(c.gw):
            past.add((c.gw, c.nc))
    assert past == {(gw, nc) for gw in sc.GWS for nc in (2, 3)}, sorted(past)


def test_new_abi_names_declared_bound_exported():
    hdr = open(os.path.join(ROOT, 'include', 'igx.h')).read()
    declared = set(re.findall(r'\b(igx_[a-z_0-9]+)\s*\(', hdr))
    bound = {name for name, _, _ in _lib.SYMBOLS}
    nm = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in NEW_NAMES:
        assert name in declared and name in bound, name
        assert re.search(r'\bT %s\b' % name, nm), name
    assert _lib.load().igx_version() == 101

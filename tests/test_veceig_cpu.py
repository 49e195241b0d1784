"""Vector-valued eigenproblems on the device (solvers.VectorEigenSystem, igx_solver_take_mass, k_block_spmm2; DESIGN.md section
27): what can be checked without a GPU.

- The new entry point is declared, bound and exported, and fails loudly (no crash, an error code and a message) on a null solver.
- Every refusal of VectorEigenSystem happens before any device work.
- with_block_spmm2_kernel reaches every (GW, MB, NM, NC), no instantiation is named outside it, and the GPU cases reach every
  one of them, with a case past one pass of scalar rows per group width.
- The controller on the golden matrices of the reference (elasticity on the quarter annulus, tests/golden/golden_veceig.npz) with
  the block-diagonal Kronecker model reaches the reference's eigenvalues.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from pyiga_amd import _lib, bspline, geometry, solvers

import _eig_model as EM
import _mpsolve_model as M
import _solver_cases as SC
import _veceig_cases as VC
import _veceig_model as VM
import _vecsolve_model as V
from test_vecsolve_cpu import _HostGeo, _no_device

from conftest import ROOT

MU_LAM = dict(mu=1.0, lam=2.0)


def _kvs(d, p=2, n=4):
    return (bspline.make_knots(p, 0.0, 1.0, n),) * d


# ---------------------------------------------------------------------------------------------
def test_take_mass_declared_bound_exported_and_loud():
    hdr = open(os.path.join(ROOT, 'include', 'igx.h')).read()
    declared = set(re.findall(r'\b(igx_[a-z_0-9]+)\s*\(', hdr))
    bound = {name for name, _, _ in _lib.SYMBOLS}
    nm = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert 'igx_solver_take_mass' in declared and 'igx_solver_take_mass' in bound
    assert re.search(r'\bT igx_solver_take_mass\b', nm)
    lib = _lib.load()
    assert lib.igx_solver_take_mass(None) == _lib.IGX_ERR_ARG
    with pytest.raises(_lib.IgxError, match='null solver'):
        _lib.check(lib.igx_solver_take_mass(None), 'igx_solver_take_mass')
    assert 'VectorEigenSystem' in solvers.__doc__


def test_vector_eigen_system_fails_loudly_without_gpu():
    """No device: IgxError, no host eigen-solver in its place."""
    code = ('import sys; sys.path.insert(0, %r)\n'
            'import numpy as np, scipy.linalg, scipy.sparse.linalg\n'
            'def _no(*a, **k):\n'
            '    raise AssertionError("host solver called")\n'
            'scipy.sparse.linalg.eigsh = scipy.sparse.linalg.lobpcg = scipy.linalg.eigh = _no\n'
            'import pyiga_amd\n'
            'from pyiga_amd import bspline, geometry, solvers\n'
            'kvs = (bspline.make_knots(2, 0.0, 1.0, 4),) * 2\n'
            'try:\n'
            '    S = solvers.VectorEigenSystem("(inner(grad(u), grad(v)) + inner(u, v)) * dx", kvs, np.arange(6),\n'
            '                                  bfuns=[("u", 2), ("v", 2)], geo=geometry.unit_square())\n'
            '    S.solve(k=2)\n'
            '    print("COMPUTED")\n'
            'except pyiga_amd._lib.IgxError as e:\n'
            '    print("RAISED", e)\n' % (ROOT,))
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1')
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, env=env)
    assert 'RAISED' in out.stdout and 'COMPUTED' not in out.stdout, out.stdout + out.stderr
    assert 'host solver called' not in out.stdout + out.stderr


# ---------------------------------------------------------------------------------------------
SIDES2 = np.arange(6)                                    # (any fixed dofs: the refusals come first)


@pytest.mark.parametrize('problem, kvs_dim, kwargs, match', [
    (V.ELASTICITY, 2, dict(bfuns=V.bfuns(2), **MU_LAM), 'geo'),                                      # no geo
    ('inner(grad(u), grad(v)) * dx', 2, dict(), 'scalar form'),                                      # a scalar form
    ('inner(u, v) * dx', 2, dict(bfuns=[('u', 2), ('v', 3)]), 'components'),                         # unequal component counts
    ('inner(u, v) * dx', 2, dict(bfuns=V.bfuns(4)), '2 or 3'),
    ('inner(u, v) * ds', 2, dict(bfuns=V.bfuns(2)), 'boundary'),
    ('inner(u, v) * dx', 1, dict(bfuns=V.bfuns(2)), 'surface'),                                      # a surface patch
    (V.ELASTICITY, 2, dict(bfuns=V.bfuns(2), mass='(u*v + inner((1.0, 2.0), grad(u))*v) * dx', **MU_LAM), 'mass'),    # not symmetric
    (V.ELASTICITY, 2, dict(bfuns=V.bfuns(2), mass='div(u)*div(v) * dx', **MU_LAM), 'mass'),          # not scalar
    (V.ELASTICITY, 2, dict(bfuns=V.bfuns(2), mass=2.5, **MU_LAM), 'mass'),                           # not a string
])
def test_refusals_before_any_device_work(monkeypatch, problem, kvs_dim, kwargs, match):
    _no_device(monkeypatch)
    kw = dict(kwargs)
    if match != 'geo':
        kw['geo'] = geometry.unit_square()
    with pytest.raises(ValueError, match=match):
        solvers.VectorEigenSystem(problem, _kvs(kvs_dim), SIDES2, **kw)


def test_refuses_a_form_object(monkeypatch):
    _no_device(monkeypatch)
    from pyiga_amd import form_assemblers
    with pytest.raises(ValueError, match='form string'):
        solvers.VectorEigenSystem(form_assemblers.FormAssembler, _kvs(2), SIDES2, geo=geometry.unit_square())


def test_table_refusals_before_any_assembly(monkeypatch):
    """What the coefficient tables decide (evaluated on the host Gauss grid): block tables that are not symmetric, and no fixed
    dof at all without a zeroth-order term; a fixed dof out of range."""
    _no_device(monkeypatch, host_patch=True)
    with pytest.raises(ValueError, match='not symmetric'):
        solvers.VectorEigenSystem(V.NONSYM, _kvs(2), SIDES2, bfuns=V.bfuns(2), geo=_HostGeo())
    for form in ('inner(grad(u), grad(v)) * dx', V.ELASTICITY):
        with pytest.raises(ValueError, match='subtract'):
            solvers.VectorEigenSystem(form, _kvs(2), None, bfuns=V.bfuns(2), geo=_HostGeo(), **MU_LAM)
    with pytest.raises(ValueError, match='out of range'):
        solvers.VectorEigenSystem(V.ELASTICITY, _kvs(2), [2 * 36], bfuns=V.bfuns(2), geo=_HostGeo(), **MU_LAM)


# ---------------------------------------------------------------------------------------------
def test_dispatch_reaches_every_instantiation_and_nothing_is_named_elsewhere():
    src = SC.read_source()
    inst, gws, mbs = VC.parse_block_spmm_dispatch(src)
    assert gws == {(64, 64), (32, 32), (16, 16), (8, 8), (None, 4)}
    assert mbs == {(4, 4), (8, 8), (None, 16)}
    assert inst == VC.INSTANCES and len(inst) == 60
    assert VC.block_spmm_outside_tables(src) == []
    # the launch and the occupancy query both go through the dispatch: k_block_spmm2 is launched nowhere by name
    assert not re.search(r'\bk_block_spmm2\s*<<<', src)


def test_case_table_reaches_every_instantiation():
    for case in VC.SMALL_CASES + VC.WRAP_CASES:
        assert SC.spmv_gw(SC.patch_maxlen(case.patch.kvs())) == case.patch.gw, case.id
    # block_products is NM = 2, block_product NM = 1: both run on every small case with every m of its columns
    reached = {(c.patch.gw, VC.eig_width(m), nm, c.nc) for c in VC.SMALL_CASES for m in c.columns for nm in (1, 2)}
    assert reached == VC.INSTANCES
    assert {c.patch.dim for c in VC.SMALL_CASES if c.nc == 2} == {2, 3} == {c.patch.dim for c in VC.SMALL_CASES if c.nc == 3}
    assert SC.parse_constants(SC.read_source()) == dict(BLOCK=VC.EC.BLOCK, NB_VEC=VC.EC.NB_VEC, NB_SPMV_MAX=VC.EC.NB_SPMV_MAX)
    # past one pass: more *scalar* rows than NB_SPMV_MAX * (BLOCK / GW), one case per group width, both component counts
    for gw in VC.GWS:
        rows = [int(np.prod([kv.numdofs for kv in c.patch.kvs()])) for c in VC.WRAP_CASES if c.patch.gw == gw]
        assert rows and max(rows) > VC.spmm_pass_rows(gw), gw
    assert sorted(c.nc for c in VC.WRAP_CASES) == [2, 2, 3, 3, 3]
    assert all(len(c.columns) == 1 for c in VC.WRAP_CASES)


# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def annulus2_factors(oracle, golden):
    return VM.component_factors(VM.annulus2_kvs(), golden('veceig')['annulus2_fixed'], 2, mats1d=M.mats1d_oracle(oracle))


def test_golden_fixture_is_what_its_script_says(golden):
    g = golden('veceig')
    for name, nc, N in (('annulus2', 2, 13 * 13), ('cylinder3', 3, 6 * 6 * 6)):
        lam, Vg, fixed, ks = g[name + '_lam'], g[name + '_V'], g[name + '_fixed'], g[name + '_ks']
        assert lam.shape == (12,) and Vg.shape == (nc * N, 12) and np.all(np.diff(lam) >= 0.0) and lam[0] > 0.0
        assert np.all(Vg[fixed] == 0.0) and len(ks) >= 2 and set(ks) <= {4, 6, 10}
        for k in ks:
            assert lam[k] - lam[k - 1] > 1e-3 * lam[k]
        assert 'layout=blocked' in str(g[name + '_desc'])
    K, M1 = VM.golden_csr(g, 'annulus2_K'), VM.golden_csr(g, 'annulus2_M1')
    assert abs(K - K.T).max() <= 1e-12 * abs(K).max() and abs(M1 - M1.T).max() <= 1e-14
    lam, Vd, free = EM.dense_eigh(K, VM.block_mass(M1, 2), g['annulus2_fixed'])
    assert (np.abs(lam[:12] - g['annulus2_lam']) <= 1e-11 * g['annulus2_lam']).all()


def test_host_model_reaches_the_golden_eigenvalues(golden, annulus2_factors):
    g = golden('veceig')
    ref = g['annulus2_lam']
    for k in g['annulus2_ks']:
        k = int(k)
        m = solvers.default_eig_block(k)
        lam, info, _ = VM.run_model(g, k, m, 0, annulus2_factors)
        print('k', k, 'block', m, 'iterations', info['iterations'], 'rel err', np.abs(lam[:k] - ref[:k]) / ref[:k])
        assert info['converged'].all() and info['failed'] is None and info['restarts'] == 0
        assert (np.abs(lam[:k] - ref[:k]) <= 1e-10 * ref[:k]).all()
        assert info['products'] == info['iterations'] + 1

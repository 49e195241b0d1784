"""BiCGStab without a GPU: the numpy model of the device iteration (tests/_bicgstab_model.py) against scipy's bicgstab on
oracle-assembled non-symmetric matrices, its breakdown on a skew-symmetric system, the new C ABI names, and the refusals of
FormSystem / MultipatchSystem(method='bicgstab') that come before any device work."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.linalg

from conftest import ROOT
from pyiga_amd import _lib, bspline, geometry, solvers

import _bicgstab_model as BM

HERE = os.path.dirname(os.path.abspath(__file__))
NEW_NAMES = ['igx_solver_create_general', 'igx_solver_set_method', 'igx_solver_last_breakdown']


def _restrict(A, fixed):
    free = np.setdiff1d(np.arange(A.shape[0]), fixed)
    return A.tocsr()[free][:, free].tocsr(), free


def _boundary(N):
    idx = np.indices(N).reshape(len(N), -1)
    on = np.zeros(idx.shape[1], dtype=bool)
    for k, n in enumerate(N):
        on |= (idx[k] == 0) | (idx[k] == n - 1)
    return np.nonzero(on)[0]


def _convdiff(oracle, p, n, diff=0.05):
    okvs = (oracle.make_knots(p, 0.0, 1.0, n),) * 3
    A = oracle.assemble_nonsymmetric('convdiff', okvs, oracle.geo_cylinder(), coeff=lambda x, y, z: diff + 0.0 * x)
    N = (n + p,) * 3
    return A, N


@pytest.mark.parametrize('precond', [None, 'jacobi'])
@pytest.mark.parametrize('diff', [1.0, 0.02])
def test_model_reproduces_scipy_iterates(oracle, precond, diff):
    A, N = _convdiff(oracle, 2, 3, diff)
    Aff, _ = _restrict(A, _boundary(N))
    b = np.random.default_rng(3).standard_normal(Aff.shape[0])
    dinv = 1.0 / Aff.diagonal()
    M = (lambda r: dinv * r) if precond else None
    Mop = scipy.sparse.linalg.LinearOperator(Aff.shape, matvec=M) if precond else None
    ref = []
    x_ref, info = scipy.sparse.linalg.bicgstab(Aff, b, rtol=1e-10, atol=0.0, maxiter=500, M=Mop,
                                               callback=lambda xk: ref.append(xk.copy()))
    assert info == 0
    mine = []
    x, inf = BM.bicgstab(Aff, b, tol=1e-10, maxiter=500, M=M, callback=lambda xk: mine.append(xk.copy()))
    assert inf['converged'] and inf['breakdown'] is None
    # scipy reports no iterate after an s-test stop; the model's last one is then its return value
    assert len(mine) in (len(ref), len(ref) + 1), (len(mine), len(ref))
    assert inf['iterations'] == len(mine)
    for k, (a, r) in enumerate(zip(mine, ref)):
        assert np.abs(a - r).max() <= 1e-9 * np.abs(r).max(), k
    assert np.abs(x - x_ref).max() <= 1e-9 * np.abs(x_ref).max()
    assert np.linalg.norm(b - Aff @ x) <= 1e-10 * np.linalg.norm(b) * (1 + 1e-6)


def test_model_freezes_after_the_stop():
    """A maxiter far beyond convergence changes nothing (the device runs frozen iterations with check_every > 1)."""
    rng = np.random.default_rng(0)
    A = scipy.sparse.random(60, 60, density=0.1, random_state=1) + 8.0 * scipy.sparse.eye(60)
    b = rng.standard_normal(60)
    x1, i1 = BM.bicgstab(A, b, tol=1e-12, maxiter=200)
    x2, i2 = BM.bicgstab(A, b, tol=1e-12, maxiter=i1['iterations'])
    assert i1 == i2 and np.array_equal(x1, x2)
    assert i1['converged'] and i1['relres'] <= 1e-12


def test_skew_symmetric_system_breaks_down_at_iteration_1(oracle):
    """Pure convection by the divergence-free field (y, -x) with every side fixed: R A R^T is skew-symmetric, so
    r0 . A r0 = 0 and alpha is undefined in the first iteration."""
    okvs = (oracle.make_knots(2, 0.0, 1.0, 6),) * 2
    table = [[None] * 4 for _ in range(4)]
    table[0][1] = lambda x, y: y
    table[0][2] = lambda x, y: -x
    A = oracle.assemble_nonsymmetric('form', okvs, oracle.geo_unit_cube(2), table=table)
    Aff, _ = _restrict(A, _boundary((8, 8)))
    assert abs(Aff + Aff.T).max() <= 1e-14 * abs(Aff).max()
    b = np.random.default_rng(5).standard_normal(Aff.shape[0])
    x, inf = BM.bicgstab(Aff, b, tol=1e-10, maxiter=100)
    assert inf['breakdown'] == 'alpha' and inf['iterations'] == 1 and not inf['converged']
    assert np.all(np.isfinite(x)) and np.array_equal(x, np.zeros_like(b))


def test_new_abi_names_declared_bound_exported():
    hdr = open(os.path.join(ROOT, 'include', 'igx.h')).read()
    declared = set(re.findall(r'\b(igx_[a-z_0-9]+)\s*\(', hdr))
    bound = {name for name, _, _ in _lib.SYMBOLS}
    nm = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in NEW_NAMES:
        assert name in declared and name in bound, name
        assert re.search(r'\bT %s\b' % name, nm), name
    for macro in ('IGX_METHOD_CG', 'IGX_METHOD_BICGSTAB', 'IGX_BREAKDOWN_RHO', 'IGX_BREAKDOWN_ALPHA', 'IGX_BREAKDOWN_OMEGA',
                  'IGX_BREAKDOWN_NONFINITE'):
        m = re.search(r'\b%s\s*=\s*(\d+)' % macro, hdr)
        assert m and int(m.group(1)) == getattr(_lib, macro), macro
    assert _lib.load().igx_version() == 101
    assert _lib.METHODS == {'cg': 0, 'bicgstab': 1}


def _kvs2():
    return (bspline.make_knots(2, 0.0, 1.0, 4),) * 2


@pytest.mark.parametrize('problem, kwargs', [
    ('(inner(grad(u), grad(v)) + Dx(u, 0, times=2) * v) * dx', {}),                 # second derivatives: parametric jet form
    ('inner(grad(u, parametric=True), grad(v)) * dx', {}),
    ('v * dx', {}),                                                                  # a functional
    ('u * v * ds', {}),                                                              # (not a volume form)
])
def test_form_system_refuses_host_valued_forms_before_the_device(monkeypatch, problem, kwargs):
    from pyiga_amd import assemblers

    def no_device(*a, **k):
        raise AssertionError('device patch created')
    monkeypatch.setattr(assemblers, 'DevicePatch', no_device)
    with pytest.raises(ValueError):
        solvers.FormSystem(problem, _kvs2(), 0.0, geo=geometry.unit_square(), **kwargs)


def test_form_system_refuses_bad_arguments_before_the_device(monkeypatch):
    from pyiga_amd import assemblers, form_assemblers

    def no_device(*a, **k):
        raise AssertionError('device patch created')
    monkeypatch.setattr(assemblers, 'DevicePatch', no_device)
    kvs = _kvs2()
    with pytest.raises(ValueError, match='method'):
        solvers.FormSystem('u*v*dx', kvs, 0.0, method='gmres', geo=geometry.unit_square())
    with pytest.raises(ValueError, match='geo'):
        solvers.FormSystem('u*v*dx', kvs, 0.0)
    with pytest.raises(ValueError, match='MultipatchSystem'):                         # a surface form (FormAssembler)
        solvers.FormSystem('u*v*dx', kvs[:1], 0.0, geo=geometry.unit_square())
    with pytest.raises(ValueError, match='MultipatchSystem'):
        solvers.FormSystem(form_assemblers.FormAssembler, kvs, 0.0, geo=geometry.unit_square())
    with pytest.raises(ValueError, match='MultipatchSystem'):
        solvers.FormSystem(object(), kvs, 0.0, geo=geometry.unit_square())
    with pytest.raises(ValueError, match='method'):
        solvers.PatchSystem(kvs, geometry.unit_square(), np.zeros(36), method='gmres')
    with pytest.raises(ValueError, match='method'):
        solvers.MultipatchSystem(None, 'u*v*dx', 'v*dx', method='gmres')


def test_device_solves_raise_without_gpu():
    """No host fallback: without a HIP device FormSystem(...).solve() and MultipatchSystem(..., method='bicgstab') raise
    IgxError, and none of scipy's host solvers is called."""
    code = ('import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n'
            'import numpy as np, scipy.sparse.linalg, scipy.linalg\n'
            'def _no(*a, **k):\n'
            '    raise AssertionError("host solver called")\n'
            'for mod, name in ((scipy.sparse.linalg, "bicgstab"), (scipy.sparse.linalg, "gmres"), (scipy.sparse.linalg, "cg"),\n'
            '                  (scipy.sparse.linalg, "spsolve"), (scipy.sparse.linalg, "splu"), (scipy.sparse.linalg, "factorized"),\n'
            '                  (np.linalg, "solve"), (scipy.linalg, "solve"), (scipy.linalg, "lu_factor")):\n'
            '    setattr(mod, name, _no)\n'
            'import pyiga_amd\n'
            'from pyiga_amd import bspline, geometry, solvers, assemble\n'
            'import _mpsolve_model as M\n'
            'kvs = (bspline.make_knots(2, 0.0, 1.0, 4),) * 2\n'
            'geo = geometry.quarter_annulus()\n'
            'form = "(inner(grad(u), grad(v)) + inner((x[1], -x[0]), grad(u)) * v) * dx"\n'
            'runs = {\n'
            '    "form": lambda: solvers.FormSystem(form, kvs, 0.0, geo=geo).solve(),\n'
            '    "mp": lambda: solvers.MultipatchSystem(M.lshape(p=2, n=4), form, "v*dx", method="bicgstab").solve(),\n'
            '}\n'
            'for name, run in runs.items():\n'
            '    try:\n'
            '        run()\n'
            '        print("COMPUTED", name)\n'
            '    except pyiga_amd._lib.IgxError as e:\n'
            '        print("RAISED", name)\n' % (ROOT, HERE))
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1')
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, env=env)
    for name in ('form', 'mp'):
        assert 'RAISED %s\n' % name in out.stdout, out.stdout + out.stderr
    assert 'COMPUTED' not in out.stdout and 'host solver called' not in out.stdout + out.stderr, out.stdout + out.stderr

"""Parabolic problems on the device (solvers.ParabolicSystem, igx_solver_*_parabolic / _dirk_*): what can be checked without a GPU.

- The tableaux of dirk_tableau: lower triangular, one diagonal value, stiffly accurate; their order conditions and R(-inf).
- The host model of the restricted DIRK (tests/_parabolic_model.py) reproduces the reference's trajectories of
  golden_parabolic.npz, and the full-vector lifted formulation the device runs equals it.
- Every refusal is a ValueError before any device work.
- The new ABI names are declared, bound and exported; igx_dirk_info's layout matches gcc's.
- ParabolicSystem fails loudly without a GPU.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from pyiga_amd import _lib, bspline, geometry, solvers

import _parabolic_model as P

from conftest import ROOT

NEW_NAMES = ('igx_solver_create_parabolic', 'igx_solver_take_values', 'igx_solver_set_dirk', 'igx_solver_dirk_run')
ORDER = {'implicit_euler': 1, 'crank_nicolson': 2, 'sdirk3': 3, 'sdirk21': 2, 'esdirk23': 2, 'esdirk34': 3}
L_STABLE = ('implicit_euler', 'sdirk3', 'sdirk21', 'esdirk23', 'esdirk34')
SCHEMES = {'cn': 'crank_nicolson', 'sdirk3': 'sdirk3', 'esdirk34': 'esdirk34'}


@pytest.mark.parametrize('name', solvers.DIRK_SCHEMES)
def test_tableaux_are_accepted(name):
    A = solvers.dirk_tableau(name)
    A2, gamma = solvers.check_tableau(A)
    s = A.shape[1]
    assert A.shape == (s + 1, s) and s <= _lib.IGX_DIRK_MAX_STAGES
    assert gamma > 0 and np.all(np.isin(np.diag(A[:s]), (0.0, gamma)))
    assert np.array_equal(A[s], A[s - 1])
    assert solvers.dirk_tableau(name) is not solvers.dirk_tableau(name)      # a fresh array each time


@pytest.mark.parametrize('name', sorted(ORDER))
def test_order_conditions(name):
    res = P.order_conditions(solvers.dirk_tableau(name))
    for p in range(1, ORDER[name] + 1):
        assert np.max(np.abs(res[p])) < 1e-12, (name, p, res[p])
    if ORDER[name] < 3:
        assert np.max(np.abs(res[ORDER[name] + 1])) > 1e-6


def test_dirk34_weights_as_the_reference_runs_them():
    """dirk34 keeps the coefficients the reference runs (main rule): their weights sum to 1.0211, not 1, and R(-inf) = -0.244
    (DESIGN.md section 16)."""
    A = solvers.dirk_tableau('dirk34')
    assert abs(A[-1].sum() - 1.0210930553737374) < 1e-15
    assert A[0, 0] == 0 and A[1, 0] == A[1, 1] == A[2, 2] == A[3, 3]


@pytest.mark.parametrize('name', solvers.DIRK_SCHEMES)
def test_stability_at_infinity(name):
    A = solvers.dirk_tableau(name)
    r = P.stability(A, -np.inf)
    if name in L_STABLE:
        assert abs(r) < 1e-6, (name, r)
    elif name == 'dirk34':
        assert abs(r + 0.244232642) < 1e-6, r          # (the reference's coefficients: not L-stable)
    else:
        assert abs(r + 1) < 1e-6, (name, r)
    # |R| <= 1 on the negative real axis (A-stable along it)
    for z in -np.logspace(-3, 6, 40):
        assert abs(P.stability(A, z)) <= 1 + 1e-12, (name, z)


def _golden_mats(oracle, case):
    if case == 'heat3':
        kvs = (oracle.make_knots(2, 0.0, 1.0, 6),) * 3
        geo = oracle.geo_cylinder()
        return oracle.assemble('mass', kvs, geo), oracle.assemble('stiffness', kvs, geo)
    kvs = (oracle.make_knots(3, 0.0, 1.0, 16),) * 2
    geo = oracle.geo_quarter_annulus()
    M = oracle.assemble('mass', kvs, geo)
    if case == 'heat2':
        return M, oracle.assemble('stiffness', kvs, geo)
    kappa = lambda x, y: 0.2 + 0.1 * x * y
    table = [[None, lambda x, y: y, lambda x, y: -x], [None, kappa, None], [None, None, kappa]]
    return M, oracle.assemble_nonsymmetric('form', kvs, geo, table=table)


GOLDEN_CASES = [('heat2', 'cn'), ('heat2', 'sdirk3'), ('heat2', 'esdirk34'), ('heat3', 'sdirk3'), ('heat3', 'cn'),
                ('cd2', 'sdirk3'), ('cd2', 'esdirk34')]


@pytest.mark.parametrize('case, scheme', GOLDEN_CASES)
def test_model_reproduces_the_reference(golden, oracle, case, scheme):
    g = golden('parabolic')
    pre = case + '_'
    M, K = _golden_mats(oracle, case)
    A = solvers.dirk_tableau(SCHEMES[scheme])
    U = g[pre + scheme + '_u']
    tau, t_end = float(g[pre + 'tau']), float(g[pre + 't_end'])
    nsteps = int(np.ceil(t_end / tau))
    args = (A, M, K, g[pre + 'rhs'], g[pre + 'bc_idx'], g[pre + 'bc_val'], g[pre + 'u0'], tau, nsteps)
    R = P.restricted_dirk(*args)
    L = P.lifted_dirk(*args)
    assert len(R) == len(U) == nsteps + 1
    scale = np.abs(U).max()
    assert max(np.abs(r - u).max() for r, u in zip(R, U)) / scale < 1e-10
    assert max(np.abs(l - r).max() for l, r in zip(L, R)) / scale < 1e-12
    assert np.allclose(g[pre + scheme + '_times'], np.arange(nsteps + 1) * tau, rtol=0, atol=1e-15)


def _kvs(d, p=2, n=4):
    return (bspline.make_knots(p, 0.0, 1.0, n),) * d


def _no_device(monkeypatch):
    from pyiga_amd import assemblers

    def no_device(*a, **k):
        raise AssertionError('device patch created')
    monkeypatch.setattr(assemblers, 'DevicePatch', no_device)


@pytest.mark.parametrize('scheme, match', [
    ('rk4', 'unknown DIRK scheme'),
    (np.array([[0.5, 0.0], [0.5, 0.5], [0.3, 0.7]]), 'stiffly accurate'),            # non-SA (as sdirk3_b)
    (np.array([[0.4, 0.0], [0.3, 0.5], [0.3, 0.5]]), 'two diagonal values'),
    (np.array([[0.5, 0.0, 0.0], [0.5, 0.0, 0.0], [0.2, 0.3, 0.5], [0.2, 0.3, 0.5]]), 'zero diagonal'),
    (np.array([[0.5, 0.1], [0.5, 0.5], [0.5, 0.5]]), 'lower triangular'),
    (np.array([[-0.5], [-0.5]]), 'positive'),
    (np.zeros((8, 7)), 'shape'),
])
def test_scheme_refusals(scheme, match):
    with pytest.raises(ValueError, match=match):
        solvers._scheme(scheme)


class _Stub(solvers.ParabolicSystem):
    """A ParabolicSystem without a device: integrate must refuse before touching the handle."""

    def __init__(self):
        self.handle = None
        self.box = ((0, 0), (3, 3))
        self._precond = None

    def _live(self):
        raise AssertionError('device work')


@pytest.mark.parametrize('kw, match', [
    (dict(scheme='sdirk3_b'), 'unknown DIRK scheme'),
    (dict(scheme=np.array([[0.5, 0.0], [0.5, 0.5], [0.3, 0.7]])), 'stiffly accurate'),
    (dict(tau=0.0), 'tau'),
    (dict(tau=-1e-3), 'tau'),
    (dict(t_end=0.0), 't_end'),
    (dict(t0=1.0, t_end=0.5), 't_end'),
    (dict(save_every=0), 'save_every'),
    (dict(precond='ilu'), 'preconditioner'),
])
def test_integrate_refusals_before_any_device_work(kw, match):
    args = dict(u0=np.zeros(9), tau=1e-3, t_end=1e-2)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        _Stub().integrate(**args)


@pytest.mark.parametrize('problem, kwargs, match', [
    ('inner(grad(u), grad(v)) * ds', {}, 'boundary'),
    ('inner(u, v) * dx', dict(method='gmres'), 'method'),
    ('(inner(grad(u), grad(v)) + inner((x[1], -x[0]), grad(u)) * v) * dx', dict(method='cg'), 'symmetric'),
])
def test_system_refusals_before_any_device_work(monkeypatch, problem, kwargs, match):
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match=match):
        solvers.ParabolicSystem(_kvs(2), geometry.unit_square(), 0.0, problem=problem, **kwargs)


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(ROOT, 'pyiga_amd', 'libigx.so')):
        ge.build()
    return _lib


def test_new_abi_declared_bound_exported(lib):
    hdr = open(os.path.join(ROOT, 'include', 'igx.h')).read()
    bound = {name for name, _, _ in lib.SYMBOLS}
    nm = subprocess.run(['nm', '-D', '--defined-only', lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in NEW_NAMES:
        assert name + '(' in hdr and name in bound, name
        assert ' T %s\n' % name in nm, name


def test_dirk_info_layout_matches_gcc(lib, tmp_path):
    src = tmp_path / 'sz.c'
    fields = [f for f, _ in lib.DirkInfo._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "igx.h"\nint main(){printf("%zu", sizeof(igx_dirk_info));' +
                   ''.join('printf(" %%zu", offsetof(igx_dirk_info, %s));' % f for f in fields) +
                   'printf(" %d %d %d\\n", IGX_DIRK_MAX_STAGES, IGX_ROLE_MASS, IGX_ROLE_OPERATOR); return 0;}')
    exe = tmp_path / 'sz'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    D = lib.DirkInfo
    assert out == [ctypes.sizeof(D)] + [getattr(D, f).offset for f in fields] + \
        [lib.IGX_DIRK_MAX_STAGES, lib.IGX_ROLE_MASS, lib.IGX_ROLE_OPERATOR]


def test_fails_loudly_without_gpu(lib):
    code = ('import sys; sys.path.insert(0, %r)\n'
            'import pyiga_amd\n'
            'from pyiga_amd import bspline, geometry, solvers\n'
            'kv = bspline.make_knots(2, 0.0, 1.0, 4)\n'
            'try:\n'
            '    solvers.ParabolicSystem((kv, kv), geometry.unit_square(), 1.0)\n'
            'except pyiga_amd._lib.IgxError as e:\n'
            '    print("RAISED", e)\n' % ROOT)
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1')
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, env=env)
    assert 'RAISED' in out.stdout, out.stdout + out.stderr

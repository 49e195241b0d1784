"""The device saddle-point solver without a device: the transposed layout, the host model's solves on the golden systems (the
yardstick of tests/test_saddle_gpu.py), the width table of the kernel cases, refusals that need no device, and the ABI."""
import os
import re

import numpy as np
import pytest
import scipy.sparse

from conftest import golden_csr

from oracle import iga_oracle as orc
from pyiga_amd import _lib, bspline, solvers

import _pair_cases as pc
import _pair_model as pm
import _saddle_cases as sc
import _saddle_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('cid', sc.TRANSPOSE_CASES)
def test_transposed_layout(cid, golden):
    """The model's transposed pattern is scipy's B.T.tocsr() of the golden pattern, and the permutation it implies carries the
    golden data to B.T.data exactly."""
    g, case = golden('pair'), pc.BY_ID[cid]
    form = case.forms[0]
    name = '%s_%s_blocked' % (cid, form.name)
    B = golden_csr(g, name)
    ncu = form.bfuns[0][1]
    B = scipy.sparse.csr_matrix(B[:, :case.shape[1]]) if ncu > 1 else B          # the first scalar block
    B.sort_indices()
    kvs_trial, kvs_test = case.kvs(bspline)
    rng = [pm.ranges(a, b) for a, b in zip(kvs_trial, kvs_test)]
    jlo, jhi = [r[0] for r in rng], [r[1] for r in rng]
    ntrial = [int(kv.numdofs) for kv in kvs_trial]
    indptr0, indices0 = sm.box_layout(jlo, jhi, ntrial)
    assert np.array_equal(indptr0, B.indptr) and np.array_equal(indices0, B.indices)
    indptr, indices, perm = sm.transposed_layout(jlo, jhi, ntrial)
    T = B.T.tocsr()
    T.sort_indices()
    assert np.array_equal(indptr, T.indptr) and np.array_equal(indices, T.indices)
    assert np.array_equal(B.data[perm], T.data)
    assert np.array_equal(np.sort(perm), np.arange(B.nnz))


def test_transposed_tables_are_ranges():
    jlo, jhi = np.array([0, 0, 1, 3]), np.array([2, 3, 4, 5])
    ilo, ihi, rpt = sm.transposed_tables(jlo, jhi, 5)
    assert ilo.tolist() == [0, 0, 1, 2, 3] and ihi.tolist() == [2, 3, 3, 4, 4] and rpt.tolist() == [0, 2, 5, 7, 9, 10]


@pytest.mark.parametrize('key', sorted(sc.MODEL, key=str))
def test_model_solves(key, golden):
    """The model MINRES converges on the golden systems; its iteration counts, errors and true residuals are the constants of
    _saddle_cases.py (counts within MODEL_ITER_SLACK, errors and residuals not above twice the recorded ones: they sit at the
    rounding level of the solve)."""
    name, which, tol = key
    its, err, res = sc.MODEL[key]
    S = sc.system(golden, name)
    u, info = sc.model_solve(S, which, tol, orc)
    e = abs(u - S.u).max() / abs(S.u).max()
    print('%s %s tol %.0e: %d iterations, err %.3e, relres %.3e, rhs mean / norm %.2e'
          % (name, which, tol, info['iterations'], e, info['relres'], abs(info['rhs_mean']) / info['rhs_norm']))
    assert info['converged'] and info['breakdown'] is None
    assert abs(info['iterations'] - its) <= sc.MODEL_ITER_SLACK
    assert e <= 2 * err and info['relres'] <= 2 * res
    if name == 'stokes' and which == 'unpinned':
        assert abs(info['rhs_mean']) <= sc.MODEL_RHS_MEAN * info['rhs_norm']


def test_model_pressure_normalisations(golden):
    """'mean' and 'first' shift the pressure of one solve: the velocity is the same."""
    S = sc.system(golden, 'stokes')
    u, _ = sc.model_solve(S, 'unpinned', 1e-12, orc)
    um = sm.normalise_pressure(u, S.nv, 'mean')
    p = um[S.nv:]
    assert abs(um[:S.nv] - u[:S.nv]).max() <= sc.MODEL_VELOCITY_DIFF and u[S.nv] == 0.0
    assert abs(p.mean()) <= p.size * sm.EPS * abs(p).max()          # (the mean of the shifted coefficients: rounding of p.size terms)


def test_model_viscosity(golden):
    """With the Schur scale a viscosity of 0.01 costs the iterations of viscosity 1; without it, more."""
    S = sc.system(golden, 'stokes')
    _, scaled = sc.model_solve(S, 'unpinned', 1e-8, orc, viscosity=0.01)
    _, unscaled = sc.model_solve(S, 'unpinned', 1e-8, orc, viscosity=0.01, scale=1.0)
    print('viscosity 0.01: %d iterations with the Schur scale, %d without' % (scaled['iterations'], unscaled['iterations']))
    assert scaled['converged'] and unscaled['converged']
    assert abs(scaled['iterations'] - sc.MODEL_VISCOSITY['scaled']) <= sc.MODEL_ITER_SLACK
    assert abs(unscaled['iterations'] - sc.MODEL_VISCOSITY['unscaled']) <= sc.MODEL_ITER_SLACK
    assert sc.MODEL_VISCOSITY['scaled'] <= 1.5 * sc.MODEL[('stokes', 'unpinned', 1e-8)][0] + 5
    assert sc.MODEL_VISCOSITY['scaled'] < sc.MODEL_VISCOSITY['unscaled']


def test_model_breakdowns():
    K = lambda x: np.array([2.0, -1.0]) * x
    x, it, conv, brk, _ = sm.minres(K, lambda r: -r, np.array([1.0, 1.0]), 1e-8, 10)
    assert not conv and brk == 'indefinite_precond' and it == 0 and not x.any()
    x, it, conv, brk, _ = sm.minres(lambda x: x * np.nan, lambda r: r, np.array([1.0, 1.0]), 1e-8, 10)
    assert not conv and brk == 'nonfinite' and not x.any()
    x, it, conv, brk, _ = sm.minres(K, lambda r: r, np.array([1.0, 1.0]), 1e-12, 10)
    assert conv and brk is None and it == 2 and abs(x - [0.5, -1.0]).max() < 1e-14


def test_kernel_cases_reach_every_width_and_one_grid_wrap():
    """The width rule is solve.hip's, and the kernel cases reach every (width, nc) instantiation of both dispatch tables; one case
    has more rows than a grid pass holds, for both kernels, at the narrowest width."""
    src = open(os.path.join(ROOT, 'pyiga_amd', 'csrc', 'solve.hip')).read()
    body = src[src.index('int spmv_gw('):]
    body = body[:body.index('\n}\n')]
    pairs = [(int(t), int(g)) for t, g in re.findall(r'maxlen >= (\d+) \? (\d+)', body)]
    for t, g in pairs:
        assert sc.spmv_gw(t) == g and sc.spmv_gw(t - 1) < g
    assert sorted({g for _, g in pairs} | {4}) == list(sc.GWS)
    sad = open(os.path.join(ROOT, 'pyiga_amd', 'csrc', 'solve_saddle.hip')).read()
    hdr = open(os.path.join(ROOT, 'pyiga_amd', 'csrc', 'solve_internal.h')).read()
    assert int(re.search(r'constexpr int NB_SPMV_MAX = (\d+);', hdr).group(1)) == sc.NB_SPMV_MAX
    assert int(re.search(r'constexpr int BLOCK = (\d+);', hdr).group(1)) == sc.BLOCK
    assert 'std::min<long long>(NB_SPMV_MAX / 2,' in sad
    for kernel in ('k_saddle_u', 'k_saddle_p'):
        inst = {(int(gw), int(nc)) for gw, nc in re.findall(r'\b%s<(\d+), \d+, (\d+)>' % kernel, sad)}
        assert inst == {(gw, nc) for gw in sc.GWS for nc in (2, 3)}
        reached = {(sc.widths(c.trial, c.test)[kernel == 'k_saddle_p'], c.nc) for c in sc.KERNEL_CASES}
        assert reached == inst, (kernel, sorted(inst - reached))
    big = sc.KERNEL_BY_ID['big-2']
    assert sc.widths(big.trial, big.test) == (4, 4)
    assert min(int(np.prod(sc.ndofs(big.trial))), int(np.prod(sc.ndofs(big.test)))) > sc.pass_rows(4)
    assert any(c.absent for c in sc.KERNEL_CASES) and any(c.pinned for c in sc.KERNEL_CASES)


def test_case_ranges_are_the_pair_model():
    """axis_ranges of _saddle_cases.py (from (p, n, mult) alone) equals the pair model's ranges from the knot vectors."""
    for case in sc.KERNEL_CASES[:-1]:
        kvs_u, kvs_p = sc.kernel_kvs(case, bspline)
        for k in range(len(case.trial)):
            jlo, jhi = pm.ranges(kvs_u[k], kvs_p[k])
            a, b = sc.axis_ranges(case.trial[k], case.test[k])
            assert np.array_equal(jlo, a) and np.array_equal(jhi, b)
        assert tuple(kv.numdofs for kv in kvs_u) == sc.ndofs(case.trial)


# ---------------------------------------------------------------------------------------------
# refusals without a device
def _spaces():
    return (tuple(bspline.make_knots(3, 0.0, 1.0, n, mult=2) for n in (3, 2)), tuple(bspline.make_knots(2, 0.0, 1.0, n) for n in (3, 2)))


class _NoGeo:
    dim = sdim = 2


def test_refuses_nonsymmetric_velocity_form():
    with pytest.raises(ValueError, match='BiCGStab.*not supported|not supported'):
        solvers.SaddlePointSystem(_spaces(), _NoGeo(), None, a='(inner(grad(u), grad(v)) + inner(dot(grad(u), w), v)) * dx',
                                  w=lambda x, y: (1.0 + 0 * x, 0 * x))


def test_refuses_bcs_out_of_range():
    kvs = _spaces()
    n = 2 * int(np.prod([kv.numdofs for kv in kvs[0]])) + int(np.prod([kv.numdofs for kv in kvs[1]]))
    with pytest.raises(ValueError, match='outside'):
        solvers.SaddlePointSystem(kvs, _NoGeo(), (np.array([0, n]), np.zeros(2)))
    with pytest.raises(ValueError, match='kvs_u, kvs_p'):
        solvers.SaddlePointSystem(kvs[0], _NoGeo(), None)


def test_refuses_unknown_solve_arguments():
    S = object.__new__(solvers.SaddlePointSystem)          # (no device: the arguments are checked before the handle is touched)
    with pytest.raises(ValueError, match='pressure'):
        S.solve(pressure='pin')
    with pytest.raises(ValueError, match='preconditioner'):
        S.solve(precond='ilu')
    with pytest.raises(ValueError, match='method'):
        S.set_method('gmres')


# ---------------------------------------------------------------------------------------------
# the ABI
NEW_FUNCTIONS = ('igx_solver_create_saddle', 'igx_solver_take_pair_block', 'igx_solver_set_saddle_schur', 'igx_solver_saddle_projection',
                 'igx_solver_download_pair_block', 'igx_solver_saddle_product_d', 'igx_solver_saddle_timing')


def test_abi():
    hdr = open(os.path.join(ROOT, 'include', 'igx.h')).read()
    lib_src = open(os.path.join(ROOT, 'pyiga_amd', '_lib.py')).read()
    for fn in NEW_FUNCTIONS:
        assert re.search(r'\bint\s+%s\(' % fn, hdr), fn
        assert "('%s'," % fn in lib_src, fn
    enums = dict((k, int(v)) for k, v in re.findall(r'\b(IGX_(?:METHOD|BREAKDOWN)_\w+) = (\d+)', hdr))
    assert enums == {'IGX_METHOD_CG': 0, 'IGX_METHOD_BICGSTAB': 1, 'IGX_METHOD_MINRES': 2, 'IGX_BREAKDOWN_RHO': 1,
                     'IGX_BREAKDOWN_ALPHA': 2, 'IGX_BREAKDOWN_OMEGA': 3, 'IGX_BREAKDOWN_NONFINITE': 4,
                     'IGX_BREAKDOWN_INDEFINITE_PRECOND': 5}
    for k, v in enums.items():
        assert getattr(_lib, k) == v
    assert _lib.METHODS == {'cg': 0, 'bicgstab': 1} and _lib.SADDLE_METHODS['minres'] == 2
    assert _lib.BREAKDOWNS[5] == 'indefinite_precond' and _lib.BREAKDOWNS[4] == 'nonfinite'

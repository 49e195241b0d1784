"""Host side of the eigen-solver: the projected eigenproblem, the LOBPCG controller on numpy operations
with the oracle's matrices, the refusals of EigenSystem that need no device, and the coverage of the kernel case table."""
import numpy as np
import pytest
import scipy.linalg

import _eig_cases as EC
import _eig_model as EM
import _solver_cases as SC
from pyiga_amd import solvers


# ---------------------------------------------------------------------------------------------
# rayleigh_ritz
@pytest.mark.parametrize('order', [6, 24, 48])
def test_rayleigh_ritz_matches_dense_eigh(order):
    rng = np.random.default_rng(order)
    m = order // 3
    A = rng.standard_normal((order, order))
    GK = A @ A.T + order * np.eye(order)
    B = rng.standard_normal((order, order))
    GM = B @ B.T + np.eye(order)
    lam, C, ok = solvers.rayleigh_ritz(GK, GM, m)
    w, V = scipy.linalg.eigh(GK, GM)
    assert ok and lam.shape == (m,) and C.shape == (order, m)
    assert np.abs(lam - w[:m]).max() <= 1e-12 * np.abs(w).max()
    assert np.abs(C.T @ GM @ C - np.eye(m)).max() <= 1e-12
    assert np.abs(C.T @ GK @ C - np.diag(lam)).max() <= 1e-11 * np.abs(w).max()
    # badly scaled blocks (a W block of tiny norm) do not change the answer
    s = np.ones(order)
    s[m:2 * m] = 1e-7
    lam2, C2, ok2 = solvers.rayleigh_ritz(GK * s[:, None] * s[None, :], GM * s[:, None] * s[None, :], m)
    assert ok2 and np.abs(lam2 - lam).max() <= 1e-10 * np.abs(w).max()


def test_rayleigh_ritz_reports_a_singular_mass_gram():
    rng = np.random.default_rng(3)
    S = rng.standard_normal((40, 12))
    S[:, 7] = S[:, 2] + S[:, 5]                        # dependent columns: the Gram matrix is singular to rounding
    GM = S.T @ S
    A = rng.standard_normal((40, 40))
    GK = S.T @ (A @ A.T) @ S
    lam, C, ok = solvers.rayleigh_ritz(GK, GM, 4)
    assert ok is False and lam is None and C is None
    for bad in (np.full((12, 12), np.nan), -np.eye(12), np.zeros((12, 12))):
        assert solvers.rayleigh_ritz(GK, bad, 4) == (None, None, False)
    assert solvers.rayleigh_ritz(np.full((12, 12), np.inf), np.eye(12), 4) == (None, None, False)


# ---------------------------------------------------------------------------------------------
# lobpcg_loop on numpy operations, the oracle's matrices
CASES = {'annulus': (3, 16, 2, 'geo_quarter_annulus'), 'square': (3, 16, 2, None), 'cylinder': (2, 6, 3, 'geo_cylinder'),
         'cube': (2, 6, 3, None)}


@pytest.fixture(scope='module')
def pencils(oracle):
    """name -> (K, M, fixed, dense eigenvalues): assembled and diagonalised once, never changed."""
    out = {}
    for name, (p, n, d, geo) in CASES.items():
        kv = oracle.make_knots(p, 0.0, 1.0, n)
        g = getattr(oracle, geo)() if geo else oracle.geo_unit_cube(d)
        K, M = oracle.assemble('stiffness', (kv,) * d, g), oracle.assemble('mass', (kv,) * d, g)
        N = int(round(K.shape[0] ** (1.0 / d)))
        fixed = EM.boundary_dofs((N,) * d)
        out[name] = (K, M, fixed, EM.dense_eigh(K, M, fixed)[0])
    return out


def run(pencil, m, k, seed=0, tol=1e-9, maxiter=400):
    K, M, fixed, _ = pencil
    ops = EM.NumpyOps(K, M, fixed, EM.start_block(K.shape[0], m, seed))
    lam, info = solvers.lobpcg_loop(ops, m, k, tol, maxiter)
    return lam, ops.b['X'][:, :k], info


@pytest.mark.parametrize('name', sorted(CASES))
def test_lobpcg_loop_reaches_the_dense_spectrum(pencils, name):
    K, M, fixed, dense = pencils[name]
    lam, U, info = run(pencils[name], 8, 6)
    assert info['converged'].all() and info['failed'] is None
    assert (np.abs(lam[:6] - dense[:6]) <= 1e-10 * dense[:6]).all(), np.abs(lam[:6] - dense[:6]) / dense[:6]
    assert np.abs(U.T @ (M @ U) - np.eye(6)).max() <= 1e-10
    assert np.abs(U[fixed]).max() == 0.0
    assert info['products'] == info['iterations'] + 1        # one block product per iteration, on W only
    assert (info['residuals'] <= 1e-9).all()
    lam2, U2, info2 = run(pencils[name], 8, 6)
    assert np.array_equal(lam, lam2) and np.array_equal(U, U2) and info2['iterations'] == info['iterations']


@pytest.mark.parametrize('m, k', [(6, 6), (4, 1)])
def test_lobpcg_loop_guard_columns(pencils, m, k):
    """k = m (no guard column: all of them must converge) and k = 1 (the others need not)."""
    K, M, fixed, dense = pencils['cylinder']
    lam, U, info = run(pencils['cylinder'], m, k)
    assert info['converged'].shape == (k,) and info['converged'].all()
    assert (np.abs(lam[:k] - dense[:k]) <= 1e-10 * dense[:k]).all()
    assert np.abs(U.T @ (M @ U) - np.eye(k)).max() <= 1e-10
    if k == 1:                                              # stopped on the first pair alone: fewer steps than all four take
        assert info['iterations'] < run(pencils['cylinder'], m, m)[2]['iterations']


def test_lobpcg_loop_gives_up_without_raising(pencils):
    K, M, fixed, _ = pencils['cube']
    X0 = EM.start_block(K.shape[0], 4, 0)
    X0[:, 3] = X0[:, 0]                                     # a start block of rank 3
    ops = EM.NumpyOps(K, M, fixed, X0)
    lam, info = solvers.lobpcg_loop(ops, 4, 2, 1e-9, 50)
    assert not info['converged'].any() and info['failed'] and info['iterations'] == 0
    lam, U, info = run(pencils['cube'], 4, 2, maxiter=3)    # out of iterations
    assert info['iterations'] == 3 and not info['converged'].all() and info['failed'] is None


# ---------------------------------------------------------------------------------------------
# refusals before any device work
def test_eigen_system_refusals_need_no_device(monkeypatch):
    from pyiga_amd import assemblers, bspline, geometry

    def no_device(*a, **k):
        raise AssertionError('device work before the refusal')
    monkeypatch.setattr(assemblers, 'DevicePatch', no_device)
    kv = bspline.make_knots(2, 0.0, 1.0, 4)
    kvs, geo = (kv, kv), geometry.unit_square()
    n = kv.numdofs ** 2
    sides = EM.boundary_dofs((kv.numdofs,) * 2)
    with pytest.raises(ValueError, match='subtract 1'):
        solvers.EigenSystem(kvs, geo)                                      # stiffness, no fixed dof
    with pytest.raises(ValueError, match='subtract 1'):
        solvers.EigenSystem(kvs, geo, problem='inner(grad(u), grad(v)) * dx')
    with pytest.raises(ValueError, match='not known to be symmetric'):
        solvers.EigenSystem(kvs, geo, sides, problem='(inner(grad(u), grad(v)) + inner((1.0, 2.0), grad(u)) * v) * dx')
    with pytest.raises(ValueError, match='not known to be symmetric'):
        solvers.EigenSystem(kvs, geo, sides, problem=assemblers.ConvDiffAssembler3D)
    with pytest.raises(ValueError, match='boundary form'):
        solvers.EigenSystem(kvs, geo, sides, problem='u * v * ds')
    with pytest.raises(ValueError, match='out of range'):
        solvers.EigenSystem(kvs, geo, [n])
    with pytest.raises(ValueError):
        solvers.EigenSystem(kvs, geo, sides, problem=assemblers.GeneralFunctionalAssembler2D)      # host-valued / not a matrix
    # the argument checks of solve()
    check = solvers._check_eig_args
    check(6, 9, 27)
    for k, block, n_free in ((0, 4, 100), (-1, 4, 100), (5, 4, 100), (6, 17, 100), (17, 17, 100), (2, 4, 11)):
        with pytest.raises(ValueError):
            check(k, block, n_free)
    assert [solvers.default_eig_block(k) for k in (1, 2, 6, 7, 12, 16)] == [3, 4, 9, 10, 16, 16]
    assert [solvers.eig_width(m) for m in (1, 4, 5, 8, 9, 16)] == [4, 4, 8, 8, 16, 16]
    with pytest.raises(ValueError):
        solvers.eig_width(17)


# ---------------------------------------------------------------------------------------------
# the kernel case table against the source
def test_case_table_reaches_every_block_kernel():
    src = SC.read_source()
    assert SC.parse_constants(src) == dict(BLOCK=EC.BLOCK, NB_VEC=EC.NB_VEC, NB_SPMV_MAX=EC.NB_SPMV_MAX)
    assert EC.parse_constants(src) == dict(NB_GRAM=EC.NB_GRAM, GR_RC=EC.GR_RC)
    inst, gws = EC.parse_spmm_dispatch(src)
    # the switch maps every group width to its own instantiation, the default to 4; nothing is instantiated elsewhere
    assert gws == {(64, 64), (32, 32), (16, 16), (8, 8), (None, 4)}
    assert inst == {(gw, mb, nm) for gw in EC.GWS for mb in EC.WIDTHS for nm in (1, 2)}
    assert EC.spmm_outside_tables(src) == []
    for kernel in ('k_gram', 'k_block_comb', 'k_resid'):
        assert EC.parse_widths(src, kernel) == set(EC.WIDTHS), kernel
    assert tuple(solvers.EIG_WIDTHS) == EC.WIDTHS
    # every case has the group width it claims
    for case in EC.SMALL_CASES + EC.WRAP_CASES:
        assert SC.spmv_gw(SC.patch_maxlen(case.patch.kvs())) == case.patch.gw, case.id
    reached = {(c.patch.gw, EC.eig_width(m)) for c in EC.SMALL_CASES + EC.WRAP_CASES for m in c.columns}
    assert reached == {(gw, mb) for gw in EC.GWS for mb in EC.WIDTHS}
    # 2D and 3D, and repeated knots on one axis
    assert {c.patch.dim for c in EC.SMALL_CASES} == {2, 3}
    assert any(mult > 1 for c in EC.SMALL_CASES for _, _, mult in c.patch.axes)
    # one case past the pass bound per group width
    for gw in EC.GWS:
        rows = [int(np.prod([kv.numdofs for kv in c.patch.kvs()])) for c in EC.WRAP_CASES if c.patch.gw == gw]
        assert rows and max(rows) > EC.spmm_pass_rows(gw), gw
    # the other block kernels: every width, fewer rows than a block, no multiple of 256, past every pass bound
    assert {EC.eig_width(m) for c in EC.ROWS_CASES for m in c.columns} == set(EC.WIDTHS)
    rows = [c.rows() for c in EC.ROWS_CASES]
    assert min(rows) < EC.BLOCK and any(r % 256 for r in rows)
    big = max(EC.ROWS_CASES, key=lambda c: c.rows())
    assert big.rows() > max(EC.vec_pass_rows(), EC.gram_pass_rows())
    assert {EC.eig_width(m) for m in big.columns} == set(EC.WIDTHS)

"""Host side of the multipatch eigen-solver: the dispatch of the CSR block product against its case
table, the oracle's summed matrices against the goldens of the reference, the LOBPCG controller with the V-cycle model on the
L-shape, the new ABI names and the refusals of MultipatchEigenSystem that need no device."""
import os
import subprocess

import numpy as np
import pytest

import _eig_model as EM
import _mg_model as G
import _mp_eig_cases as MC
import _mpsolve_model as M
import _solver_cases as SC
from pyiga_amd import solvers


# ---------------------------------------------------------------------------------------------
# the kernel case table against the source
def test_dispatch_reaches_every_csr_block_product():
    src = SC.read_source()
    inst, gws, us = MC.parse_csr_spmm_dispatch(src)
    assert gws == {(64, 64), (32, 32), (16, 16), (8, 8), (None, 4)}
    assert inst == {(gw, mb, nm) for gw in MC.GWS for mb in MC.WIDTHS for nm in (1, 2)} and len(inst) == 30
    assert MC.csr_spmm_outside_tables(src) == []
    # U: a compile-time expression in MB per group width (the table of DESIGN.md section 23), at least 1 at every width
    for gw, expr in us.items():
        for mb in MC.WIDTHS:
            assert int(eval(expr, {'MB': mb})) >= 1, (gw, expr, mb)
    # the launch and the occupancy query go through the table, the grid as eig_products sizes it
    body = SC._function_body(src, 'int eig_products(')
    assert body.count('with_csr_spmm2_kernel(') == 3 and 'NB_SPMV_MAX' in body


def test_case_table_reaches_every_group_width():
    ids = [c.id for c in MC.SMALL_CASES + MC.WRAP_CASES]
    assert len(set(ids)) == len(ids)
    for case in MC.SMALL_CASES + MC.WRAP_CASES:
        MP = case.mp.build()
        assert SC.spmv_gw(SC.max_row(SC.multipatch_pattern(MP))) == case.mp.gw, case.id
        if case in MC.WRAP_CASES:
            assert MP.numdofs > SC.NB_SPMV_MAX * (SC.BLOCK // case.mp.gw), case.id
    assert [c.mp.gw for c in MC.SMALL_CASES] == list(MC.GWS) and [c.mp.gw for c in MC.WRAP_CASES] == list(MC.GWS)
    reached = {(c.mp.gw, MC.eig_width(m)) for c in MC.SMALL_CASES for m in c.columns}
    assert reached == {(gw, mb) for gw in MC.GWS for mb in MC.WIDTHS}
    assert {MC.eig_width(m) for c in MC.WRAP_CASES for m in c.columns} == set(MC.WIDTHS)
    assert MC.ROWS_CASE.build().numdofs % 256 != 0
    assert {MC.eig_width(m) for m in MC.ROWS_COLUMNS} == set(MC.WIDTHS)


# ---------------------------------------------------------------------------------------------
# the oracle's summed matrices against the reference's
@pytest.mark.parametrize('name', sorted(MC.GOLDEN_CASES))
def test_oracle_sums_reproduce_the_golden_eigenvalues(oracle, golden, name):
    g = golden('mp_eig')
    domain, p, n = MC.GOLDEN_CASES[name]
    MP, _ = MC.golden_domain(name)
    fixed = MC.outer_dofs(MP, domain)
    assert np.array_equal(fixed, g[name + '_fixed'])
    K, Mm = MC.oracle_sums(oracle, MP, domain, p, n)
    lam, _, _ = EM.dense_eigh(K, Mm, fixed)
    ref = g[name + '_lam']
    assert (np.abs(lam[:ref.size] - ref) <= 1e-10 * ref).all(), np.abs(lam[:ref.size] - ref) / ref
    V = g[name + '_V']
    assert V.shape == (MP.numdofs, ref.size) and np.abs(V[fixed]).max() == 0.0
    assert np.abs(V.T @ (Mm @ V) - np.eye(ref.size)).max() <= 1e-10


# ---------------------------------------------------------------------------------------------
# lobpcg_loop on numpy operations with the model V-cycle, the L-shape at p = 3
@pytest.fixture(scope='module')
def lshape_runs(oracle):
    """n -> (lam, info, K, M, fixed) of the model run with V(1,1) (k = 6, block 9, tol 1e-9, seed 0; the coarsest level 4 spans),
    and the Jacobi run at n = 32: each solved once."""
    geos = MC.oracle_geos(oracle, 'lshape')
    out = {}
    for n, nlev in ((16, 3), (32, 4)):
        As, MPs, fixed = G.oracle_levels(oracle, M.lshape, geos, 3, n, nlev, MC.LSHAPE_OUTER)
        model = G.Model(As, MPs, fixed)
        K = As[0]
        Mm = MC.oracle_sums(oracle, MPs[0], 'lshape', 3, n, kinds=('mass',))[0]
        X0 = EM.start_block(K.shape[0], 9, 0)

        def vcycles(R):
            return np.stack([model.apply_full(R[:, j]) for j in range(R.shape[1])], axis=1)
        ops = EM.NumpyOps(K, Mm, fixed[0], X0, vcycles)
        lam, info = solvers.lobpcg_loop(ops, 9, 6, 1e-9, 200)
        out[n] = (lam[:6], info, K, Mm, fixed[0])
    d = K.diagonal()
    ops = EM.NumpyOps(K, Mm, fixed[0], X0, lambda R: R / d[:, None])
    out['jacobi'] = solvers.lobpcg_loop(ops, 9, 6, 1e-9, 1000)[1]
    return out


def test_model_vcycle_reaches_the_dense_spectrum(lshape_runs):
    lam, info, K, Mm, fixed = lshape_runs[16]
    dense = EM.dense_eigh(K, Mm, fixed)[0][:6]
    assert info['converged'].all() and info['failed'] is None
    assert (np.abs(lam - dense) <= 1e-10 * dense).all(), np.abs(lam - dense) / dense
    assert 0.0 < lam[0] / 9.6397238440219 - 1.0 <= 6.4e-4                   # the L-shaped membrane (measured 3.197e-4)
    assert -1e-10 <= lam[2] / (2 * np.pi ** 2) - 1.0 <= 4e-9                # the smooth third eigenfunction: exactly 2 pi^2


def test_model_iterations_do_not_grow_and_beat_jacobi(lshape_runs):
    it16, it32, itj = lshape_runs[16][1]['iterations'], lshape_runs[32][1]['iterations'], lshape_runs['jacobi']['iterations']
    print('V(1,1) model iterations', it16, it32, 'jacobi at n = 32:', itj)
    assert lshape_runs[32][1]['converged'].all() and lshape_runs['jacobi']['converged'].all()
    assert abs(it16 - it32) <= 2                                            # (observed 20 and 20 at this tol)
    assert itj >= 2 * it32                                                  # (observed 123 against 20)


# ---------------------------------------------------------------------------------------------
def test_new_abi_names_are_declared_bound_and_exported():
    from pyiga_amd import _lib
    root = SC.ROOT
    with open(os.path.join(root, 'include', 'igx.h')) as f:
        header = f.read()
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    for name in ('igx_multipatch_values_d', 'igx_solver_set_mass_d'):
        assert ('int  %s(' % name) in header, name
        assert name in bound and len(bound[name][1]) == 2, name
    lib = os.path.join(root, 'pyiga_amd', 'libigx.so')
    if os.path.exists(lib):                                                 # (the built library, where there is one)
        syms = subprocess.run(['nm', '-D', '--defined-only', lib], capture_output=True, text=True).stdout
        for name in ('igx_multipatch_values_d', 'igx_solver_set_mass_d'):
            assert (' T ' + name) in syms, name
    assert set(solvers.MultipatchEigenSystem.PRECONDS) == {None, 'none', 'jacobi', 'mg'}


# ---------------------------------------------------------------------------------------------
# refusals before any device work
def test_multipatch_eigen_system_refusals_need_no_device(monkeypatch):
    from pyiga_amd import assemblers, multipatch

    def no_device(*a, **k):
        raise AssertionError('device work before the refusal')
    monkeypatch.setattr(assemblers, 'DevicePatch', no_device)
    monkeypatch.setattr(multipatch.Multipatch, '_device', no_device)
    monkeypatch.setattr(multipatch.Multipatch, '_sum_system', no_device)
    MP = M.lshape(p=2, n=4)
    sides = MC.outer_dofs(MP, 'lshape')
    E = solvers.MultipatchEigenSystem
    with pytest.raises(ValueError, match='subtract 1'):
        E(MP)                                                               # stiffness, no fixed dof
    with pytest.raises(ValueError, match='subtract 1'):
        E(MP, problem='inner(grad(u), grad(v)) * dx')
    with pytest.raises(ValueError, match='not known to be symmetric'):
        E(MP, sides, problem='(inner(grad(u), grad(v)) + inner((1.0, 2.0), grad(u)) * v) * dx')
    with pytest.raises(ValueError, match='not known to be symmetric'):
        E(MP, sides, problem=assemblers.ConvDiffAssembler3D)
    with pytest.raises(ValueError, match='boundary form'):
        E(MP, sides, problem='u * v * ds')
    with pytest.raises(ValueError, match='out of range'):
        E(MP, [MP.numdofs])
    with pytest.raises(ValueError):
        E(MP, sides, problem=assemblers.GeneralFunctionalAssembler2D)       # host-valued / not a matrix
    with pytest.raises(ValueError):
        E(MP, sides, problem='inner(u, v) * dx', bfuns=[('u', 2), ('v', 2)])    # vector-valued: `bfuns` is no input of a scalar form
    # solve() checks its arguments, and refuses Schwarz by name, before it asks for the device solver
    S = object.__new__(E)
    S.n, S.n_free, S.handle = MP.numdofs, MP.numdofs - sides.size, None
    for kw in (dict(k=0), dict(k=5, block=4), dict(k=2, block=17), dict(k=1, block=S.n_free // 3 + 1)):
        with pytest.raises(ValueError):
            S.solve(**kw)
    with pytest.raises(ValueError, match="not offered for eigenproblems.*'mg'"):
        S.solve(k=2, precond='schwarz')
    with pytest.raises(ValueError, match="not offered for eigenproblems.*'mg'"):
        S.set_precond('schwarz')

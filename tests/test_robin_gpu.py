"""Robin / Neumann boundary terms of the device-resident systems against the reference's data (tests/golden/golden_robin.npz,
made by tests/golden/make_golden_robin.py): the summed matrix and load through ``Multipatch.assemble_system``, the solutions of
``PatchSystem`` / ``FormSystem`` / ``MultipatchSystem`` (``max|u - u_ref| / max|u_ref| <= 1e-9`` at ``tol=1e-13``, the measure of
tests/test_solve_gpu.py), the trajectories of ``ParabolicSystem`` (the bound of tests/test_parabolic_gpu.py for its golden
trajectories), the shifted Kronecker preconditioner of the pure-Robin problem, and that the matrix never comes down."""
import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.linalg

import _robin_cases as rc
from conftest import golden_csr, rel_maxdiff

pytestmark = pytest.mark.gpu

K = 'inner(grad(u),grad(v))*dx'
RTOL = 1e-12          # matrix and load parity: tests/test_gpu_parity.py, tests/test_multipatch_gpu.py (golden systems)


def _rel(u, ref):
    return float(np.abs(u - ref).max() / np.abs(ref).max())


def _bcs(g, prefix):
    idx = g[prefix + 'bc_idx']
    return (idx, g[prefix + 'bc_val']) if idx.size else None


def _one_patch(kvs, geo):
    from pyiga_amd import assemble
    MP = assemble.Multipatch([(kvs, geo)])
    MP.finalize()
    return MP


@pytest.mark.parametrize('prefix,problem,extra,scale', [('robin2_', K, {}, 1.0), ('robin3_', K, {}, 1.0),
                                                         ('cd2_', rc.CD2_FORM, dict(diff_coeff=rc.kappa2), 1.0), ('heat2_', K, {}, 4.0)])
def test_summed_matrix_and_load_one_patch(golden, prefix, problem, extra, scale):
    g = golden('robin')
    kvs, geo, terms = rc.golden_patch_case(prefix)
    f = rc.f2 if len(kvs) == 2 else rc.f3
    MP = _one_patch(kvs, geo)
    try:
        A, b = MP.assemble_system(problem, 'f*v*dx', f=lambda *x: scale * f(*x), boundary_terms=rc.boundary_terms([(0, t) for t in terms], patch=True),
                                  **extra)
    finally:
        MP.close()
    W = golden_csr(g, prefix + 'A')
    assert rel_maxdiff(A, W) <= RTOL, (prefix, rel_maxdiff(A, W))
    assert np.abs(b - g[prefix + 'b']).max() <= RTOL * np.abs(g[prefix + 'b']).max()
    # ... and the terms are in it: without them the system differs
    assert rel_maxdiff(golden_csr(g, prefix + 'A0'), W) > 1e-3


def test_summed_matrix_and_load_multipatch(golden):
    g = golden('robin')
    MP = rc.lshape()
    try:
        for p in range(3):
            assert np.array_equal(MP.patch_to_global_idx(p), g['mp_p2g%d' % p])
        A, b = MP.assemble_system(K, 'f*v*dx', f=rc.fmp, boundary_terms=rc.boundary_terms(rc.MPTERMS, patch=True))
    finally:
        MP.close()
    W = golden_csr(g, 'mp_A')
    assert rel_maxdiff(A, W) <= RTOL, rel_maxdiff(A, W)
    assert np.abs(b - g['mp_b']).max() <= RTOL * np.abs(g['mp_b']).max()


@pytest.mark.parametrize('prefix', ['robin2_', 'robin3_'])
def test_patch_system_solution(golden, prefix):
    from pyiga_amd import solvers
    g = golden('robin')
    kvs, geo, terms = rc.golden_patch_case(prefix)
    S = solvers.PatchSystem(kvs, geo, rc.f2 if len(kvs) == 2 else rc.f3, _bcs(g, prefix), boundary_terms=rc.boundary_terms(terms))
    try:
        assert np.abs(S.b - g[prefix + 'b']).max() <= RTOL * np.abs(g[prefix + 'b']).max()
        for precond in ('kron', 'jacobi'):
            u = S.solve(tol=1e-13, maxiter=2000, precond=precond)
            print(prefix, precond, 'iterations', S.info['iterations'], 'rel. error %.2e' % _rel(u, g[prefix + 'u']))
            assert S.info['converged'] and _rel(u, g[prefix + 'u']) <= 1e-9, (prefix, precond, S.info, _rel(u, g[prefix + 'u']))
        u2 = S.solve(tol=1e-13, maxiter=2000, precond='jacobi')
        assert np.array_equal(u, u2)                              # two solves of one system: bit-identical
        # the Dirichlet values win on the dofs a Robin side shares with the fixed side
        assert np.array_equal(u[g[prefix + 'bc_idx']], g[prefix + 'bc_val'])
    finally:
        S.close()


def test_pure_robin_shifted_kron_and_jacobi(golden):
    """robin2n_: no fixed dof.  Both preconditioners converge to the reference's solution; the counts are printed (and recorded by
    tools/robin_timing.py), not asserted against a number."""
    from pyiga_amd import solvers
    g = golden('robin')
    kvs, geo, terms = rc.golden_patch_case('robin2n_')
    S = solvers.PatchSystem(kvs, geo, rc.f2, None, boundary_terms=rc.boundary_terms(terms))
    try:
        want = sum(float(g['robin2n_R%d' % k].sum()) for k in range(2))
        assert abs(S._sigma - want) <= 1e-12 * abs(want)          # 1^T R 1 from the faces' Gauss grids = the entry sums of the face matrices
        its = {}
        for precond in ('kron', 'jacobi'):
            u = S.solve(tol=1e-13, maxiter=3000, precond=precond)
            its[precond] = S.info['iterations']
            assert S.info['converged'] and _rel(u, g['robin2n_u']) <= 1e-9, (precond, S.info, _rel(u, g['robin2n_u']))
        print('pure Robin 2D p=3 n=8: iterations', its)
    finally:
        S.close()
    # without terms the preconditioner keeps today's factors: no shift
    S0 = solvers.PatchSystem(kvs, geo, rc.f2, _bcs(g, 'robin2_'))
    try:
        U, lam, mode = S0._kron_factors()
        U1, lam1, _ = solvers.fastdiag_factors(kvs, S0.box[0], S0.box[1], True)
        assert all(np.array_equal(a, b) for a, b in zip(lam, lam1))
    finally:
        S0.close()


def test_form_system_convection_diffusion(golden):
    from pyiga_amd import solvers
    g = golden('robin')
    kvs, geo, terms = rc.golden_patch_case('cd2_')
    S = solvers.FormSystem(rc.CD2_FORM, kvs, rc.f2, _bcs(g, 'cd2_'), geo=geo, diff_coeff=rc.kappa2, boundary_terms=rc.boundary_terms(terms))
    try:
        assert S.method == 'bicgstab'
        u = S.solve(tol=1e-13, maxiter=2000)
        assert S.info['converged'] and _rel(u, g['cd2_u']) <= 1e-9, (S.info, _rel(u, g['cd2_u']))
        assert np.array_equal(u, S.solve(tol=1e-13, maxiter=2000))
    finally:
        S.close()


@pytest.mark.parametrize('precond', [None, 'jacobi', 'schwarz'])
def test_multipatch_system_solution(golden, precond):
    from pyiga_amd import solvers
    g = golden('robin')
    MP = rc.lshape()
    try:
        S = solvers.MultipatchSystem(MP, K, 'f*v*dx', _bcs(g, 'mp_'), f=rc.fmp, boundary_terms=rc.boundary_terms(rc.MPTERMS, patch=True))
        u = S.solve(tol=1e-13, maxiter=3000, precond=precond)
        assert S.info['converged'] and _rel(u, g['mp_u']) <= 1e-9, (precond, S.info, _rel(u, g['mp_u']))
        assert np.array_equal(u, S.solve(tol=1e-13, maxiter=3000, precond=precond))
        with pytest.raises(ValueError, match='boundary'):
            S.solve(tol=1e-13, precond='mg')
        with pytest.raises(ValueError, match='boundary'):
            S.set_multigrid()
        S.close()
    finally:
        MP.close()


def test_multipatch_load_only_term_with_multigrid(golden):
    """A term without a matrix leaves the hierarchy of 'mg' valid.  Expected solution: spsolve of the reference's volume matrix
    with the reference's face load added to its load vector."""
    from pyiga_amd import solvers
    g = golden('robin')
    A = golden_csr(g, 'mp_A0').tocsr()
    b = g['mp_b0'].copy()
    b[g['mp_p2g0'][g['mp_R0_dofs']]] += g['mp_r0']
    idx, vals = g['mp_bc_idx'], g['mp_bc_val']
    free = np.setdiff1d(np.arange(b.size), idx)
    want = np.zeros(b.size)
    want[idx] = vals
    want[free] = scipy.sparse.linalg.spsolve(A[free][:, free].tocsc(), b[free] - A[free][:, idx] @ vals)
    MP = rc.lshape()
    try:
        bd, _, load, inp = rc.MPTERMS[0][1]
        S = solvers.MultipatchSystem(MP, K, 'f*v*dx', (idx, vals), f=rc.fmp, boundary_terms=[solvers.BoundaryTerm(bd, rhs=load, patch=0, **inp)])
        u = S.solve(tol=1e-13, maxiter=500, precond='mg')
        assert S.info['converged'] and _rel(u, want) <= 1e-9, (S.info, _rel(u, want))
        S.close()
    finally:
        MP.close()


@pytest.mark.parametrize('scheme,name', [('sdirk3', 'sdirk3'), ('cn', 'crank_nicolson')])
def test_parabolic_trajectories(golden, scheme, name):
    from pyiga_amd import solvers
    g = golden('robin')
    kvs, geo, terms = rc.golden_patch_case('heat2_')
    S = solvers.ParabolicSystem(kvs, geo, lambda x, y: 4.0 * rc.f2(x, y), None, boundary_terms=rc.boundary_terms(terms))
    try:
        assert S.method == 'cg'
        assert np.abs(S.b - g['heat2_b']).max() <= RTOL * np.abs(g['heat2_b']).max()
        times, sols = S.integrate(g['heat2_u0'], float(g['heat2_tau']), float(g['heat2_t_end']), scheme=name, tol=1e-12)
        U = g['heat2_%s_u' % scheme]
        assert np.allclose(times, g['heat2_%s_times' % scheme], rtol=0, atol=1e-15)
        err = max(np.abs(a - b).max() for a, b in zip(sols, U)) / max(np.abs(b).max() for b in U)
        assert len(sols) == len(U) and err < 1e-8, (scheme, err)
        # the terms matter at this bound: the trajectory without them is far away
        S0 = solvers.ParabolicSystem(kvs, geo, lambda x, y: 4.0 * rc.f2(x, y), None)
        try:
            _, sols0 = S0.integrate(g['heat2_u0'], float(g['heat2_tau']), float(g['heat2_t_end']), scheme=name, tol=1e-12)
        finally:
            S0.close()
        assert np.abs(sols0[-1] - U[-1]).max() > 1e-4 * np.abs(U[-1]).max()
    finally:
        S.close()


def test_matrix_and_face_matrix_never_leave_the_device(golden, monkeypatch):
    """3D: neither the volume values nor those of the face patches come down, and no pattern is requested."""
    from pyiga_amd import assemblers, solvers
    orig = assemblers.DevicePatch.assemble
    seen = []

    def no_pattern(self, *a, **k):
        raise AssertionError('pattern requested')

    def device_only(self, kind, algo='auto', to_host=True):
        if to_host:
            raise AssertionError('matrix values downloaded')
        seen.append(self.dim)
        return orig(self, kind, algo=algo, to_host=False)
    monkeypatch.setattr(assemblers.DevicePatch, 'pattern', no_pattern)
    monkeypatch.setattr(assemblers.DevicePatch, 'assemble', device_only)
    monkeypatch.setattr(assemblers.DevicePatch, 'csr', no_pattern)
    g = golden('robin')
    kvs, geo, terms = rc.golden_patch_case('robin3_')
    S = solvers.PatchSystem(kvs, geo, g['robin3_b0'], _bcs(g, 'robin3_'), boundary_terms=rc.boundary_terms(terms))
    try:
        u = S.solve(tol=1e-13, maxiter=2000)
        assert _rel(u, g['robin3_u']) <= 1e-9
        assert seen.count(3) == 1 and seen.count(2) == 3          # the volume once, one face patch per matrix term
    finally:
        S.close()


def test_nonsymmetric_boundary_matrix_needs_bicgstab(golden):
    from pyiga_amd import solvers
    g = golden('robin')
    kvs, geo, _ = rc.golden_patch_case('robin2_')
    skew = solvers.BoundaryTerm('right', matrix='(alpha*u*v + inner((1.0, 2.0), grad(u)) * v) * ds', alpha=rc.alpha2)
    with pytest.raises(ValueError, match='symmetric'):
        solvers.PatchSystem(kvs, geo, rc.f2, _bcs(g, 'robin2_'), boundary_terms=[skew])
    S = solvers.PatchSystem(kvs, geo, rc.f2, _bcs(g, 'robin2_'), boundary_terms=[skew], method='bicgstab')
    try:
        u = S.solve(tol=1e-12, maxiter=2000, precond='jacobi')
        assert S.info['converged'] and np.isfinite(u).all()
    finally:
        S.close()

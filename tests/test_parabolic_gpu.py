"""Parabolic problems integrated on the device by DIRK schemes (solvers.ParabolicSystem), on an MI355X.

1. Exact stability function: discrete eigenvectors of the identity map of the unit square / cube take u_N = R(-tau lam)^N u0,
   and with the Kronecker preconditioner (the exact inverse there) every stage solve takes one iteration.
2. The reference's trajectories of golden_parabolic.npz (heat 2D / 3D, convection-diffusion by BiCGStab).
3. The host model at larger sizes.  4. Conservation without Dirichlet dofs.  5. The steady state of implicit Euler.
6. The SpMV is R (M + tau gamma K) R^T.  7. Saving, determinism, re-assembly of the patch.  8. Refusals on the device path.
"""
import numpy as np
import pytest
import scipy.sparse

from pyiga_amd import assemble, bspline, geometry, solvers

import _parabolic_model as P

pytestmark = pytest.mark.gpu

CD2_FORM = '(inner(diff_coeff*grad(u),grad(v))+inner((x[1],-x[0]),grad(u))*v)*dx'
SCHEMES = {'cn': 'crank_nicolson', 'sdirk3': 'sdirk3', 'esdirk34': 'esdirk34'}


def _boundary(ndofs):
    idx = np.indices(ndofs).reshape(len(ndofs), -1)
    on = np.zeros(idx.shape[1], dtype=bool)
    for k, n in enumerate(ndofs):
        on |= (idx[k] == 0) | (idx[k] == n - 1)
    return np.flatnonzero(on)


def _relmax(states, ref):
    return max(np.abs(a - b).max() for a, b in zip(states, ref)) / max(np.abs(b).max() for b in ref)


@pytest.mark.parametrize('d, p, n', [(2, 3, 16), (3, 2, 6)])
def test_exact_stability_function(d, p, n):
    kvs = (bspline.make_knots(p, 0.0, 1.0, n),) * d
    geo = geometry.unit_square() if d == 2 else geometry.unit_cube()
    ndofs = tuple(kv.numdofs for kv in kvs)
    fixed = _boundary(ndofs)
    S = solvers.ParabolicSystem(kvs, geo, 0.0, bcs=(fixed, np.zeros(fixed.size)))
    try:
        U, lam, _ = solvers.fastdiag_factors(kvs, (1,) * d, tuple(m - 1 for m in ndofs), True)
        m = len(lam[0])
        lam_min, lam_max = d * lam[0][0], d * lam[0][-1]
        tau = 0.1 / lam_min
        for k in (0, m // 2, m - 1):                              # tau lam from 0.1 to tau lam_max
            mode = U[0][:, k]
            for e in range(1, d):
                mode = np.multiply.outer(mode, U[e][:, k])
            u0 = np.zeros(ndofs)
            u0[(slice(1, -1),) * d] = mode
            u0 = u0.ravel()
            z = -tau * d * lam[0][k]
            for name in solvers.DIRK_SCHEMES:
                times, sols = S.integrate(u0, tau, 2.5 * tau, scheme=name, precond='kron')
                assert len(sols) == 4 and S.info['converged']
                R = P.stability(solvers.dirk_tableau(name), z)
                err = np.abs(sols[-1] - R ** 3 * u0).max() / np.abs(u0).max()
                assert err < 1e-10, (name, k, z, err)
                assert np.all(S.info['stage_iterations'] == 1), (name, k, S.info['stage_iterations'])
        assert lam_max > lam_min
    finally:
        S.close()


def _golden_system(g, case):
    pre = case + '_'
    bcs = (g[pre + 'bc_idx'], g[pre + 'bc_val'])
    if case == 'heat3':
        kvs = (bspline.make_knots(2, 0.0, 1.0, 6),) * 3
        geo = geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.quarter_annulus())
        return solvers.ParabolicSystem(kvs, geo, g[pre + 'rhs'], bcs)
    kvs = (bspline.make_knots(3, 0.0, 1.0, 16),) * 2
    geo = geometry.quarter_annulus()
    if case == 'heat2':
        return solvers.ParabolicSystem(kvs, geo, g[pre + 'rhs'], bcs)
    return solvers.ParabolicSystem(kvs, geo, g[pre + 'rhs'], bcs, problem=CD2_FORM, diff_coeff=lambda x, y: 0.2 + 0.1 * x * y)


@pytest.mark.parametrize('case, schemes', [('heat2', ('cn', 'sdirk3', 'esdirk34')), ('heat3', ('sdirk3', 'cn')),
                                           ('cd2', ('sdirk3', 'esdirk34'))])
def test_golden_parity(golden, case, schemes):
    g = golden('parabolic')
    pre = case + '_'
    S = _golden_system(g, case)
    try:
        assert S.method == ('bicgstab' if case == 'cd2' else 'cg')
        for scheme in schemes:
            times, sols = S.integrate(g[pre + 'u0'], float(g[pre + 'tau']), float(g[pre + 't_end']), scheme=SCHEMES[scheme], tol=1e-12)
            U = g[pre + scheme + '_u']
            assert len(sols) == len(U) and S.info['converged']
            assert np.allclose(times, g[pre + scheme + '_times'], rtol=0, atol=1e-15)
            assert _relmax(sols, U) < 1e-8, (case, scheme, _relmax(sols, U))
    finally:
        S.close()


@pytest.mark.parametrize('d, p, n', [(2, 3, 64), (3, 3, 16)])
def test_model_parity_at_larger_sizes(d, p, n):
    kvs = (bspline.make_knots(p, 0.0, 1.0, n),) * d
    if d == 2:
        geo = geometry.quarter_annulus()
        f, u0f, gf = (lambda x, y: 10 * (1 + x * y)), (lambda x, y: np.sin(x) + y), (lambda x, y: 1 + 0.1 * x)
    else:
        geo = geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.quarter_annulus())
        f, u0f, gf = (lambda x, y, z: 10 * (1 + x - z)), (lambda x, y, z: np.cos(x) + y * z), (lambda x, y, z: 1 + 0.1 * z)
    bcs = assemble.compute_dirichlet_bcs(kvs, geo, [('left', gf), ('right', gf)])
    rhs = assemble.inner_products(kvs, f, f_physical=True, geo=geo).ravel()
    M, K = assemble.mass(kvs, geo), assemble.stiffness(kvs, geo)
    S = solvers.ParabolicSystem(kvs, geo, rhs, bcs)
    try:
        tau = 1e-3
        times, sols = S.integrate(u0f, tau, 2.5 * tau, scheme='sdirk3', tol=1e-12)
        ref = P.restricted_dirk(solvers.dirk_tableau('sdirk3'), M, K, rhs, bcs[0], bcs[1], sols[0], tau, 3)
        assert _relmax(sols, ref) < 1e-8, _relmax(sols, ref)
        assert S.info['precond'] == 'kron'
    finally:
        S.close()


@pytest.mark.parametrize('scheme', ['crank_nicolson', 'sdirk3', 'esdirk34'])
def test_conservation_without_dirichlet_dofs(scheme):
    kvs = (bspline.make_knots(2, 0.0, 1.0, 8),) * 2
    geo = geometry.quarter_annulus()
    rhs = assemble.inner_products(kvs, lambda x, y: 1 + x * y, f_physical=True, geo=geo).ravel()
    M = assemble.mass(kvs, geo)
    u0 = np.random.default_rng(7).standard_normal(M.shape[0])
    S = solvers.ParabolicSystem(kvs, geo, rhs)
    try:
        assert S.box is not None and S.default_precond == 'kron'
        times, sols = S.integrate(u0, 0.01, 0.545, scheme=scheme, t0=0.5, tol=1e-12)
        m0 = np.sum(M @ u0)
        for t, x in zip(times, sols):
            want = m0 + (t - 0.5) * rhs.sum()
            assert abs(np.sum(M @ x) - want) <= 1e-10 * abs(want), (t, np.sum(M @ x), want)
    finally:
        S.close()


def test_steady_state_of_implicit_euler():
    kvs = (bspline.make_knots(3, 0.0, 1.0, 12),) * 2
    geo = geometry.quarter_annulus()
    bcs = assemble.compute_dirichlet_bcs(kvs, geo, [('left', lambda x, y: x), ('bottom', 1.0)])
    f = lambda x, y: np.cos(x) * y
    ref = solvers.PatchSystem(kvs, geo, f, bcs)
    try:
        u = ref.solve(tol=1e-13)
    finally:
        ref.close()
    S = solvers.ParabolicSystem(kvs, geo, f, bcs)
    try:
        times, sols = S.integrate(np.zeros(u.size), 1e8, 1.5e8, scheme='implicit_euler', tol=1e-13)
        assert np.abs(sols[-1] - u).max() / np.abs(u).max() < 1e-8
    finally:
        S.close()


def test_spmv_is_the_stage_matrix():
    kvs = (bspline.make_knots(3, 0.0, 1.0, 10),) * 2
    geo = geometry.quarter_annulus()
    bcs = assemble.compute_dirichlet_bcs(kvs, geo, [('top', 1.0)])
    M, K = assemble.mass(kvs, geo), assemble.stiffness(kvs, geo)
    S = solvers.ParabolicSystem(kvs, geo, 1.0, bcs)
    try:
        tau = 1e-3
        S.set_scheme('sdirk3', tau)
        gamma = solvers.check_tableau(solvers.dirk_tableau('sdirk3'))[1]
        x = np.random.default_rng(1).standard_normal(M.shape[0])
        free = np.ones(M.shape[0])
        free[bcs[0]] = 0
        want = free * ((M + tau * gamma * K) @ (free * x))
        y = S.spmv(x)
        assert np.abs(y - want).max() / np.abs(want).max() < 1e-13
    finally:
        S.close()


def test_saving_determinism_and_reassembly():
    kvs = (bspline.make_knots(2, 0.0, 1.0, 12),) * 2
    geo = geometry.quarter_annulus()
    bcs = assemble.compute_dirichlet_bcs(kvs, geo, [('left', 1.0)])
    S = solvers.ParabolicSystem(kvs, geo, lambda x, y: x * y, bcs, problem=CD2_FORM, diff_coeff=lambda x, y: 0.3 + 0.0 * x)
    try:
        u0 = np.random.default_rng(3).standard_normal(S.n)
        for scheme in ('sdirk3', 'esdirk34'):
            t1, s1 = S.integrate(u0, 0.01, 0.065, scheme=scheme, tol=1e-12)
            t2, s2 = S.integrate(u0, 0.01, 0.065, scheme=scheme, tol=1e-12, save_every=3)
            assert len(s1) == 8 and [round(t / 0.01) for t in t2] == [0, 3, 6, 7]
            for t, x in zip(t2, s2):
                assert np.array_equal(x, s1[round(t / 0.01)])
            _, s3 = S.integrate(u0, 0.01, 0.065, scheme=scheme, tol=1e-12)
            assert all(np.array_equal(a, b) for a, b in zip(s1, s3))
        S.patch.assemble('stiffness', to_host=False)
        S.patch.assemble('mass', to_host=False)
        _, s4 = S.integrate(u0, 0.01, 0.065, scheme='esdirk34', tol=1e-12)
        assert all(np.array_equal(a, b) for a, b in zip(s3, s4))
    finally:
        S.close()


def test_refusals_on_the_device_path():
    from pyiga_amd import form_assemblers
    kvs = (bspline.make_knots(2, 0.0, 1.0, 4),) * 2
    geo = geometry.unit_square()
    with pytest.raises(ValueError, match='boundary'):
        solvers.ParabolicSystem(kvs, geo, 0.0, problem='inner(grad(u), grad(v)) * ds')
    with pytest.raises(ValueError, match='FormAssembler'):                             # vector-valued forms
        solvers.ParabolicSystem(kvs, geo, 0.0, problem=form_assemblers.FormAssembler)
    with pytest.raises(ValueError, match='surface'):
        solvers.ParabolicSystem(kvs[:1], geo, 0.0, problem='u * v * dx')


# ---------------------------------------------------------------------------------------------
# k_vals_axpby and k_dirk_rhs past one grid and at full length (the constants and tableaux: tests/_mg_cases.py)
def _check_stage_matrix(kvs, geo, sides, tag):
    """S.spmv against free * ((M + tau gamma K) (free * x)) row by row in long double, M and K as the device assembled them.
    Returns the number of values of C."""
    bcs = assemble.compute_dirichlet_bcs(kvs, geo, [(s, 1.0) for s in sides])
    from pyiga_amd import assemblers
    patch = assemblers.DevicePatch(kvs, geo)                   # (the values in the patch's own layout: no entry is dropped)
    try:
        M = patch.csr('mass').copy()
        K = patch.csr('stiffness').copy()
    finally:
        patch.close()
    assert np.array_equal(M.indptr, K.indptr) and np.array_equal(M.indices, K.indices)
    S = solvers.ParabolicSystem(kvs, geo, 1.0, bcs)
    try:
        tau = 1e-3
        S.set_scheme('sdirk3', tau)
        gamma = solvers.check_tableau(solvers.dirk_tableau('sdirk3'))[1]
        n = M.shape[0]
        x = np.random.default_rng(1).standard_normal(n)
        free = np.ones(n)
        free[bcs[0]] = 0
        y = S.spmv(x)
        nv = int(S.patch.pattern()[1].size)        # the values k_vals_axpby combines: those of the patch's layout
        assert nv == M.nnz
    finally:
        S.close()
    ld = np.longdouble
    tg = ld(tau) * ld(gamma)
    Cl = scipy.sparse.csr_matrix((M.data.astype(ld) + tg * K.data.astype(ld), M.indices, M.indptr), shape=M.shape)
    Ca = scipy.sparse.csr_matrix((np.abs(M.data).astype(ld) + tg * np.abs(K.data).astype(ld), M.indices, M.indptr), shape=M.shape)
    xf = (free * x).astype(ld)
    want = free * (Cl @ xf)
    mag = Ca @ np.abs(xf)
    err = np.abs(y.astype(ld) - want)
    rel = float(err.max() / np.abs(want).max())
    rows = float((err[free > 0] / mag[free > 0]).max())
    print('C = M + tau gamma K', tag, 'values', nv, 'rel. difference %.2e' % rel, 'largest row error / row magnitude %.2e' % rows)
    assert rel < 1e-13, (tag, rel)
    assert rows < 1e-13, (tag, rows)                # a single wrong value of C changes its row by the order of its magnitude
    assert not y[bcs[0]].any()
    return nv


def test_stage_matrix_past_one_grid_of_k_vals_axpby():
    """3D p = 3, n = 30: 219^3 = 10 503 459 values, an odd number (the last value is the tail lane's) and more than the 16 ncu
    blocks of 256 lanes cover with AXPBY_U = 4 pairs each, so every u and a second trip of the outer loop run."""
    import subprocess
    import sys
    import _mg_cases as mc
    # (torch in a child process: this one has initialised the library's HIP runtime, beside which torch's finds no device)
    out = subprocess.run([sys.executable, '-c', 'import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)'],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    ncu = int(out.stdout.split()[-1])
    kvs = (bspline.make_knots(3, 0.0, 1.0, 30),) * 3
    geo = geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.quarter_annulus())
    nv = _check_stage_matrix(kvs, geo, [(0, 1)], '3d_p3_n30')
    one_trip = 16 * ncu * 256 * mc.AXPBY_U * 2
    print('k_vals_axpby: values', nv, 'one trip of the grid', one_trip, '(ncu %d)' % ncu)
    assert one_trip == 32768 * ncu and nv > one_trip and nv % 2 == 1


def test_stage_matrix_of_an_odd_tiny_patch():
    """2D p = 1, n = 2: 49 values; 24 pairs in a partial block and the tail lane do all the work."""
    kvs = (bspline.make_knots(1, 0.0, 1.0, 2),) * 2
    assert _check_stage_matrix(kvs, geometry.quarter_annulus(), [(0, 1)], '2d_p1_n2') == 49


def test_full_tableaux_past_one_grid_of_k_dirk_rhs():
    """2D p = 2, n = 512: 264 196 dofs, more than the NB_VEC blocks of k_dirk_rhs hold, and tableaux of IGX_DIRK_MAX_STAGES stages
    with a full lower triangle, with and without an explicit first stage: the last stage combines 7 vectors (M x, five F_j, f).
    Two steps of each against the host model (one factorization: the tableaux share their gamma)."""
    import _mg_cases as mc
    import _solver_cases as sc
    tabs = mc.dirk6_tableaux()
    kvs = (bspline.make_knots(2, 0.0, 1.0, 512),) * 2
    geo = geometry.quarter_annulus()
    f, gf = (lambda x, y: 10 * (1 + x * y)), (lambda x, y: 1 + 0.1 * x)
    bcs = assemble.compute_dirichlet_bcs(kvs, geo, [('left', gf), ('right', gf)])
    rhs = assemble.inner_products(kvs, f, f_physical=True, geo=geo).ravel()
    M, K = assemble.mass(kvs, geo), assemble.stiffness(kvs, geo)
    n = M.shape[0]
    assert n == 264196 > sc.vec_pass_rows()
    u0 = 1.0 + 0.1 * np.random.default_rng(9).standard_normal(n)     # rough: K u0 is large, every F_j weighs in the stage sums
    tau = 1e-5
    gamma = {solvers.check_tableau(A)[1] for A in tabs.values()}
    assert len(gamma) == 1
    solve = P.stage_solver(M, K, bcs[0], tau, gamma.pop())
    S = solvers.ParabolicSystem(kvs, geo, rhs, bcs)
    try:
        for name in ('sdirk6', 'esdirk6'):
            A = tabs[name]
            times, sols = S.integrate(u0, tau, 1.5 * tau, scheme=A, tol=1e-12)
            assert len(sols) == 3 and S.info['converged']
            implicit = int(np.count_nonzero(np.diag(A[:6])))
            assert S.info['stage_iterations'].shape == (2, implicit) and implicit == (5 if name == 'esdirk6' else 6)
            ref = P.restricted_dirk(A, M, K, rhs, bcs[0], bcs[1], sols[0], tau, 2, solve=solve)
            d = _relmax(sols, ref)
            step = _relmax([sols[2] - sols[0]], [ref[2] - ref[0]])
            print('DIRK', name, 'dofs', n, 'stage iterations', S.info['stage_iterations'].tolist(), 'rel. difference %.2e' % d,
                  'of the change over two steps %.2e' % step)
            assert d < 1e-8, (name, d)
    finally:
        S.close()

"""solvers.NavierStokesSystem and OseenSystem.update on the device against the goldens of the reference
(tests/golden/golden_ns*.npz, made by make_golden_ns.py): the replaced blocks through the solver's product, the Picard and
Newton iterates within the tolerance T measured on the host model (tests/_ns_model.py, tests/test_ns_cpu.py), and the pieces
around them.  The device runs solve as the goldens' conditions were checked: triangular Kronecker preconditioner, restart 128,
lin_tol = 1e-10, and they stop where the golden runs stop (rtol = 1e-10 of the first residual)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse

from pyiga_amd import _lib, assemblers, bspline, geometry, solvers

import _ns_model as nm
import _oseen_systems as osys
import _saddle_cases as sc
import _saddle_systems as ssys

pytestmark = pytest.mark.gpu

RUN = dict(atol=0.0, rtol=nm.RTOL, lin_tol=nm.LIN_TOL, restart=nm.RESTART, triangular=True)


def _system(golden, name, which='pinned'):
    kvs_u, kvs_p, geo, bcs, nv = ssys.problem(nm.BASE[name])
    if which == 'unpinned':
        bcs = (bcs[0][:-1], bcs[1][:-1])
    nu = float(golden('ns')[name + '_nu'])
    return solvers.NavierStokesSystem((kvs_u, kvs_p), geo, bcs, viscosity=nu, restart=nm.RESTART), nv, nu


def _gold_matrix(golden, name, which, tag):
    return sc.golden_csr(golden(nm.golden_wind_file(name, tag)), '%s_A_%s_%s' % (name, which, tag))


def _err(u, ref):
    return abs(u - ref).max() / abs(ref).max()


@pytest.mark.parametrize('newton', [False, True])
@pytest.mark.parametrize('name', nm.CASES)
def test_product_after_update_is_the_golden_matrices(name, newton, golden):
    """update(w=...) with the golden random wind, given by its dofs: the fused evaluation, the tables formed on the device, the
    blocks assembled and replaced.  R K R^T x for seeded random x against the golden matrices on the free rows, within 1e-12 of
    max(|K| |x|)."""
    g = golden('ns')
    S, nv, nu = _system(golden, name)
    try:
        w = np.asarray(golden(nm.golden_wind_file(name, 'rand'))[name + '_w_rand'])
        A = nu * sc.golden_csr(g, name + '_A_grad') + _gold_matrix(golden, name, 'conv', 'rand')
        if newton:
            A = A + _gold_matrix(golden, name, 'newt', 'rand')
        B = sc.golden_csr(g, name + '_A_div')
        K = scipy.sparse.bmat([[A, B.T], [B, None]], format='csr')
        free = np.ones(S.n, dtype=bool)
        free[S.bc_indices] = False
        for form in ('vector', 'coefficients'):
            S.update(newton=newton, w=w if form == 'vector' else S.split(np.concatenate((w, np.zeros(S.n - nv))))[0])
            for seed in (0, 1):
                x = np.random.default_rng(seed).standard_normal(S.n)
                xm = np.where(free, x, 0.0)
                ref = np.where(free, K @ xm, 0.0)
                y = S.spmv(x)
                bound = 1e-12 * (abs(K) @ abs(xm)).max()
                print('%s %s %s seed %d: %.2e (bound %.2e)' % (name, 'newton' if newton else 'picard', form, seed, abs(y - ref).max(), bound))
                assert abs(y - ref).max() <= bound
        if newton:                      # back to the Picard blocks: the Newton terms of the off-diagonal blocks are gone
            S.update(w=w)
            K = scipy.sparse.bmat([[A - _gold_matrix(golden, name, 'newt', 'rand'), B.T], [B, None]], format='csr')
            x = np.random.default_rng(2).standard_normal(S.n)
            xm = np.where(free, x, 0.0)
            assert abs(S.spmv(x) - np.where(free, K @ xm, 0.0)).max() <= 1e-12 * (abs(K) @ abs(xm)).max()
    finally:
        S.close()


@pytest.mark.parametrize('name', ['oseen2', 'oseen3'])
def test_update_with_a_callable_wind_gives_the_bits_of_a_fresh_system(name, golden):
    nu = float(golden('oseen')[name + '_nu'])
    wind = osys.wind2 if name == 'oseen2' else osys.wind3

    def other(*x):
        return tuple(1.0 + 0.5 * c for c in x)
    fresh, _ = osys.system(name, nu, restart=128)
    live, _ = osys.system(name, nu, restart=128, w=other)
    try:
        ref = fresh.solve(tol=1e-10)
        first = live.solve(tol=1e-10)
        assert not np.array_equal(first, ref)
        live.update(w=wind)
        again = live.solve(tol=1e-10)
        assert np.array_equal(again, ref) and live.info['iterations'] == fresh.info['iterations']
        grid = np.stack(np.broadcast_arrays(*other(*np.moveaxis(_gauss_points(live), -1, 0))), axis=-1)
        x = np.random.default_rng(4).standard_normal(live.n)
        live.update(w=other)
        y = live.spmv(x)
        live.update(w=grid)             # an array over the Gauss grid: the same wind sampled here, tables equal to rounding
        assert abs(live.spmv(x) - y).max() <= 1e-12 * abs(y).max()
    finally:
        fresh.close()
        live.close()


def _gauss_points(S):
    grid = tuple(S.patch.gauss(k)[0] for k in range(len(S.kvs)))
    return S._geo.grid_eval(grid)


@pytest.fixture(scope='module')
def device_runs(golden):
    """The four golden runs on the device, each once: (solution, iterates, info)."""
    cache = {}

    def get(name, method):
        if (name, method) not in cache:
            S, nv, nu = _system(golden, name)
            try:
                its = []
                u = S.solve(method=method, callback=lambda k, x: its.append(x), **RUN)
                cache[(name, method)] = (u, its, S.info)
            finally:
                S.close()
        return cache[(name, method)]
    return get


@pytest.mark.parametrize('method', nm.METHODS)
@pytest.mark.parametrize('name', nm.CASES)
def test_golden_iterates(name, method, golden, device_runs):
    g = golden('ns')
    gold, norms = np.asarray(g['%s_%s_iterates' % (name, method)]), np.asarray(g['%s_%s_norms' % (name, method)])
    u, its, info = device_runs(name, method)
    steps = nm.GOLDEN_STEPS[(name, method)]
    print('%s %s: %d steps, inner %s, residual norms %s' % (name, method, info['iterations'], info['inner_iterations'],
                                                           ' '.join('%.2e' % r for r in info['residual_norms'])))
    assert info['converged'] and info['iterations'] == steps == len(its) == gold.shape[0] - 1
    errs = [_err(its[k - 1], gold[k]) for k in range(1, steps + 1)]
    print('    iterates within %.2e (T = %.2e)' % (max(errs), nm.T))
    assert max(errs) <= nm.T and np.array_equal(u, its[-1])
    # info: a norm before every step and after the last, one solve per step, every solve one cycle, the blocks of _ns_model
    assert len(info['residual_norms']) == steps + 1 and len(info['inner_iterations']) == steps == len(info['restarts'])
    assert info['residual_norms'][-1] < info['target'] == nm.RTOL * info['residual_norms'][0]
    assert all(r >= info['target'] for r in info['residual_norms'][:-1])
    assert all(0 < n <= nm.RESTART for n in info['inner_iterations']) and not any(info['restarts'])
    assert info['blocks_assembled'] == nm.blocks_assembled(len(ssys.problem(nm.BASE[name])[0]), method, steps)
    assert info['method'] == method and info['stokes']['converged'] and info['triangular'] and info['restart'] == nm.RESTART
    # (the later norms are those of iterates that differ from the golden ones by the linear solves' stops: only the first compares)
    assert abs(info['residual_norms'][0] - norms[0]) <= 1e-6 * norms[0]


@pytest.mark.parametrize('name', nm.CASES)
def test_stokes_start_is_the_first_golden_iterate(name, golden):
    S, nv, nu = _system(golden, name)
    try:
        with pytest.raises(solvers.NoConvergenceError) as e:
            S.solve(method='picard', maxiter=0, **RUN)
        assert _err(e.value.last_iterate, np.asarray(golden('ns')[name + '_picard_iterates'])[0]) <= nm.T
        assert S.info['iterations'] == 0 and S.info['blocks_assembled'] == S.ncomp
    finally:
        S.close()


@pytest.mark.parametrize('method', nm.METHODS)
def test_maxiter_one_raises_with_the_first_iterate(method, golden):
    gold = np.asarray(golden('ns')['ns2_%s_iterates' % method])
    S, nv, nu = _system(golden, 'ns2')
    try:
        with pytest.raises(solvers.NoConvergenceError) as e:
            S.solve(method=method, maxiter=1, **RUN)
        assert e.value.method == method and e.value.num_iter == 1
        assert _err(e.value.last_iterate, gold[1]) <= nm.T
        assert S.info['iterations'] == 1 and not S.info['converged']
    finally:
        S.close()


@pytest.mark.parametrize('name', nm.CASES)
def test_repeated_solves_are_bit_identical(name, golden, device_runs):
    S, nv, nu = _system(golden, name)
    try:
        a = S.solve(method='newton', **RUN)
        b = S.solve(method='newton', **RUN)            # (the solver holds the Newton blocks of the last step: Stokes is restored)
        assert np.array_equal(a, b) and np.array_equal(a, device_runs(name, 'newton')[0])
        c = S.solve(method='picard', x0=a, **dict(RUN, atol=1e-6))      # from the solution: converged before the first step
        assert S.info['iterations'] == 0 and np.array_equal(c, a)
    finally:
        S.close()


@pytest.mark.parametrize('name', nm.CASES)
def test_picard_steps_then_newton(name, golden):
    g = golden('ns')
    gold_p, gold_n = np.asarray(g[name + '_picard_iterates']), np.asarray(g[name + '_newton_iterates'])
    S, nv, nu = _system(golden, name)
    try:
        its = []
        u = S.solve(method='newton', picard_steps=2, callback=lambda k, x: its.append(x), **RUN)
        steps = S.info['iterations']
        print('%s: %d steps (2 Picard, then Newton), within %.2e of the golden solution' % (name, steps, _err(u, gold_n[-1])))
        assert S.info['converged'] and 2 < steps <= 2 + nm.GOLDEN_STEPS[(name, 'newton')]
        assert _err(its[0], gold_p[1]) <= nm.T and _err(its[1], gold_p[2]) <= nm.T
        assert _err(u, gold_n[-1]) <= nm.T
        assert S.info['blocks_assembled'] == nm.blocks_assembled(S.ncomp, 'newton', steps, 2)
    finally:
        S.close()


def test_unpinned_pressure_is_projected(golden):
    """The enclosed flow without a pinned pressure dof: a singular matrix, solved with the projection of DESIGN.md section 31.
    It runs as the golden runs do, to 1e-10 of the first residual, with the reference's step count.

    On the quarter annulus the constant pressure is only nearly in the kernel of the discrete matrix: B^T 1 on the free velocity
    rows is the quadrature error of int div v, 9.8e-10.  The correction solves therefore run on Q K Q and Q P, Q taking the
    pressure mean off (igx_solver_saddle_correct_d); with the operators left as they are GMRES resolves the near-kernel --
    corrections with pressures of 3e3 to 6e3, a velocity 2e-4 from the pinned one and residuals that stall at 5e-13 -- on the
    device and in the host model alike.  The model with the projected operators takes 3 Newton steps (residuals 5.7e-3, 6.7e-6,
    1.8e-12, 7.9e-17) and ends 8.4e-10 (velocity) and 3.7e-9 (pressure) from the pinned golden solution."""
    gold = np.asarray(golden('ns')['ns2_newton_iterates'])[-1]
    S, nv, nu = _system(golden, 'ns2', 'unpinned')
    try:
        assert S.enclosed
        u = S.solve(method='newton', pressure='auto', **RUN)
        assert S.info['iterations'] == nm.GOLDEN_STEPS[('ns2', 'newton')] and not any(S.info['restarts'])
        ev = abs(u[:nv] - gold[:nv]).max() / abs(gold).max()
        ep = abs(u[nv:] - (gold[nv:] - gold[nv])).max() / abs(gold).max()
        print('ns2 unpinned: velocity %.2e, pressure %.2e (T = %.2e), %d steps' % (ev, ep, nm.T, S.info['iterations']))
        assert S.info['converged'] and u[nv] == 0.0
        assert ev <= nm.T and ep <= nm.T
    finally:
        S.close()


def test_jacobi_takes_the_diagonal_of_a_replaced_block(golden):
    g = golden('ns')
    S, nv, nu = _system(golden, 'ns2')
    try:
        w = np.asarray(g['ns2_w_rand'])
        free = np.ones(S.n, dtype=bool)
        free[S.bc_indices] = False
        r = np.where(free, np.random.default_rng(3).standard_normal(S.n), 0.0)
        before = S.apply_precond(r, 'jacobi', triangular=False)
        S.update(w=w)
        after = S.apply_precond(r, triangular=False)
        A = nu * sc.golden_csr(g, 'ns2_A_grad') + _gold_matrix(golden, 'ns2', 'conv', 'rand')
        ref = np.where(free[:nv], r[:nv] / A.diagonal(), 0.0)
        assert abs(after[:nv] - ref).max() <= 1e-12 * abs(ref).max()
        assert abs(before[:nv] - ref).max() > 1e-3 * abs(ref).max()          # (the old diagonal is another one)
        assert np.array_equal(after[nv:], before[nv:])
    finally:
        S.close()


def test_replace_block_refusals(golden):
    lib = _lib.load()
    P = solvers.PatchSystem((bspline.make_knots(2, 0.0, 1.0, 4),) * 2, geometry.unit_square(), np.ones(36))
    try:
        assert lib.igx_solver_replace_block(P.handle, 0, 0) == _lib.IGX_ERR_ARG             # not a block solver
        assert lib.igx_solver_hide_block(P.handle, 0, 1, 1) == _lib.IGX_ERR_UNSUPPORTED
    finally:
        P.close()
    S, nv, nu = _system(golden, 'ns2')
    try:
        assert lib.igx_solver_replace_block(None, 0, 0) == _lib.IGX_ERR_ARG
        assert lib.igx_d_csr_data(S.patch.handle) is None
        assert lib.igx_solver_replace_block(S.handle, 0, 0) == _lib.IGX_ERR_ARG             # the patch holds no IGX_FORM values
        assert 'IGX_FORM' in _lib.last_error()
        S.patch.assemble('form', to_host=False)
        for p, q in ((2, 0), (0, 2), (-1, 0)):
            assert lib.igx_solver_replace_block(S.handle, p, q) == _lib.IGX_ERR_ARG         # out of range
        assert lib.igx_solver_hide_block(S.handle, 0, 0, 1) == _lib.IGX_ERR_ARG and lib.igx_solver_hide_block(S.handle, 0, 2, 1) == _lib.IGX_ERR_ARG
        assert lib.igx_solver_take_block(S.handle, 0, 0) == _lib.IGX_ERR_ARG                # taken already: the refusal stays
        assert lib.igx_solver_replace_block(S.handle, 0, 1) == _lib.IGX_OK                  # a block absent so far
        assert lib.igx_d_csr_data(S.patch.handle) is None                                   # (nothing to hand back)
        S.patch.assemble('form', to_host=False)
        assert lib.igx_solver_replace_block(S.handle, 0, 1) == _lib.IGX_OK
        assert lib.igx_d_csr_data(S.patch.handle) is not None                               # the old buffer is the patch's next one
        # the correction calls need GMRES and a saddle-point solver
        d_x = S.patch._dev_buffer('_d_test', 8 * S.n)
        nrm = C.c_double()
        M, _ = ssys.system('stokes', 'pinned')
        try:
            assert lib.igx_solver_saddle_residual_d(M.handle, None, d_x, C.byref(nrm)) == _lib.IGX_ERR_UNSUPPORTED      # MINRES
            assert lib.igx_solver_saddle_correct_d(M.handle, d_x, 1e-8, 10, 1, 0, None) == _lib.IGX_ERR_UNSUPPORTED
        finally:
            M.close()
        assert lib.igx_solver_saddle_residual_d(S.handle, None, d_x, C.byref(nrm)) == _lib.IGX_ERR_UNSUPPORTED      # GMRES not selected yet
        S._select(None, False, nm.RESTART)
        assert lib.igx_solver_saddle_residual_d(S.handle, None, None, C.byref(nrm)) == _lib.IGX_ERR_ARG
    finally:
        S.close()


def test_set_form_sum_is_the_host_sum(golden):
    """igx_patch_set_form_sum_d against igx_patch_set_form of the sum formed on the host, through the assembled values: equal
    bits, entries present on one side only included; a failed call leaves the form in place."""
    kvs = (bspline.make_knots(2, 0.0, 1.0, 5), bspline.make_knots(3, 0.0, 1.0, 4))
    patch = assemblers.DevicePatch(kvs, geometry.quarter_annulus())
    try:
        G = tuple(int(patch.info.ngauss[k]) for k in range(2))
        rng = np.random.default_rng(9)
        a = {(1, 1): rng.uniform(1.0, 2.0, G), (2, 2): rng.uniform(1.0, 2.0, G), (0, 0): rng.uniform(0.0, 1.0, G)}
        b = {(0, 1): rng.standard_normal(G), (0, 2): rng.standard_normal(G), (0, 0): rng.standard_normal(G)}
        scale = 0.3

        def table(d):
            t = [[None] * 4 for _ in range(4)]
            for (r, s), v in d.items():
                t[r][s] = v
            return t
        host ={k: (scale * a[k] + b[k]) if (k in a and k in b) else (scale * a[k] if k in a else b[k]) for k in set(a) | set(b)}
        patch.set_form(table(host))
        ref = patch.assemble('form').copy()

        def resident(d, buf):
            keys = sorted(d)
            ptrs = patch.upload_fields([d[k] for k in keys], buf=buf)
            return table(dict(zip(keys, ptrs)))
        ta, tb = resident(a, '_d_ta'), resident(b, '_d_tb')
        patch.set_form_sum_resident(ta, scale, tb)
        assert np.array_equal(patch.assemble('form'), ref)
        with pytest.raises(_lib.IgxError):
            patch.set_form_sum_resident(table({}), scale, table({}))            # all absent: refused, the form stays
        assert np.array_equal(patch.assemble('form'), ref)
        patch.set_form_sum_resident(ta, scale, None)
        patch.set_form(table({k: scale * v for k, v in a.items()}))
        only_a = patch.assemble('form').copy()
        patch.set_form_sum_resident(ta, scale, None)
        assert np.array_equal(patch.assemble('form'), only_a)
    finally:
        patch.close()


def test_existing_solvers_repeat_their_bits(golden):
    """MINRES and GMRES on existing golden systems after the library gained the new calls: two solves, equal bits, and the
    golden solutions within the bounds their own tests hold them to."""
    M, nv = ssys.system('stokes', 'pinned')
    try:
        a, b = M.solve(tol=1e-10), M.solve(tol=1e-10)
        assert np.array_equal(a, b) and M.info['converged']
    finally:
        M.close()
    nu = float(golden('oseen')['oseen2_nu'])
    S, nv = osys.system('oseen2', nu, restart=128)
    try:
        a, b = S.solve(tol=1e-10), S.solve(tol=1e-10)
        assert np.array_equal(a, b) and S.info['converged']
        assert _err(a, np.asarray(golden('oseen')['oseen2_u'])) <= 10 * float(golden('oseen')['oseen2_amp']) * 1e-10
    finally:
        S.close()

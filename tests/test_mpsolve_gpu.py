"""Multipatch Dirichlet problems solved on the device (solvers.MultipatchSystem, igx_solver_create_multipatch): solutions against
scipy's spsolve of the restricted system MP.assemble_system gives, the CSR SpMV against R A R^T, the Schwarz and Jacobi
preconditioners against numpy, iteration counts against the numpy model, determinism, and the refusals."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.linalg

from pyiga_amd import _lib, assemble, bspline, geometry, solvers

import _mpsolve_model as M

pytestmark = pytest.mark.gpu

STIFF = 'inner(grad(u),grad(v))*dx'


def f2(x, y):
    return np.exp(-5 * ((x - 0.3) ** 2 + (y - 1) ** 2))


def g2(x, y):
    return 1e-1 * np.sin(8 * x)


def f3(x, y, z):
    return 1.0 + x * y - z


def g3(x, y, z):
    return x + 0.5 * y * z


def _case(name):
    """(MP, rhs functional, f, bcs) of a test domain."""
    if name == 'notebook':
        MP = M.notebook(p=3, n=15)
        bcs = MP.compute_dirichlet_bcs([(p, bd, g2) for p, bd in M.NOTEBOOK_DIRICHLET])
        return MP, f2, bcs
    if name == 'lshape':
        MP = M.lshape(p=2, n=8)
        bcs = MP.compute_dirichlet_bcs([(0, 'left', g2), (0, 'bottom', g2), (2, 'top', g2)])
        return MP, f2, bcs
    MP = M.three_cubes(p=2, n=4)                      # the middle cube has no fixed face: a floating patch
    bcs = MP.compute_dirichlet_bcs([(0, (0, 0), g3), (2, (2, 1), g3)])
    return MP, f3, bcs


def _reference(MP, f, bcs):
    A, b = MP.assemble_system(STIFF, 'f*v*dx', f=f)
    RS = assemble.RestrictedLinearSystem(A, b, bcs)
    return A, b, RS, RS.complete(scipy.sparse.linalg.spsolve(RS.A.tocsc(), RS.b))


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@pytest.mark.parametrize('name', ['notebook', 'lshape', 'cubes3d'])
def test_solutions_match_scipy(name):
    MP, f, bcs = _case(name)
    A, b, RS, u_ref = _reference(MP, f, bcs)
    S = solvers.MultipatchSystem(MP, STIFF, 'f*v*dx', bcs=bcs, f=f)
    try:
        for precond in (None, 'jacobi', 'schwarz'):
            u = S.solve(tol=1e-12, maxiter=5000, precond=precond)
            assert S.info['converged'], (name, precond, S.info)
            assert _rel(u, u_ref) <= 1e-8, (name, precond, _rel(u, u_ref))
            assert np.array_equal(u[bcs[0]], bcs[1])
        # SpMV: R A R^T x
        free = np.ones(MP.numdofs, dtype=bool)
        free[bcs[0]] = False
        x = np.random.default_rng(3).standard_normal(MP.numdofs)
        y = S.spmv(x)
        xf = np.where(free, x, 0.0)
        ref = np.where(free, A @ xf, 0.0)
        assert abs(y - ref).max() <= 1e-13 * abs(ref).max()
        # preconditioners: Jacobi against 1 / diag, Schwarz against the numpy model built from the same factors
        r = np.random.default_rng(4).standard_normal(MP.numdofs)
        zj = S.apply_precond(r, 'jacobi')
        ref = np.where(free, r / A.diagonal(), 0.0)
        assert abs(zj - ref).max() <= 1e-14 * abs(ref).max()
        zs = S.apply_precond(r, 'schwarz')
        boxes, U, lam, mode = S.schwarz_setup()
        shapes, maps = M.shapes_maps(MP)
        ref = M.SchwarzModel(MP.numdofs, shapes, maps, bcs[0], boxes, U, lam, mode).apply(r)
        assert abs(zs - ref).max() <= 1e-12 * abs(ref).max()
        assert not zs[~free].any()
    finally:
        S.close()


def test_schwarz_halves_jacobi_on_notebook_n64_and_matches_model():
    MP = M.notebook(p=3, n=64)
    bcs = MP.compute_dirichlet_bcs([(p, bd, g2) for p, bd in M.NOTEBOOK_DIRICHLET])
    A, b = MP.assemble_system(STIFF, 'f*v*dx', f=f2)
    RS = assemble.RestrictedLinearSystem(A, b, bcs)
    S = solvers.MultipatchSystem(MP, STIFF, 'f*v*dx', bcs=bcs, f=f2)
    try:
        S.solve(tol=1e-8, precond='jacobi')
        it_j = S.info['iterations']
        S.solve(tol=1e-8, precond='schwarz')
        it_s = S.info['iterations']
        assert 2 * it_s <= it_j, (it_s, it_j)
        # the numpy model with scipy's CG on the same restricted system
        boxes, U, lam, mode = S.schwarz_setup()
        shapes, maps = M.shapes_maps(MP)
        model = M.SchwarzModel(MP.numdofs, shapes, maps, bcs[0], boxes, U, lam, mode)
        free = model.free

        def schwarz(r):
            z = np.zeros(MP.numdofs)
            z[free] = r
            return model.apply(z)[free]
        d = RS.A.diagonal()
        mj, _, _ = M.cg_iterations(RS.A.tocsr(), RS.b, lambda r: r / d, 1e-8)
        ms, _, _ = M.cg_iterations(RS.A.tocsr(), RS.b, schwarz, 1e-8)
        assert abs(it_j - mj) <= 2 and abs(it_s - ms) <= 2, (it_j, mj, it_s, ms)
    finally:
        S.close()


def test_two_solves_are_bit_identical_and_rhs_stays_on_the_device():
    MP, f, bcs = _case('notebook')
    A, b = MP.assemble_system(STIFF, 'f*v*dx', f=f)
    S = solvers.MultipatchSystem(MP, STIFF, 'f*v*dx', bcs=bcs, f=f)
    try:
        for precond in ('schwarz', 'jacobi'):
            u1 = S.solve(tol=1e-10, precond=precond)
            u2 = S.solve(tol=1e-10, precond=precond)
            assert np.array_equal(u1, u2), precond
            u3 = S.solve(tol=1e-10, precond=precond, b=b)           # the downloaded vector passed explicitly
            assert np.array_equal(u1, u3), precond
    finally:
        S.close()


def test_stale_sums_and_closed_multipatch_refused():
    MP, f, bcs = _case('lshape')
    S = solvers.MultipatchSystem(MP, STIFF, 'f*v*dx', bcs=bcs, f=f)
    S.solve(precond='schwarz')
    MP.assemble_system('u*v*dx', 'f*v*dx', f=f)                     # restarts the sums
    with pytest.raises(_lib.IgxError) as e:
        S.solve(precond='schwarz')
    assert e.value.code == _lib.IGX_ERR_ARG and 'restarted' in str(e.value)
    with pytest.raises(_lib.IgxError):
        S.spmv(np.ones(MP.numdofs))
    S2 = solvers.MultipatchSystem(MP, STIFF, 'f*v*dx', bcs=bcs, f=f)
    S2.solve(precond='jacobi')
    MP.close()
    assert S2.handle is None
    with pytest.raises(_lib.IgxError):
        S2.solve(precond='jacobi')
    with pytest.raises(_lib.IgxError):
        S2.apply_precond(np.ones(MP.numdofs))
    # a new system after the close builds the device structures again
    S3 = solvers.MultipatchSystem(MP, STIFF, 'f*v*dx', bcs=bcs, f=f)
    assert S3.solve(precond='schwarz').shape == (MP.numdofs,) and S3.info['converged']
    S3.close()


def test_refusals():
    MP, f, bcs = _case('lshape')
    with pytest.raises(ValueError):
        solvers.MultipatchSystem(MP, '(inner(grad(u),grad(v)) + u*Dx(v,0))*dx', 'f*v*dx', bcs=bcs, f=f)
    S = solvers.MultipatchSystem(MP, STIFF, 'f*v*dx', bcs=bcs, f=f)
    with pytest.raises(ValueError):
        S.solve(precond='kron')
    lib = _lib.load()
    assert lib.igx_solver_set_precond(S.handle, _lib.IGX_PRECOND_KRON, None, None, None, None, 0) == _lib.IGX_ERR_UNSUPPORTED
    # z = P r into the buffer of r is refused (z is cleared before r is read)
    from pyiga_amd.operators import DeviceArray
    S.set_precond('schwarz')
    d = DeviceArray.from_host(S._ctx, np.ones(MP.numdofs))
    assert lib.igx_solver_precond_d(S.handle, d.ptr, d.ptr) == _lib.IGX_ERR_ARG
    assert S._ctx is MP._ctx
    S.close()
    kvs = 2 * (bspline.make_knots(2, 0.0, 1.0, 6),)
    P = solvers.PatchSystem(kvs, geometry.unit_square(), np.ones(64), None, kind='mass')
    try:
        with pytest.raises(ValueError):
            P.solve(precond='schwarz')
        lo, hi = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(8, 8, 0)
        assert lib.igx_solver_set_schwarz(P.handle, lo, hi, None, None, _lib.IGX_KRON_PRODUCT) == _lib.IGX_ERR_UNSUPPORTED
        assert lib.igx_solver_set_precond(P.handle, _lib.IGX_PRECOND_SCHWARZ, None, None, None, None, 0) == _lib.IGX_ERR_UNSUPPORTED
    finally:
        P.close()


def test_non_injective_join_schwarz_unsupported_jacobi_solves():
    kvs = 2 * (bspline.make_knots(2, 0.0, 1.0, 4),)
    MP = assemble.Multipatch([(kvs, geometry.unit_square()), (kvs, geometry.unit_square().translate((1, 0)))])
    MP.join_dofs(0, [5], 1, [12])
    MP.join_dofs(1, [12], 0, [23])
    MP.finalize()
    assert not MP.injective
    bcs = MP.compute_dirichlet_bcs([(0, 'left', g2), (1, 'right', g2)])
    A, b, RS, u_ref = _reference(MP, f2, bcs)
    S = solvers.MultipatchSystem(MP, STIFF, 'f*v*dx', bcs=bcs, f=f2)
    try:
        with pytest.raises(_lib.IgxError) as e:
            S.solve(precond='schwarz')
        assert e.value.code == _lib.IGX_ERR_UNSUPPORTED
        u = S.solve(tol=1e-12, precond='jacobi')
        assert S.info['converged'] and _rel(u, u_ref) <= 1e-8
    finally:
        S.close()

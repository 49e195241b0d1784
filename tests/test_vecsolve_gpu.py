"""Vector-valued Dirichlet problems solved on the device (solvers.VectorFormSystem, igx_solver_create_block; one MI355X).

- Block SpMV (k_block_spmv): every case of tests/_vecsolve_model.py (every group width past one grid of scalar rows, 2 and 3
  components, absent blocks included) row by row against a long-double product of R A R^T, A the blocked matrix of
  ``assemble(..., layout='blocked')``; fixed rows exactly 0.  Jacobi bit for bit against the diagonals of the diagonal blocks.
- The block-Kronecker preconditioner against the numpy model.
- Solves against RestrictedLinearSystem + spsolve: 2D elasticity (CG + kron), 3D p = 2 elasticity on the cylinder (CG), a
  non-symmetric 2D form (BiCGStab, Jacobi and kron): true residual, Dirichlet values, iteration counts against the models,
  bit-identical repeats, check_every.
- Refusals: a missing diagonal block, a block taken twice, CG on a non-symmetric solver, a closed system.
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.linalg

from pyiga_amd import _lib, assemble, bspline, geometry, solvers
from pyiga_amd.form_assemblers import _full_table

import _bicgstab_model as BM
import _vecsolve_model as V

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
MU_LAM = dict(mu=1.0, lam=2.0)


def _cyl():
    return geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.quarter_annulus())


def _geo(dim):
    return geometry.quarter_annulus() if dim == 2 else _cyl()


def _rng(tag):
    return np.random.default_rng(zlib.crc32(tag.encode()))


def _spread(rng, n, binades=20):
    return rng.choice([-1.0, 1.0], n) * np.exp2(rng.uniform(-binades, binades, n))


def _ld(A):
    A = A.tocsr()
    return scipy.sparse.csr_matrix((A.data.astype(np.longdouble), A.indices, A.indptr), shape=A.shape)


def _blocked(form, kvs, geo, nc, **inputs):
    return assemble.assemble(form, kvs, bfuns=V.bfuns(nc), geo=geo, layout='blocked', **inputs).tocsr()


# ---------------------------------------------------------------------------------------------
# block SpMV and Jacobi: every width past one grid of scalar rows, 2 and 3 components
@pytest.mark.parametrize('case', V.VEC_CASES, ids=[c.id for c in V.VEC_CASES])
def test_block_spmv_and_jacobi(case):
    kvs = case.kvs()
    nc, d = case.nc, case.patch.dim
    N = int(np.prod([kv.numdofs for kv in kvs]))
    n = nc * N
    rng = _rng(case.id)
    # component 0 clamped on one side, the last one on another, and random dofs of every component
    fixed = np.unique(np.concatenate([V.side_dofs(kvs, [(0, 0)], 1), V.side_dofs(kvs, [(d - 1, 1)], 1) + (nc - 1) * N,
                                      rng.choice(n, size=max(1, n // 50), replace=False)]))
    form = V.COUPLED[nc]
    S = solvers.VectorFormSystem(form, kvs, 0.0, (fixed, np.zeros(fixed.size)), bfuns=V.bfuns(nc), geo=_geo(d))
    try:
        assert not S.symmetric and S.method == 'bicgstab'
        assert not all(all(r) for r in S.present) and all(S.present[c][c] for c in range(nc))
        A = _blocked(form, kvs, _geo(d), nc)
        assert A.shape == (n, n)
        free = np.ones(n, dtype=bool)
        free[fixed] = False
        x = _spread(rng, n)
        y = S.spmv(x)
        xf = np.where(free, x, 0.0)
        Al = _ld(A)
        ref = np.where(free, Al @ xf.astype(np.longdouble), 0.0)
        mag = abs(Al) @ np.abs(xf).astype(np.longdouble)
        bound = 2 * np.diff(A.indptr) * U53 * mag
        err = np.abs(y.astype(np.longdouble) - ref)
        bad = np.flatnonzero(free & (err > bound))
        assert bad.size == 0, (case.id, bad.size, bad[:8])
        assert np.all(y[~free] == 0.0), case.id
        assert np.all(mag[free] > 0)
        x2 = x.copy()
        x2[fixed] = _spread(rng, fixed.size) * 1e3
        assert np.array_equal(S.spmv(x2), y), case.id              # the fixed entries of x are not read
        # Jacobi: the diagonals of the diagonal blocks, bit for bit
        r = _spread(_rng(case.id + 'r'), n, 8)
        z = S.apply_precond(r, 'jacobi')
        assert np.array_equal(z, np.where(free, (1.0 / A.diagonal()) * r, 0.0)), case.id
    finally:
        S.close()


# ---------------------------------------------------------------------------------------------
def _elasticity_2d(n=24, p=3, **kw):
    kvs = (bspline.make_knots(p, 0.0, 1.0, n),) * 2
    fixed = V.side_dofs(kvs, [(1, 0)], 2)                            # clamped on one side
    N = kvs[0].numdofs * kvs[1].numdofs
    vals = np.where(fixed < N, 0.01, -0.02)
    rhs = np.concatenate([np.full(N, 1e-3), np.full(N, -2e-3)])
    S = solvers.VectorFormSystem(V.ELASTICITY, kvs, rhs, (fixed, vals), bfuns=V.bfuns(2), geo=_geo(2), **MU_LAM, **kw)
    return S, kvs, fixed, vals, rhs


def _reference(S, form, kvs, geo, fixed, vals, rhs, **inputs):
    A = _blocked(form, kvs, geo, S.ncomp, **inputs)
    LS = assemble.RestrictedLinearSystem(A, rhs, (fixed, vals))
    return A, LS, LS.complete(scipy.sparse.linalg.spsolve(LS.A.tocsc(), LS.b))


def _check_solution(S, u, A, LS, uref, fixed, vals, rhs, tol):
    assert np.array_equal(u[fixed], vals)                          # the Dirichlet values exact
    free = np.setdiff1d(np.arange(S.n), fixed)
    res = (rhs - A @ u)[free]
    r0 = LS.b
    assert np.linalg.norm(res) <= 2 * tol * np.linalg.norm(r0), (np.linalg.norm(res), np.linalg.norm(r0))
    assert np.linalg.norm(u - uref) <= 1e-5 * np.linalg.norm(uref)


def test_elasticity_2d_cg_kron_against_spsolve_and_model():
    S, kvs, fixed, vals, rhs = _elasticity_2d()
    try:
        assert S.symmetric and S.method == 'cg' and S.default_precond == 'kron'
        u = S.solve(tol=1e-10, maxiter=2000)
        assert S.info['converged'] and S.info['precond'] == 'kron' and S.info['method'] == 'cg'
        A, LS, uref = _reference(S, V.ELASTICITY, kvs, _geo(2), fixed, vals, rhs, **MU_LAM)
        _check_solution(S, u, A, LS, uref, fixed, vals, rhs, 1e-10)
        # the preconditioner against the model, and the model's iteration count
        P = V.BlockKronModel(S.ndofs, S.kron_factors())
        r = _spread(_rng('kron2d'), S.n, 4)
        z = S.apply_precond(r, 'kron')
        free = np.ones(S.n, dtype=bool)
        free[fixed] = False
        zm = P.apply(np.where(free, r, 0.0))
        assert np.max(np.abs(z - zm)) <= 1e-11 * np.max(np.abs(zm))
        assert np.all(z[~free] == 0.0)
        fr = np.flatnonzero(free)

        def Mfree(v):
            full = np.zeros(S.n)
            full[fr] = v
            return P.apply(full)[fr]
        _, it, conv = V.pcg(LS.A, LS.b, Mfree, tol=1e-10, maxiter=2000)
        assert conv and abs(S.info['iterations'] - it) <= 2, (S.info['iterations'], it)
        # two solves bit-identical.  CG has no freeze on stop: with check_every = 10 it runs on to the next
        # multiple of 10, so u is another converged iterate (BiCGStab freezes: bit-identical, test_nonsymmetric_2d_...)
        it1 = S.info['iterations']
        assert np.array_equal(S.solve(tol=1e-10, maxiter=2000), u)
        u10 = S.solve(tol=1e-10, maxiter=2000, check_every=10)
        assert S.info['converged'] and it1 <= S.info['iterations'] < it1 + 10 and S.info['iterations'] % 10 == 0
        assert np.linalg.norm(u10 - uref) <= 1e-5 * np.linalg.norm(uref)
        # re-assembling the patch after the takes leaves the solver's blocks as they are
        S.patch.set_form(_full_table(S.assembler._table[0][0], 2))
        S.patch.assemble('form', to_host=False)
        S.patch.assemble('mass', to_host=False)
        assert np.array_equal(S.solve(tol=1e-10, maxiter=2000), u)
    finally:
        S.close()


def test_elasticity_3d_p2_cylinder_cg_against_spsolve():
    kvs = (bspline.make_knots(2, 0.0, 1.0, 6),) * 3
    N = int(np.prod([kv.numdofs for kv in kvs]))
    fixed = V.side_dofs(kvs, [(0, 0)], 3)
    vals = np.zeros(fixed.size)
    rhs = np.concatenate([np.full(N, 1e-3), np.zeros(N), np.full(N, -1e-3)])
    S = solvers.VectorFormSystem(V.ELASTICITY, kvs, rhs, (fixed, vals), bfuns=V.bfuns(3), geo=_cyl(), **MU_LAM)
    try:
        assert S.symmetric and S.method == 'cg' and S.ncomp == 3
        u = S.solve(tol=1e-10, maxiter=3000)
        assert S.info['converged'] and S.info['precond'] == 'kron'
        A, LS, uref = _reference(S, V.ELASTICITY, kvs, _cyl(), fixed, vals, rhs, **MU_LAM)
        _check_solution(S, u, A, LS, uref, fixed, vals, rhs, 1e-10)
        uj = S.solve(tol=1e-10, maxiter=5000, precond='jacobi')
        assert S.info['converged'] and np.linalg.norm(uj - uref) <= 1e-5 * np.linalg.norm(uref)
    finally:
        S.close()


@pytest.mark.parametrize('precond', ['jacobi', 'kron'])
def test_nonsymmetric_2d_bicgstab_against_spsolve_and_model(precond):
    kvs = (bspline.make_knots(2, 0.0, 1.0, 20),) * 2
    N = int(np.prod([kv.numdofs for kv in kvs]))
    fixed = V.side_dofs(kvs, [(0, 0), (1, 1)], 2)
    vals = np.where(fixed < N, 0.5, -0.25)
    rng = _rng('nonsym')
    rhs = rng.standard_normal(2 * N) * 1e-2
    S = solvers.VectorFormSystem(V.NONSYM, kvs, rhs, (fixed, vals), bfuns=V.bfuns(2), geo=_geo(2))
    try:
        assert not S.symmetric and S.method == 'bicgstab' and S.default_precond == 'kron'
        u = S.solve(tol=1e-10, maxiter=2000, precond=precond)
        assert S.info['converged'] and S.info['breakdown'] is None
        A, LS, uref = _reference(S, V.NONSYM, kvs, _geo(2), fixed, vals, rhs)
        _check_solution(S, u, A, LS, uref, fixed, vals, rhs, 1e-10)
        free = np.setdiff1d(np.arange(S.n), fixed)
        if precond == 'jacobi':
            dinv = 1.0 / A.diagonal()[free]
            Mf = (lambda v: dinv * v)
        else:
            P = V.BlockKronModel(S.ndofs, S.kron_factors())

            def Mf(v):
                full = np.zeros(S.n)
                full[free] = v
                return P.apply(full)[free]
        _, inf = BM.bicgstab(LS.A, LS.b, tol=1e-10, maxiter=2000, M=Mf)
        assert inf['converged'] and abs(S.info['iterations'] - inf['iterations']) <= 2, (S.info['iterations'], inf)
        assert np.array_equal(S.solve(tol=1e-10, maxiter=2000, precond=precond), u)
        assert np.array_equal(S.solve(tol=1e-10, maxiter=2000, precond=precond, check_every=10), u)
        with pytest.raises(_lib.IgxError):
            S.set_method('cg')                                     # made as non-symmetric: IGX_ERR_UNSUPPORTED
    finally:
        S.close()


def test_rhs_forms_and_shapes():
    kvs = (bspline.make_knots(2, 0.0, 1.0, 8),) * 2
    N = int(np.prod([kv.numdofs for kv in kvs]))
    fixed = V.side_dofs(kvs, [(1, 0)], 2)
    bcs = (fixed, np.zeros(fixed.size))
    f = assemble.assemble('inner(f, v) * dx', kvs, bfuns=[('v', 2)], geo=_geo(2), f=(1.0, -0.5), layout='blocked')
    assert np.shape(f) == (2,) + tuple(kv.numdofs for kv in kvs)
    us = []
    for rhs, kw in (('inner(f, v) * dx', dict(f=(1.0, -0.5))), (f, {}), (np.ravel(f), {})):
        S = solvers.VectorFormSystem(V.ELASTICITY, kvs, rhs, bcs, bfuns=V.bfuns(2), geo=_geo(2), **MU_LAM, **kw)
        try:
            us.append(S.solve(tol=1e-10))
            assert S.info['converged']
        finally:
            S.close()
    assert np.array_equal(us[0], us[1]) and np.array_equal(us[1], us[2])
    S = solvers.VectorFormSystem(V.ELASTICITY, kvs, 1.0, bcs, bfuns=V.bfuns(2), geo=_geo(2), **MU_LAM)
    try:
        assert np.array_equal(S.b, np.ones(2 * N))
    finally:
        S.close()


# ---------------------------------------------------------------------------------------------
def test_refusals():
    lib = _lib.load()
    kvs = (bspline.make_knots(2, 0.0, 1.0, 6),) * 2
    from pyiga_amd.form_assemblers import FormAssembler
    FA = FormAssembler(kvs, _geo(2), V.ELASTICITY, bfuns=V.bfuns(2), inputs=MU_LAM)
    patch = FA.patch
    h = C.c_void_p()
    fixed = np.zeros(0, dtype=np.int64)
    _lib.check(lib.igx_solver_create_block(patch.handle, 2, 1, fixed.ctypes.data_as(C.POINTER(C.c_int64)), 0, C.byref(h)),
               'igx_solver_create_block')
    s = h.value
    try:
        n = 2 * int(np.prod(patch.ndofs))
        # no IGX_FORM values yet; then the diagonal block (0, 0) only
        assert lib.igx_solver_take_block(s, 0, 0) == _lib.IGX_ERR_ARG
        patch.set_form(_full_table(FA._table[0][0], 2))
        patch.assemble('form', to_host=False)
        assert lib.igx_solver_take_block(s, 2, 0) == _lib.IGX_ERR_ARG
        assert lib.igx_solver_take_block(s, 0, 0) == _lib.IGX_OK
        assert lib.igx_d_csr_data(patch.handle) is None            # handed over: the patch holds no values
        patch.assemble('form', to_host=False)
        assert lib.igx_solver_take_block(s, 0, 0) == _lib.IGX_ERR_ARG      # taken twice
        ctx = patch.ctx
        from pyiga_amd.operators import DeviceArray
        d_x, d_y = DeviceArray.from_host(ctx, np.ones(n)), DeviceArray(ctx, n)
        assert lib.igx_solver_spmv_d(s, d_x.ptr, d_y.ptr) == _lib.IGX_ERR_ARG          # diagonal block (1, 1) missing
        assert lib.igx_solver_set_precond(s, _lib.IGX_PRECOND_JACOBI, None, None, None, None, 0) == _lib.IGX_ERR_ARG
        assert 'diagonal block (1, 1)' in _lib.last_error()
        u = np.empty(n)
        b = np.zeros(n)
        assert lib.igx_solver_solve(s, _lib.dptr(b), None, None, 1e-8, 10, 1, 0, _lib.dptr(u), None) == _lib.IGX_ERR_ARG
        assert lib.igx_solver_take_block(s, 1, 1) == _lib.IGX_OK                       # (the values of block (0, 0): any will do)
        assert lib.igx_solver_spmv_d(s, d_x.ptr, d_y.ptr) == _lib.IGX_OK
        assert lib.igx_solver_set_precond(s, _lib.IGX_PRECOND_KRON, None, None, None, None, 0) == _lib.IGX_ERR_ARG   # no factors
    finally:
        lib.igx_solver_destroy(s)
        patch.close()
    # a closed system
    S, *_ = _elasticity_2d(n=6, p=2)
    S.close()
    for call in (lambda: S.solve(), lambda: S.spmv(np.zeros(S.n)), lambda: S.apply_precond(np.zeros(S.n), 'jacobi')):
        with pytest.raises(_lib.IgxError):
            call()

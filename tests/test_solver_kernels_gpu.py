"""The solver kernels of pyiga_amd/csrc/solve.hip at every SpMV width and past one grid of rows, each against a plain
high-precision reference of the same operation.

The reference is the matrix the device assembled, downloaded once and multiplied by scipy in long double (64 mantissa bits):
the assembly is checked elsewhere, these tests isolate the solver kernels.
- SpMV (k_spmv, k_csr_spmv): every case of tests/_solver_cases.py, mass and stiffness, row by row against the rounding bound of
  the row's own dot product, with inputs spread over 40 binades so that a dropped or mis-gathered entry cannot hide.
- Preconditioners applied alone: Jacobi (k_diag, k_csr_diag, k_scale) bit for bit, none (k_mask_copy) exactly, Kronecker
  (k_kron through apply_kron) and Schwarz against the numpy contraction model of tests/_mpsolve_model.py.
- Solves past the vector grid (n > NB_VEC * BLOCK) of a manufactured discrete solution: the true residual recomputed in long
  double, the Dirichlet values, the iteration count against the host models, bit-identical repeats, and the dot products of
  the start (relres at maxiter = 0) against the host.
"""
import zlib

import numpy as np
import pytest
import scipy.sparse

from pyiga_amd import _lib, assemble, geometry, solvers

import _bicgstab_model as BM
import _mpsolve_model as M
import _solver_cases as sc

pytestmark = pytest.mark.gpu

STIFF = 'inner(grad(u),grad(v))*dx'
MASS = 'u*v*dx'
CD3_FORM = '(inner(diff_coeff*grad(u),grad(v))+inner((x[1],-x[0],1.0),grad(u))*v)*dx'
U53 = 2.0 ** -53


def _cyl():
    return geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.quarter_annulus())


def _geo(dim):
    return geometry.quarter_annulus() if dim == 2 else _cyl()


def _rng(tag):
    return np.random.default_rng(zlib.crc32(tag.encode()))


def _spread(rng, n, binades=20):
    """Random signs, magnitudes 2^[-binades, binades]."""
    return rng.choice([-1.0, 1.0], n) * np.exp2(rng.uniform(-binades, binades, n))


def _ld(A):
    A = A.tocsr()
    return scipy.sparse.csr_matrix((A.data.astype(np.longdouble), A.indices, A.indptr), shape=A.shape)


def _patch_matrix(S, kind):
    """The values the device assembled for `S` (assembled again into the same place, downloaded) as a host CSR."""
    vals = S.patch.assemble(kind, to_host=True)
    indptr, indices = S.patch.pattern()
    return scipy.sparse.csr_matrix((vals, indices, indptr), shape=(S.n, S.n))


def _mp_matrix(MP):
    """The global sums the multipatch holds on the device now (those its solvers read), downloaded."""
    indptr, indices = MP.pattern()
    data = np.empty(indices.shape[0])
    b = np.empty(MP.numdofs)
    _lib.check(_lib.load().igx_multipatch_download(MP._device(), _lib.dptr(data), _lib.dptr(b)), 'igx_multipatch_download')
    return scipy.sparse.csr_matrix((data, indices.copy(), indptr.copy()), shape=(MP.numdofs, MP.numdofs))


def _check_spmv(S, A, fixed, tag):
    """y = R A R^T x on the device against long double, row by row; fixed rows exactly 0, and the values of x at fixed dofs
    never read."""
    n = A.shape[0]
    rng = _rng(tag)
    free = np.ones(n, dtype=bool)
    free[fixed] = False
    x = _spread(rng, n)
    y = S.spmv(x)
    xf = np.where(free, x, 0.0)
    Al = _ld(A)
    ref = np.where(free, Al @ xf.astype(np.longdouble), 0.0)
    mag = abs(Al) @ np.abs(xf).astype(np.longdouble)
    lens = np.diff(A.indptr)
    bound = 2 * lens * U53 * mag
    err = np.abs(y.astype(np.longdouble) - ref)
    bad = np.flatnonzero(free & (err > bound))
    assert bad.size == 0, (tag, bad.size, bad[:8], [float(err[i] / max(mag[i], 1e-300)) for i in bad[:4]])
    assert np.all(y[~free] == 0.0), tag
    assert np.all(mag[free] > 0)                             # (no free row without entries: each row is checked)
    x2 = x.copy()
    x2[fixed] = _spread(rng, fixed.size) * 1e3
    assert np.array_equal(S.spmv(x2), y), tag                # the R^T side: fixed entries of x are not read


def _check_jacobi_and_none(S, A, fixed, tag):
    n = A.shape[0]
    free = np.ones(n, dtype=bool)
    free[fixed] = False
    r = _spread(_rng(tag + 'r'), n, 8)
    z = S.apply_precond(r, 'jacobi')
    ref = np.where(free, (1.0 / A.diagonal()) * r, 0.0)
    assert np.array_equal(z, ref), (tag, int(np.count_nonzero(z != ref)))
    S.set_precond(None)
    z = S.apply_precond(r)
    assert np.array_equal(z, np.where(free, r, 0.0)), tag


# ---------------------------------------------------------------------------------------------
# SpMV: every width, past one grid of rows
def _patch_fixed(kvs, rng):
    n = int(np.prod([kv.numdofs for kv in kvs]))
    d = len(kvs)
    return np.unique(np.concatenate([assemble.boundary_dofs(kvs, (0, 0), ravel=True),
                                     assemble.boundary_dofs(kvs, (d - 1, 1), ravel=True),
                                     rng.choice(n, size=max(1, n // 50), replace=False)]))


@pytest.mark.parametrize('case', sc.PATCH_CASES, ids=[c.id for c in sc.PATCH_CASES])
@pytest.mark.parametrize('kind', ['mass', 'stiffness'])
def test_patch_spmv_and_jacobi(case, kind):
    kvs = case.kvs()
    n = int(np.prod([kv.numdofs for kv in kvs]))
    fixed = _patch_fixed(kvs, _rng(case.id + kind + 'fixed'))
    S = solvers.PatchSystem(kvs, _geo(case.dim), np.zeros(n), (fixed, np.zeros(fixed.size)), kind=kind)
    try:
        A = _patch_matrix(S, kind)
        maxlen = sc.max_row(A)
        assert maxlen == sc.patch_maxlen(kvs) and sc.spmv_gw(maxlen) == case.gw, (case.id, maxlen)
        _check_spmv(S, A, fixed, case.id + kind)
        _check_jacobi_and_none(S, A, fixed, case.id + kind)
    finally:
        S.close()


def _mp_fixed(MP, case, rng):
    sides = {'lshape': [(0, 'left'), (0, 'bottom'), (2, 'top')], 'notebook': M.NOTEBOOK_DIRICHLET,
             'cubes2': [(0, (2, 0)), (1, (0, 1))]}[case.domain]
    n = MP.numdofs
    return np.unique(np.concatenate([M.fixed_dofs(MP, sides), rng.choice(n, size=max(1, n // 50), replace=False)]))


def f_one(*x):
    return 1.0 + 0.0 * x[0]


@pytest.mark.parametrize('case', sc.MULTIPATCH_CASES, ids=[c.id for c in sc.MULTIPATCH_CASES])
@pytest.mark.parametrize('kind', ['mass', 'stiffness'])
def test_multipatch_spmv_and_jacobi(case, kind):
    MP = case.build()
    fixed = _mp_fixed(MP, case, _rng(case.id + kind + 'fixed'))
    S = solvers.MultipatchSystem(MP, MASS if kind == 'mass' else STIFF, 'f*v*dx', bcs=(fixed, np.zeros(fixed.size)), f=f_one)
    try:
        A = _mp_matrix(MP)
        # the device pattern is the host's sum of X_p A_p X_p^T, and its longest row decides the width
        H = sc.multipatch_pattern(MP)
        assert np.array_equal(A.indptr, H.indptr) and np.array_equal(A.indices, H.indices), case.id
        assert sc.spmv_gw(sc.max_row(A)) == case.gw, (case.id, sc.max_row(A))
        _check_spmv(S, A, fixed, case.id + kind)
        _check_jacobi_and_none(S, A, fixed, case.id + kind)
    finally:
        S.close()
        MP.close()


# ---------------------------------------------------------------------------------------------
# Kronecker and Schwarz preconditioners applied alone
def _kron_model(S):
    """SchwarzModel with one part and the identity map: the contraction model of the patch's Kronecker preconditioner."""
    U, lam, mode = S._kron_factors()
    n = S.n
    return M.SchwarzModel(n, [tuple(S.ndofs)], [np.arange(n)], S.bc_indices, [S.box], [U], [lam], mode)


def _check_kron_apply(S, tag):
    r = _spread(_rng(tag + 'kron'), S.n, 4)
    z = S.apply_precond(r, 'kron')
    ref = _kron_model(S).apply(r)
    assert np.abs(z - ref).max() <= 1e-12 * np.abs(ref).max(), (tag, np.abs(z - ref).max() / np.abs(ref).max())
    assert not z[S.bc_indices].any(), tag


KRON_KVS = {
    2: ((2, 70, 1), (3, 29, 1)),                       # 72 x 32 dofs: the first axis crosses a 64-row tile
    3: ((2, 9, 1), (3, 66, 1), (1, 7, 1)),             # 11 x 69 x 8
}
KRON_SIDES = {
    'all': 'all',
    'one': [(0, 0)],
    'opposite': [(0, 0), (0, 1)],
    'three': [(0, 1), (1, 0), (1, 1)],
}


def _kvs(axes):
    from pyiga_amd import bspline
    return tuple(bspline.make_knots(p, 0.0, 1.0, n, mult=m) for p, n, m in axes)


def _side_dofs(kvs, sides):
    if sides == 'all':
        sides = [(k, s) for k in range(len(kvs)) for s in (0, 1)]
    return np.unique(np.concatenate([assemble.boundary_dofs(kvs, bd, ravel=True) for bd in sides]))


@pytest.mark.parametrize('dim', [2, 3])
@pytest.mark.parametrize('sides', sorted(KRON_SIDES))
@pytest.mark.parametrize('kind', ['mass', 'stiffness'])
def test_kron_precond_vs_contraction_model(dim, sides, kind):
    kvs = _kvs(KRON_KVS[dim])
    fixed = _side_dofs(kvs, KRON_SIDES[sides])
    n = int(np.prod([kv.numdofs for kv in kvs]))
    S = solvers.PatchSystem(kvs, _geo(dim), np.zeros(n), (fixed, np.ones(fixed.size)), kind=kind)
    try:
        assert S.box is not None
        _check_kron_apply(S, 'kron%d%s%s' % (dim, sides, kind))
    finally:
        S.close()


@pytest.mark.parametrize('dim', [2, 3])
def test_kron_precond_mass_without_fixed_dofs(dim):
    kvs = _kvs(KRON_KVS[dim])
    n = int(np.prod([kv.numdofs for kv in kvs]))
    S = solvers.PatchSystem(kvs, _geo(dim), np.zeros(n), None, kind='mass')
    try:
        _check_kron_apply(S, 'kronfree%d' % dim)
    finally:
        S.close()


@pytest.mark.parametrize('dim', [2, 3])
def test_kron_precond_of_a_form_system(dim):
    """FormSystem: the factors of the parametric Laplacian on the free box (IGX_KRON_SUM) for a non-symmetric form."""
    kvs = _kvs(KRON_KVS[dim])
    fixed = _side_dofs(kvs, KRON_SIDES['three'])
    if dim == 2:
        S = solvers.FormSystem('(inner(grad(u), grad(v)) + inner((x[1] + 2.0, 1.0 - x[0]), grad(u)) * v) * dx', kvs, 0.0,
                               (fixed, np.ones(fixed.size)), geo=_geo(2))
    else:
        S = solvers.FormSystem(CD3_FORM, kvs, 0.0, (fixed, np.ones(fixed.size)), geo=_cyl(), diff_coeff=lambda x, y, z: 0.5 + z)
    try:
        assert S.default_precond == 'kron'
        _check_kron_apply(S, 'kronform%d' % dim)
    finally:
        S.close()


# ---------------------------------------------------------------------------------------------
# solves of a manufactured discrete solution past the vector grid
def _manufactured(A, n, fixed, tag):
    """u* (nonzero everywhere), b = A u* formed in long double and rounded, g = u*[fixed]."""
    rng = _rng(tag)
    u_star = rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)
    b = (_ld(A) @ u_star.astype(np.longdouble)).astype(np.float64)
    return u_star, b, u_star[fixed].copy()


def _residuals(A, b, fixed, g, u):
    """||R (b - A u)||, ||R (b - A ext(g))|| and the free part of b - A ext(g), in long double."""
    free = np.ones(A.shape[0], dtype=bool)
    free[fixed] = False
    Al = _ld(A)
    ext = np.zeros(A.shape[0])
    ext[fixed] = g
    r0 = (b.astype(np.longdouble) - Al @ ext.astype(np.longdouble))[free]
    r = (b.astype(np.longdouble) - Al @ u.astype(np.longdouble))[free]
    return float(np.sqrt(np.sum(r * r))), float(np.sqrt(np.sum(r0 * r0))), r0


def _check_start(S, A, rhs, fixed, g, tag, precond, **solve_kw):
    """maxiter = 0 from a random x0: relres is ||r0 - R A R^T x0|| / ||r0|| as the device's dot products (k_dot2, or the partials
    of k_update / the first BiCGStab reduction) form it over several grid-stride passes; against long double."""
    n = A.shape[0]
    free = np.ones(n, dtype=bool)
    free[fixed] = False
    x0 = np.where(free, _rng(tag + 'x0').standard_normal(n), 0.0)
    _, nrm0, r0 = _residuals(A, rhs, fixed, g, np.zeros(n))
    Al = _ld(A)
    r1 = r0 - (Al @ x0.astype(np.longdouble))[free]
    ref = float(np.sqrt(np.sum(r1 * r1))) / nrm0
    S.solve(tol=1e-8, maxiter=0, precond=precond, x0=x0, **solve_kw)
    assert S.info['iterations'] == 0
    assert abs(S.info['relres'] - ref) <= 1e-12 * ref, (tag, precond, S.info['relres'], ref)


def _check_solution(S, A, b, fixed, g, u, tol, tag):
    assert S.info['converged'], (tag, S.info)
    assert np.array_equal(u[fixed], g), tag
    res, nrm0, _ = _residuals(A, b, fixed, g, u)
    assert res <= 2 * tol * nrm0, (tag, res / nrm0)


def _restricted(A, fixed, b, g):
    n = A.shape[0]
    free = np.ones(n, dtype=bool)
    free[fixed] = False
    ext = np.zeros(n)
    ext[fixed] = g
    Aff = A[free][:, free].tocsr()
    return free, Aff, (b - A @ ext)[free]


def _restrict_op(model, free):
    n = free.size

    def op(r):
        z = np.zeros(n)
        z[free] = r
        return model.apply(z)[free]
    return op


def _cg_model_iterations(A, fixed, b, g, precond_op, tol):
    free, Aff, rhs = _restricted(A, fixed, b, g)
    it, _, info = M.cg_iterations(Aff, rhs, precond_op, tol)
    assert info == 0
    return it


TOL = 1e-8


def test_patch_cg_kron_2d_past_the_vector_grid():
    case = next(c for c in sc.PATCH_CASES if c.id == '2d_p1_n725')
    kvs = case.kvs()
    n = int(np.prod([kv.numdofs for kv in kvs]))
    assert n > sc.vec_pass_rows()
    fixed = _side_dofs(kvs, 'all')
    S = solvers.PatchSystem(kvs, _geo(2), np.zeros(n), (fixed, np.ones(fixed.size)), kind='stiffness')
    try:
        A = _patch_matrix(S, 'stiffness')
        _check_kron_apply(S, 'cgkron2d')                     # (a 724 x 724 box: 12 x 12 tiles per contraction)
        _, b, g = _manufactured(A, n, fixed, 'cgkron2d')
        S.b[:] = b
        S.bc_values[:] = g
        u = S.solve(tol=TOL, maxiter=500, precond='kron')
        _check_solution(S, A, b, fixed, g, u, TOL, 'cgkron2d')
        it = S.info['iterations']
        assert np.array_equal(S.solve(tol=TOL, maxiter=500, precond='kron'), u)
        free = np.ones(n, dtype=bool)
        free[fixed] = False
        m = _cg_model_iterations(A, fixed, b, g, _restrict_op(_kron_model(S), free), TOL)
        assert abs(it - m) <= 2, (it, m)
        for precond in ('kron', 'jacobi', None):
            _check_start(S, A, b, fixed, g, 'cgkron2d', precond)
    finally:
        S.close()


def test_patch_cg_jacobi_3d_past_the_vector_grid_and_check_every():
    from pyiga_amd import bspline
    kvs = 3 * (bspline.make_knots(1, 0.0, 1.0, 64),)
    n = int(np.prod([kv.numdofs for kv in kvs]))
    assert n == 65 ** 3 and n > sc.vec_pass_rows()
    rng = _rng('cgjac3d')
    fixed = np.unique(np.concatenate([_side_dofs(kvs, [(0, 0), (2, 1)]), rng.choice(n, size=n // 100, replace=False)]))
    S = solvers.PatchSystem(kvs, _cyl(), np.zeros(n), (fixed, np.ones(fixed.size)), kind='stiffness')
    try:
        A = _patch_matrix(S, 'stiffness')
        _, b, g = _manufactured(A, n, fixed, 'cgjac3d')
        S.b[:] = b
        S.bc_values[:] = g
        u = S.solve(tol=TOL, maxiter=2000, precond='jacobi')
        _check_solution(S, A, b, fixed, g, u, TOL, 'cgjac3d')
        it = S.info['iterations']
        assert np.array_equal(S.solve(tol=TOL, maxiter=2000, precond='jacobi'), u)
        free = np.ones(n, dtype=bool)
        free[fixed] = False
        dinv = 1.0 / A.diagonal()[free]
        m = _cg_model_iterations(A, fixed, b, g, lambda r: dinv * r, TOL)
        assert abs(it - m) <= 2, (it, m)
        # check_every: the same iterations, read back every 7th -- CG stops at the first check past convergence
        u7 = S.solve(tol=TOL, maxiter=2000, precond='jacobi', check_every=7)
        assert S.info['iterations'] == -(-it // 7) * 7, (S.info['iterations'], it)
        _check_solution(S, A, b, fixed, g, u7, TOL, 'cgjac3d/7')
        for precond in ('jacobi', None):
            _check_start(S, A, b, fixed, g, 'cgjac3d', precond)
    finally:
        S.close()


def kappa3(x, y, z):
    return 0.2 + 0.1 * z


@pytest.mark.parametrize('precond', ['kron', 'jacobi'])
def test_form_bicgstab_3d_past_the_vector_grid(precond):
    from pyiga_amd import bspline
    kvs = 3 * (bspline.make_knots(2, 0.0, 1.0, 63),)
    n = int(np.prod([kv.numdofs for kv in kvs]))
    assert n == 65 ** 3 and n > sc.vec_pass_rows()
    fixed = _side_dofs(kvs, 'all')
    S = solvers.FormSystem(CD3_FORM, kvs, 0.0, (fixed, np.ones(fixed.size)), geo=_cyl(), diff_coeff=kappa3)
    try:
        A = _patch_matrix(S, S.kind)
        tag = 'bicg3d' + precond
        if precond == 'kron':
            _check_kron_apply(S, tag)
        _, b, g = _manufactured(A, n, fixed, tag)
        S.b[:] = b
        S.bc_values[:] = g
        u = S.solve(tol=TOL, maxiter=3000, precond=precond)
        _check_solution(S, A, b, fixed, g, u, TOL, tag)
        assert S.info['method'] == 'bicgstab' and S.info['breakdown'] is None, S.info
        it = S.info['iterations']
        assert np.array_equal(S.solve(tol=TOL, maxiter=3000, precond=precond), u)
        # frozen after the stop: reading back every 10th iteration changes nothing
        assert np.array_equal(S.solve(tol=TOL, maxiter=3000, precond=precond, check_every=10), u)
        assert S.info['iterations'] == it
        free, Aff, rhs = _restricted(A, fixed, b, g)
        if precond == 'jacobi':
            dinv = 1.0 / Aff.diagonal()
            Mop = lambda r: dinv * r                                           # noqa: E731
        else:
            Mop = _restrict_op(_kron_model(S), free)
        _, inf = BM.bicgstab(Aff, rhs, tol=TOL, maxiter=3000, M=Mop)
        assert inf['converged'] and abs(it - inf['iterations']) <= 3, (it, inf['iterations'])
        _check_start(S, A, b, fixed, g, tag, precond)
    finally:
        S.close()


def test_multipatch_schwarz_past_the_vector_grid():
    case = next(c for c in sc.MULTIPATCH_CASES if c.id == 'notebook_p3_n260')
    MP = case.build()
    n = MP.numdofs
    assert n > sc.vec_pass_rows() and n > sc.spmv_pass_rows(case.gw)
    rng = _rng('mpschwarz')
    fixed = np.unique(np.concatenate([M.fixed_dofs(MP, M.NOTEBOOK_DIRICHLET), rng.choice(n, size=n // 200, replace=False)]))
    S = solvers.MultipatchSystem(MP, STIFF, 'f*v*dx', bcs=(fixed, np.ones(fixed.size)), f=f_one)
    try:
        A = _mp_matrix(MP)
        # the preconditioner alone, against the contraction model
        boxes, U, lam, mode = S.schwarz_setup()
        shapes, maps = M.shapes_maps(MP)
        model = M.SchwarzModel(n, shapes, maps, fixed, boxes, U, lam, mode)
        r = _spread(_rng('mpschwarz r'), n, 4)
        z = S.apply_precond(r, 'schwarz')
        ref = model.apply(r)
        assert np.abs(z - ref).max() <= 1e-12 * np.abs(ref).max()
        assert not z[fixed].any()
        # the solve of a manufactured solution
        _, b, g = _manufactured(A, n, fixed, 'mpschwarz')
        S.bc_values[:] = g
        u = S.solve(tol=TOL, maxiter=1000, precond='schwarz', b=b)
        _check_solution(S, A, b, fixed, g, u, TOL, 'mpschwarz')
        it = S.info['iterations']
        assert np.array_equal(S.solve(tol=TOL, maxiter=1000, precond='schwarz', b=b), u)
        free = model.free
        m = _cg_model_iterations(A, fixed, b, g, _restrict_op(model, free), TOL)
        assert abs(it - m) <= 2, (it, m)
        for precond in ('schwarz', 'jacobi', None):
            _check_start(S, A, b, fixed, g, 'mpschwarz', precond, b=b)
    finally:
        S.close()
        MP.close()

"""Hierarchical spline spaces on the device: `assemble.assemble(form, hs, ...)` against the reference's matrices
(tests/golden/golden_hier.npz), the self-checks of the contraction kernel, the affine identity that needs no golden data,
function evaluation, and a Poisson solve end to end.

Tolerances: 1e-12 relative (`rel_maxdiff`) is what the entry-wise kernel meets against the reference (tests/test_gpu_parity.py
RTOL); the contraction weights are non-negative and sum to at most one per axis, so they do not amplify it.  THB matrices are
T' A T: the bound is multiplied by the measured amplification `thb_amp` of that product (golden file, 2.0 .. 3.2)."""
import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.linalg

import _hier_cases as hc
from conftest import golden_csr

from pyiga_amd import approx, assemble, bspline, geometry, hierarchical
from pyiga_amd.hierarchical import HDiscretization, HSpace, HSplineFunc

pytestmark = pytest.mark.gpu

RTOL = 1e-12
CASE_IDS = list(hc.CASES)
_SPACES, _MATS = {}, {}


def space(name):
    if name not in _SPACES:
        _SPACES[name] = hc.build(bspline, HSpace, name)[0]
    return _SPACES[name]


def gold_matrix(g, name):
    if name + 'u_data' in g.files:
        U = golden_csr(g, name + 'u')
        return (U + scipy.sparse.triu(U, k=1).T).tocsr()
    return golden_csr(g, name)


def tol(g, name, base=RTOL):
    return base * max(1.0, float(g[name + '_thb_amp'])) if hc.CASES[name][1] else base


def device_matrix(name, form, affine=False, **inputs):
    key = (name, form, affine)
    if key not in _MATS:
        hs = space(name)
        _MATS[key] = assemble.assemble(form, hs, geo=hc.geometry_of(geometry, hs.dim, affine=affine), **inputs)
    return _MATS[key]


@pytest.mark.parametrize('name', CASE_IDS)
def test_matrix_and_rhs_match_reference(golden, name):
    g = golden('hier')
    hs = space(name)
    A = device_matrix(name, hc.CASES[name][5])
    assert A.shape == (hs.numdofs, hs.numdofs) and scipy.sparse.isspmatrix_csr(A)
    err = hc.rel_maxdiff(A, gold_matrix(g, name + '_A'))
    b = assemble.assemble('f * v * dx', hs, geo=hc.geometry_of(geometry, hs.dim), f=hc.f_rhs)
    errb = abs(b - g[name + '_rhs']).max() / abs(g[name + '_rhs']).max()
    print(name, 'device vs reference: matrix %.2e rhs %.2e (bound %.1e)' % (err, errb, tol(g, name)))
    assert err < tol(g, name)
    assert errb < tol(g, name)


@pytest.mark.parametrize('name', hc.EXTRA_FORM_CASES)
def test_mass_and_coefficient_form_match_reference(golden, name):
    g = golden('hier')
    errM = hc.rel_maxdiff(device_matrix(name, hc.MASS), gold_matrix(g, name + '_M'))
    errC = hc.rel_maxdiff(device_matrix(name, hc.COEFF, c=hc.c_coeff), gold_matrix(g, name + '_C'))
    print(name, 'mass %.2e coefficient form %.2e' % (errM, errC))
    assert errM < tol(g, name)
    assert errC < tol(g, name)


def test_kernel_self_checks():
    """The pattern is the host plan's, two runs give the same bits, symmetric forms give an exactly symmetric matrix, and
    computing one orientation (symmetric=True) agrees with computing both."""
    hs = space('hb2d')
    geo = hc.geometry_of(geometry, 2)
    disc = HDiscretization(hs, hc.STIFF, {'geo': geo})
    v1 = disc.assemble_hb_values()
    assert disc.values_d
    pl = hierarchical.plan(hs)
    assert np.array_equal(disc.indptr, pl['indptr']) and np.array_equal(disc.indices, pl['indices'])
    assert v1.size == pl['indices'].size and np.isfinite(v1).all()
    v2 = disc.assemble_hb_values()
    assert np.array_equal(v1, v2)
    n = hs.numdofs
    A = scipy.sparse.csr_matrix((v1, disc.indices, disc.indptr), shape=(n, n))
    assert abs(A - A.T).max() == 0.0
    disc.close()
    # a symmetric form through the general path: both orientations summed (symmetric=False) against one mirrored
    for name, form, inputs in (('hb2d', hc.COEFF, {'c': hc.c_coeff}), ('hb3', hc.COEFF, {'c': hc.c_coeff})):
        hs = space(name)
        d2 = HDiscretization(hs, form, dict(inputs, geo=hc.geometry_of(geometry, hs.dim)))
        both = d2.assemble_hb_values(symmetric=False)
        one = d2.assemble_hb_values(symmetric=True)
        d2.close()
        assert abs(both - one).max() <= 1e-13 * abs(both).max()
        n = hs.numdofs
        S = scipy.sparse.csr_matrix((one, d2.indices, d2.indptr), shape=(n, n))
        assert abs(S - S.T).max() == 0.0


@pytest.mark.parametrize('name,form', [('hb2d', hc.STIFF), ('nonsym', hc.NONSYM), ('hb3', hc.STIFF)])
def test_grid_wrap(name, form):
    """The grid of the contraction capped at 2 blocks: every group walks many items; the values are the same bits."""
    hs = space(name)
    geo = hc.geometry_of(geometry, hs.dim)
    free = HDiscretization(hs, form, {'geo': geo})
    capped = HDiscretization(hs, form, {'geo': geo}, max_blocks=2)
    v0, v1 = free.assemble_hb_values(), capped.assemble_hb_values()
    free.close()
    capped.close()
    assert v0.size > 2 * 16 * 8 and np.array_equal(v0, v1)


@pytest.mark.parametrize('name', hc.AFFINE_CASES)
def test_affine_identity(name):
    """On an affine geometry the Gauss rules of all levels are exact for the same integrands, so the hierarchical matrix is
    I' A_fine I with I = represent_fine() -- a check that needs no golden data."""
    hs = space(name)
    geo = hc.geometry_of(geometry, hs.dim, affine=True)
    I = hs.represent_fine()
    kvs = hs.knotvectors(-1)
    for form, fine in ((hc.STIFF, assemble.stiffness(kvs, geo)), (hc.MASS, assemble.mass(kvs, geo))):
        A = device_matrix(name, form, affine=True)
        ref = (I.T @ fine @ I).toarray()
        err = hc.rel_maxdiff(A, ref)
        print(name, form, 'affine identity %.2e' % err)
        assert err < RTOL
    # the load vector: a polynomial of degree one per axis, which the rule of every level (max(p) + 1 >= 3 points per span)
    # integrates exactly against the basis functions, so the levels differ by rounding only
    def poly(*X):
        return 1.0 + X[0] * X[1] + (X[2] if len(X) == 3 else 0.0)
    b = assemble.assemble('f * v * dx', hs, geo=geo, f=poly)
    ref = I.T @ assemble.inner_products(kvs, poly, f_physical=True, geo=geo).ravel()
    assert abs(b - ref).max() / abs(ref).max() < RTOL


@pytest.mark.parametrize('name', hc.EVAL_CASES)
@pytest.mark.parametrize('truncate', [False, True])
def test_function_evaluation(name, truncate):
    hs = space(name)
    u = np.random.default_rng(7).standard_normal(hs.numdofs)
    f = HSplineFunc(hs, u, truncate=truncate)
    fine = bspline.BSplineFunc(hs.knotvectors(-1), hs.represent_fine(truncate=truncate) @ u)
    grid = 2 * (np.linspace(0, 1, 9),)
    assert f.sdim == 2 and f.dim == 1 and f.support == ((0.0, 1.0), (0.0, 1.0))
    for mine, ref in ((f.grid_eval(grid), fine.grid_eval(grid)), (f.grid_jacobian(grid), fine.grid_jacobian(grid)),
                      (f.grid_hessian(grid), fine.grid_hessian(grid))):
        assert mine.shape == ref.shape
        assert abs(mine - ref).max() <= 1e-12 * abs(ref).max()
    vals = f.grid_eval(grid)
    # the point value is the same evaluation on a grid of one point: it EQUALS the grid entry (an axis slip would not)
    point = f(grid[1][3], grid[0][5])
    print(name, truncate, 'point value - grid entry: %.3e' % (point - vals[5, 3]))
    assert point == vals[5, 3]
    assert f.eval(grid[1][2], grid[0][7]) == vals[7, 2]
    assert abs(hs.grid_eval(u, grid, truncate=truncate) - vals).max() == 0.0


def test_poisson_and_projection_end_to_end(golden):
    g = golden('hier')
    name = hc.SOLVE_CASE
    hs = space(name)
    geo = hc.geometry_of(geometry, hs.dim)
    A = device_matrix(name, hc.STIFF)
    b = assemble.assemble('f * v * dx', hs, geo=geo, f=hc.f_rhs)
    free = np.array(hs.non_dirichlet_dofs())
    assert np.array_equal(free, g[name + '_free'])
    u = scipy.sparse.linalg.spsolve(A[free][:, free].tocsc(), b[free])
    err = abs(u - g[name + '_u']).max() / abs(g[name + '_u']).max()
    bound = 10 * float(g[name + '_solve_amp']) * 1e-12
    proj = approx.project_L2(hs, hc.f_rhs, f_physical=True, geo=geo)
    errp = abs(proj - g[name + '_proj']).max() / abs(g[name + '_proj']).max()
    boundp = 10 * float(g[name + '_proj_amp']) * 1e-12
    print('solve %.2e (bound %.1e)  projection %.2e (bound %.1e)' % (err, bound, errp, boundp))
    assert err < bound
    assert errp < boundp

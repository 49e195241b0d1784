"""Multipatch solver host side without a GPU: the Schwarz boxes of every patch, the floating-patch shift, a numpy model of the
whole Schwarz operator (SPD on the free dofs; fewer CG iterations than Jacobi on the notebook domain), the new C ABI names,
and MultipatchSystem failing loudly without a device."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse

from conftest import ROOT
from pyiga_amd import _lib, assemble, solvers

import _mpsolve_model as M

GOLD = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'golden_multipatch.npz'))
NEW_NAMES = ('igx_solver_create_multipatch', 'igx_solver_set_schwarz', 'igx_solver_precond_d')


def _boxes(MP, fixed):
    shapes, maps = M.shapes_maps(MP)
    return solvers.schwarz_boxes(shapes, maps, fixed)


def test_notebook_numbering_by_hand_matches_reference():
    MP = M.notebook()
    assert MP.numdofs == GOLD['nb_numdofs']
    for p in range(4):
        assert np.array_equal(MP.patch_to_global_idx(p), GOLD['nb_p2g%d' % p])
    assert np.array_equal(M.fixed_dofs(MP, M.NOTEBOOK_DIRICHLET), GOLD['nb_bc_idx'])


def test_boxes_notebook():
    MP = M.notebook()
    fixed = GOLD['nb_bc_idx']
    # patch 0: bottom (0, 0) and right (1, 1); patch 1: top (0, 1); patch 2: bottom and left (1, 0); patch 3: bottom
    assert _boxes(MP, fixed) == [((1, 0), (18, 17)), ((0, 0), (17, 18)), ((1, 1), (18, 18)), ((1, 0), (18, 18))]


def test_boxes_corner_fixed_by_a_neighbour_stays_in_the_box():
    MP = M.lshape()
    fixed = M.fixed_dofs(MP, [(0, 'bottom')])
    lo, hi = _boxes(MP, fixed)[1]
    assert (lo, hi) == ((0, 0), (10, 10))
    # patch 0's bottom side ends in a dof of its right side, which patch 1 shares: fixed in patch 1, inside its box
    loc = np.isin(MP.patch_to_global_idx(1), fixed).reshape(10, 10)
    assert np.argwhere(loc).tolist() == [[0, 0]]


def test_boxes_lshape_with_flip():
    MP = M.lshape()
    fixed = M.fixed_dofs(MP, [(0, 'left'), (0, 'bottom'), (2, 'top'), (2, 'right')])
    assert _boxes(MP, fixed) == [((1, 1), (10, 10)), ((0, 0), (10, 10)), ((0, 0), (9, 9))]
    # a partly fixed side stays in the box
    MP = M.lshape()
    kvs = MP.patches[0][0]
    part = MP.patch_to_global_idx(0)[assemble.boundary_dofs(kvs, 'left', ravel=True)[:5]]
    assert _boxes(MP, part)[0] == ((0, 0), (10, 10))


def test_boxes_floating_patch():
    MP = M.lshape()
    fixed = M.fixed_dofs(MP, [(0, 'left')])
    boxes = _boxes(MP, fixed)
    assert boxes[0] == ((0, 1), (10, 10))
    assert boxes[1] == boxes[2] == ((0, 0), (10, 10))           # floating: no wholly fixed side


def _factors(MP, fixed, kind, oracle):
    shapes, maps = M.shapes_maps(MP)
    boxes = solvers.schwarz_boxes(shapes, maps, fixed)
    U, lam, mode = solvers.schwarz_factors([kvs for kvs, _ in MP.patches], boxes, kind, mats1d=M.mats1d_oracle(oracle, kind))
    return shapes, maps, boxes, U, lam, mode


def test_floating_shift_makes_every_block_spd(oracle):
    MP = M.lshape(p=2, n=5)
    fixed = M.fixed_dofs(MP, [(0, 'left')])
    shapes, maps, boxes, U, lam, mode = _factors(MP, fixed, 'stiffness', oracle)
    assert mode == _lib.IGX_KRON_SUM
    for p in range(3):
        D = np.add.outer(lam[p][0], lam[p][1])
        K = np.kron(U[p][0], U[p][1])
        B = K @ np.diag(1.0 / D.ravel()) @ K.T
        assert abs(B - B.T).max() <= 1e-12 * abs(B).max()
        assert np.linalg.eigvalsh(0.5 * (B + B.T)).min() > 0
    # without the shift the floating patches' eigenvalue sums have a (numerically) zero entry
    okv = oracle.KnotVector(MP.patches[1][0][0].kv, 2)
    K1 = oracle.bsp_mixed_deriv_biform_1d(okv, 1, 1).toarray()
    M1 = oracle.bsp_mixed_deriv_biform_1d(okv, 0, 0).toarray()
    import scipy.linalg
    w = scipy.linalg.eigh(K1, M1, eigvals_only=True)
    assert abs(w[0]) < 1e-10 * w[-1]
    sigma = w[1]                                                 # (both axes of the patch have this knot vector)
    assert np.allclose(lam[1][0], w + sigma / 2, rtol=1e-12, atol=1e-12 * w[-1])


@pytest.mark.parametrize('case', ['notebook', 'lshape_floating', 'lshape_mass'])
def test_schwarz_model_is_spd_on_free_dofs(case, oracle):
    if case == 'notebook':
        MP, kind = M.notebook(p=2, n=4), 'stiffness'
        fixed = M.fixed_dofs(MP, M.NOTEBOOK_DIRICHLET)
    else:
        MP, kind = M.lshape(p=2, n=4), ('mass' if case == 'lshape_mass' else 'stiffness')
        fixed = M.fixed_dofs(MP, [(0, 'left')] if case == 'lshape_floating' else [])
    shapes, maps, boxes, U, lam, mode = _factors(MP, fixed, kind, oracle)
    model = M.SchwarzModel(MP.numdofs, shapes, maps, fixed, boxes, U, lam, mode)
    P = model.dense()
    free = model.free
    Pf = P[np.ix_(free, free)]
    assert abs(Pf - Pf.T).max() <= 1e-12 * abs(Pf).max()
    assert np.linalg.eigvalsh(0.5 * (Pf + Pf.T)).min() > 0
    assert not P[~free].any() and not P[:, ~free].any()
    r = np.random.default_rng(1).standard_normal(MP.numdofs)
    assert np.allclose(model.apply(r), P @ r, rtol=0, atol=1e-12 * abs(P @ r).max())


def _notebook_system(oracle, n):
    MP = M.notebook(p=3, n=n)
    fixed = M.fixed_dofs(MP, M.NOTEBOOK_DIRICHLET)
    okv = oracle.make_knots(3, 0.0, 1.0, n)
    # stiffness is invariant under the rotations and translations that place the patches
    geos = [oracle.geo_quarter_annulus(), oracle.geo_unit_cube(2), oracle.geo_quarter_annulus(), oracle.geo_quarter_annulus()]
    A = None
    for p in range(4):
        X = MP.patch_to_global(p)
        T = X @ oracle.assemble('stiffness', (okv, okv), geos[p]) @ X.T
        A = T if A is None else A + T
    return MP, fixed, scipy.sparse.csr_matrix(A)


def test_schwarz_halves_jacobi_iterations_in_the_model(oracle):
    """The bound the device test takes: on the notebook domain at p = 3, n = 64 CG with the Schwarz model needs at most half the
    iterations of CG with Jacobi (measured here: 164 against 374 for a random right-hand side)."""
    MP, fixed, A = _notebook_system(oracle, 64)
    shapes, maps, boxes, U, lam, mode = _factors(MP, fixed, 'stiffness', oracle)
    model = M.SchwarzModel(MP.numdofs, shapes, maps, fixed, boxes, U, lam, mode)
    free = model.free
    Aff = A[free][:, free]
    b = np.random.default_rng(0).standard_normal(Aff.shape[0])

    def schwarz(r):
        z = np.zeros(MP.numdofs)
        z[free] = r
        return model.apply(z)[free]
    d = Aff.diagonal()
    it_j, _, info_j = M.cg_iterations(Aff, b, lambda r: r / d, 1e-8)
    it_s, _, info_s = M.cg_iterations(Aff, b, schwarz, 1e-8)
    assert info_j == 0 and info_s == 0
    assert 2 * it_s <= it_j, (it_s, it_j)


def test_new_abi_names_declared_bound_exported():
    hdr = open(os.path.join(ROOT, 'include', 'igx.h')).read()
    declared = set(re.findall(r'\b(igx_[a-z_0-9]+)\s*\(', hdr))
    bound = {name for name, _, _ in _lib.SYMBOLS}
    nm = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in NEW_NAMES:
        assert name in declared and name in bound, name
        assert re.search(r'\bT %s\b' % name, nm), name
    assert _lib.IGX_PRECOND_SCHWARZ == 3 and 'schwarz' in _lib.MP_PRECONDS and 'schwarz' not in _lib.PRECONDS
    assert 'kron' not in _lib.MP_PRECONDS


def test_multipatch_system_fails_loudly_without_gpu():
    code = ('import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n'
            'import numpy as np, scipy.sparse.linalg\n'
            'def _no(*a, **k):\n'
            '    raise AssertionError("host solver called")\n'
            'scipy.sparse.linalg.cg = scipy.sparse.linalg.spsolve = _no\n'
            'import pyiga_amd\n'
            'from pyiga_amd import solvers\n'
            'import _mpsolve_model as M\n'
            'MP = M.lshape(p=2, n=4)\n'
            'try:\n'
            '    S = solvers.MultipatchSystem(MP, "inner(grad(u),grad(v))*dx", "v*dx")\n'
            '    S.solve()\n'
            '    print("COMPUTED")\n'
            'except pyiga_amd._lib.IgxError as e:\n'
            '    print("RAISED", e)\n' % (ROOT, os.path.dirname(os.path.abspath(__file__))))
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1')
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, env=env)
    assert 'RAISED' in out.stdout and 'COMPUTED' not in out.stdout, out.stdout + out.stderr
    assert 'host solver called' not in out.stdout + out.stderr

"""The multigrid kernels of pyiga_amd/csrc/multigrid.hip at every group width, on both sweep paths, past one pass of the colour
grid, on anisotropic transfers and at every size class of the dense inverse, each against a plain long-double reference of the
same operation (the cases and their bounds: tests/_mg_cases.py; tests/test_mg_coverage_cpu.py checks what they reach).

The reference is always computed on the host from the matrices the device assembled, downloaded (S.mg_level(l).matrix()): the
assembly is checked elsewhere, these tests isolate the kernels.  Every figure is printed before it is asserted.
- Relax (k_csr_gs, k_csr_gs_block): forward, backward and symmetric sweeps against Gauss-Seidel in colour order in long double.
- Transfers (k_mg_transfer): prolongation and restriction of every level pair against the global prolongation applied in long
  double, and the adjoint identity <P xc, rf> = <xc, P^T rf> to rounding.
- Dense apply (k_dense_apply): against the symmetrised inverse set_multigrid uploads, row by row.
- The V-cycle against the numpy model (tests/_mg_model.py), and its symmetry, on the 3D anisotropic case and at GW 64."""
import time

import numpy as np
import pytest
import scipy.linalg

from pyiga_amd import solvers

import _mg_cases as mc
import _mg_model as G
import _solver_cases as sc

pytestmark = pytest.mark.gpu

STIFF = 'inner(grad(u),grad(v))*dx'
PATHS = {'per_colour': 0, 'one_block': 1 << 30}
LD = np.longdouble


def f_one(*x):
    return 1.0 + 0.0 * x[0]


def _system(MP, sides, **mg):
    fixed = mc.fixed_dofs(MP, sides)
    S = solvers.MultipatchSystem(MP, STIFF, 'f*v*dx', bcs=(fixed, np.zeros(fixed.size)), f=f_one)
    if mg:
        S.set_multigrid(**mg)
    return S, fixed


def _colours(S, level=0):
    """The rows of every colour of `level`, from the host colouring of the downloaded pattern; their concatenation is the order
    the device sweeps in."""
    L = S.mg_level(level)
    A = L.matrix()
    free = np.ones(L.n, dtype=bool)
    free[L.bc_indices] = False
    colour, nc = solvers.first_fit_colouring(A.indptr, A.indices, free)
    lists = mc.colour_lists(colour)
    assert nc == S.mg_info()[level]['colours'] and np.array_equal(np.concatenate(lists), S.mg_colour_order(level))
    return A, lists


def _close(S):
    MP = S.MP
    S.close()
    MP.close()


# ---------------------------------------------------------------------------------------------
# the sweeps
@pytest.mark.parametrize('path', sorted(PATHS))
@pytest.mark.parametrize('case', mc.GS_CASES, ids=[c.id for c in mc.GS_CASES])
def test_relax_at_every_width(case, path):
    S, fixed = _system(case.build(), case.sides, levels=2, block_rows=PATHS[path])
    try:
        info = S.mg_info()
        assert info[0]['one_block'] == (path == 'one_block') and len(info) == 2
        A, lists = _colours(S)
        assert sc.spmv_gw(sc.max_row(A)) == case.gw and info[0]['colours'] == case.colours, (sc.max_row(A), info[0]['colours'])
        ref = mc.ColourSweep(A, lists)
        x0, b = mc.relax_inputs(case.id, S.n, fixed)
        for sweep in ('forward', 'backward', 'symmetric'):
            x = S.relax(x0, b, sweep=sweep)
            want = ref.sweep(x0, b, sweep)
            d = mc.relmax(x, want)
            print('relax', case.id, path, sweep, 'gw', case.gw, 'colours', info[0]['colours'], 'largest colour',
                  max(len(r) for r in lists), 'rel. difference %.2e' % d)
            assert d <= mc.RELAX_BOUND, (case.id, path, sweep, d)
            assert not x[fixed].any()
        # the values at the fixed dofs of the start vector and of b are not read
        x1, b1 = x0.copy(), b.copy()
        x1[fixed], b1[fixed] = 7.0, -3.0
        assert np.array_equal(S.relax(x1, b1, sweep='symmetric'), x)
    finally:
        _close(S)


def test_relax_past_one_pass_of_the_colour_grid():
    """lshape p = 1, n = 1024: the largest colour has more rows than NB_GS_MAX blocks of BLOCK / 4 row groups hold, so the
    grid-stride loop of k_csr_gs takes a second pass.  Per colour only (the level is far past block_rows)."""
    case = mc.GS_BIG_CASE
    t0 = time.perf_counter()
    S, fixed = _system(case.build(), case.sides)
    try:
        S.set_multigrid()
        info = S.mg_info()
        t1 = time.perf_counter()
        assert not info[0]['one_block'] and info[-1]['dense_inverse'] and info[-1]['spans'][0] == (16, 16)
        A, lists = _colours(S)
        largest = max(len(r) for r in lists)
        print(case.id, 'dofs', S.n, 'nonzeros', A.nnz, 'levels', len(info), 'colours', len(lists), 'largest colour', largest,
              'one pass', mc.gs_pass_rows(case.gw), 'set-up %.1f s' % (t1 - t0))
        assert sc.spmv_gw(sc.max_row(A)) == case.gw and len(lists) == case.colours
        assert largest > mc.gs_pass_rows(case.gw)
        ref = mc.ColourSweep(A, lists)
        x0, b = mc.relax_inputs(case.id, S.n, fixed)
        for sweep in ('forward', 'backward'):
            x = S.relax(x0, b, sweep=sweep)
            d = mc.relmax(x, ref.sweep(x0, b, sweep))
            print('relax', case.id, sweep, 'rel. difference %.2e' % d)
            assert d <= mc.RELAX_BOUND, (sweep, d)
            assert not x[fixed].any()
    finally:
        _close(S)


# ---------------------------------------------------------------------------------------------
# the transfers
@pytest.mark.parametrize('case', mc.TRANSFER_CASES, ids=[c.id for c in mc.TRANSFER_CASES])
def test_transfers_on_anisotropic_patches(case):
    S, fixed = _system(case.make(), case.sides, levels=case.levels)
    try:
        assert len(S.mg_info()) == case.levels
        rng = np.random.default_rng(12)
        for level, want_MP in zip(range(case.levels - 1), case.hierarchy()[1:]):
            F, Cs = S.mg_level(level), S.mg_level(level + 1)
            assert Cs.n == want_MP.numdofs and [tuple(kv.numdofs for kv in k) for k, _ in Cs.MP.patches] == \
                [tuple(kv.numdofs for kv in k) for k, _ in want_MP.patches]
            Pl = mc._ld(G.global_prolongation(F.MP, Cs.MP)[0])
            ff, fc = np.ones(F.n, dtype=LD), np.ones(Cs.n, dtype=LD)
            ff[F.bc_indices] = 0
            fc[Cs.bc_indices] = 0
            assert F.bc_indices.size and Cs.bc_indices.size
            xc, rf = rng.standard_normal(Cs.n), rng.standard_normal(F.n)
            ref = ff * (Pl @ (fc * xc))
            y = S.prolong(xc, level)
            d = mc.relmax(y, ref)
            print('prolong', case.id, 'level', level, 'rel. difference %.2e' % d)
            assert d <= mc.TRANSFER_BOUND, (case.id, level, d)
            assert not y[F.bc_indices].any()
            ref = fc * (Pl.T @ (ff * rf))
            z = S.restrict(rf, level)
            d = mc.relmax(z, ref)
            print('restrict', case.id, 'level', level, 'rel. difference %.2e' % d)
            assert d <= mc.TRANSFER_BOUND, (case.id, level, d)
            assert not z[Cs.bc_indices].any()
            # the adjoint identity on the free dofs, both sides summed in long double from what the device returned
            a = (y.astype(LD) * (ff * rf)).sum()
            c = ((fc * xc) * z.astype(LD)).sum()
            terms = (np.abs(ff * rf) * (abs(Pl) @ np.abs(fc * xc))).sum()
            print('adjoint', case.id, 'level', level, '|<P xc, rf> - <xc, R rf>| = %.2e, 64 eps sum|terms| = %.2e'
                  % (abs(a - c), 64 * mc.EPS * terms))
            assert abs(a - c) <= 64 * mc.EPS * terms, (case.id, level)
    finally:
        _close(S)


# ---------------------------------------------------------------------------------------------
# the dense inverse
@pytest.mark.parametrize('case', mc.DENSE_CASES, ids=[c.id for c in mc.DENSE_CASES])
def test_dense_apply(case):
    S, fixed = _system(case.build(), case.sides, levels=1, coarse_max=8192)
    try:
        info = S.mg_info()
        assert len(info) == 1 and info[0]['dense_inverse']
        fr = np.setdiff1d(np.arange(S.n), fixed)
        m = fr.size
        assert case.lo < m <= case.hi and m % mc.BLOCK != 0 and info[0]['free'] == m
        inv = scipy.linalg.inv(S.matrix()[fr][:, fr].toarray())
        inv = np.ascontiguousarray(0.5 * (inv + inv.T))                    # what set_multigrid uploads
        r = np.random.default_rng(m).standard_normal(S.n)
        z = S.apply_precond(r, 'mg')
        invl = inv.astype(LD)
        ref = invl @ r[fr].astype(LD)
        bound = 64 * mc.EPS * (np.abs(invl) @ np.abs(r[fr]).astype(LD))
        err = np.abs(z[fr].astype(LD) - ref)
        print('dense apply', case.id, 'free dofs', m, 'largest error / bound %.2e' % float((err / bound).max()),
              'rel. difference %.2e' % mc.relmax(z[fr], ref))
        assert (err <= bound).all(), (case.id, int(np.count_nonzero(err > bound)))
        assert not z[fixed].any()
    finally:
        _close(S)


# ---------------------------------------------------------------------------------------------
# the V-cycle
def _vcycle_cases():
    aniso = next(c for c in mc.TRANSFER_CASES if '3d' in c.tags)
    gw64 = next(c for c in mc.GS_CASES if c.id == 'cubes2_p3_n4')
    return [(aniso.id, aniso.make, aniso.sides), (gw64.id, gw64.build, gw64.sides)]


@pytest.mark.parametrize('path', sorted(PATHS))
@pytest.mark.parametrize('name,make,sides', _vcycle_cases(), ids=[c[0] for c in _vcycle_cases()])
def test_vcycle_matches_the_model_and_is_symmetric(name, make, sides, path):
    S, fixed = _system(make(), sides, levels=2, block_rows=PATHS[path])
    try:
        info = S.mg_info()
        assert len(info) == 2 and info[0]['one_block'] == (path == 'one_block')
        levels = [S.mg_level(l) for l in range(2)]
        model = G.Model([L.matrix() for L in levels], [L.MP for L in levels], [L.bc_indices for L in levels],
                        smooth_steps=S._mg['smooth_steps'])
        rng = np.random.default_rng(13)
        x, y = rng.standard_normal(S.n), rng.standard_normal(S.n)
        Bx, By = S.apply_precond(x, 'mg'), S.apply_precond(y)
        ref = model.apply_full(x)
        d = mc.relmax(Bx, ref)
        print('V-cycle', name, path, 'colours', [i['colours'] for i in info], 'rel. difference to the model %.2e' % d)
        assert d <= mc.VCYCLE_BOUND
        assert not Bx[fixed].any()
        free = np.ones(S.n, dtype=bool)
        free[fixed] = False
        a, b = Bx[free] @ y[free], x[free] @ By[free]
        print('V-cycle', name, path, 'symmetry %.2e' % (abs(a - b) / abs(a)))
        assert abs(a - b) <= 1e-11 * abs(a)
    finally:
        _close(S)

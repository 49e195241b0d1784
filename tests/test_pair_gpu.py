"""Forms over two spline spaces through the public interface (``assemble.assemble`` with ``kvs=(kvs0, kvs1)`` and the space of
every function in `bfuns`) against the reference (tests/golden/golden_pair.npz, made by tests/golden/make_golden_pair.py), and
the reference's solve-stokes notebook run on this package.
"""
import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.linalg

from conftest import golden_csr, rel_maxdiff

from pyiga_amd import assemble, bspline, geometry

import _pair_cases as pc

pytestmark = pytest.mark.gpu

RTOL = 1e-12


def _geo(case):
    return geometry.quarter_annulus() if case.geo == 'quarter_annulus' else geometry.twisted_box()


@pytest.mark.parametrize('cid', [c.id for c in pc.CASES])
def test_forms_over_two_spaces_vs_reference(cid, golden):
    """Every golden matrix in both layouts at rel_maxdiff <= 1e-12, the pattern exactly; shapes, num_components, asm.kvs; picked
    entries / blocks of the assembler object."""
    g, case = golden('pair'), pc.BY_ID[cid]
    kvs, geo = case.kvs(bspline), _geo(case)
    for form in case.forms:
        args = case.args(form)
        ncu, ncv = form.bfuns[0][1], form.bfuns[1][1]
        for layout in form.layouts:
            A = assemble.assemble(form.form, kvs, bfuns=form.bfuns, geo=geo, layout=layout, **args)
            ref = golden_csr(g, '%s_%s_%s' % (cid, form.name, layout))
            assert A.shape == ref.shape == (ncv * case.shape[0], ncu * case.shape[1])
            err = rel_maxdiff(A, ref)
            print('%s %s %s: %.2e' % (cid, form.name, layout, err))
            assert err <= RTOL, (cid, form.name, layout, err)
            A = scipy.sparse.csr_matrix(A)
            A.sort_indices()
            assert np.array_equal(A.indptr, ref.indptr) and np.array_equal(A.indices, ref.indices)
        asm = assemble.instantiate_assembler(form.form, kvs, dict(args, geo=geo), form.bfuns)
        try:
            assert asm.arity == 2 and tuple(asm.num_components()) == (ncu, ncv)
            assert asm.kvs == kvs and asm.pair.shape == case.shape and asm.nqp == case.q() == asm.patch.nqp
            idx = g['%s_%s_idx' % (cid, form.name)]
            if ncu == ncv == 1:
                want = g['%s_%s_entries' % (cid, form.name)]
                got = asm.multi_entries(idx)
                assert asm.entry(int(idx[0, 0]), int(idx[0, 1])) == got[0]
            else:
                want = g['%s_%s_blocks' % (cid, form.name)]
                got = np.asarray(asm.multi_blocks(idx))
            assert got.shape == want.shape and abs(got - want).max() <= RTOL * abs(want).max(), (cid, form.name)
        finally:
            asm.pair.close()
            asm.patch.close()


def test_transposed_block(golden):
    """'p * div(v) * dx' over (kvs_p, kvs_u) is the transpose of 'div(u) * p * dx' over (kvs_u, kvs_p) at 1e-12."""
    a, t = pc.BY_ID['th2'], pc.BY_ID['th2t']
    geo = _geo(a)
    A = assemble.assemble(a.forms[0].form, a.kvs(bspline), bfuns=a.forms[0].bfuns, geo=geo)
    T = assemble.assemble(t.forms[0].form, t.kvs(bspline), bfuns=t.forms[0].bfuns, geo=geo)
    assert T.shape == A.shape[::-1] == (160, 30) and rel_maxdiff(T, A.T.tocsr()) <= RTOL


def test_both_functions_in_space_1_is_a_square_assembler():
    """Every function in one space: the form on that space alone, the result of the one-space call bit for bit."""
    case = pc.BY_ID['th2']
    ku, kp = case.kvs(bspline)
    geo = _geo(case)
    form = '(inner(grad(u), grad(v)) + u * v) * dx'
    A = assemble.assemble(form, (ku, kp), bfuns=[('u', 1, 1), ('v', 1, 1)], geo=geo)
    B = assemble.assemble(form, kp, bfuns=[('u', 1), ('v', 1)], geo=geo)
    assert A.shape == (30, 30) and np.array_equal(A.indices, B.indices) and np.array_equal(A.data, B.data)
    asm = assemble.instantiate_assembler(form, (ku, kp), dict(geo=geo), [('u', 1, 1), ('v', 1, 1)])
    assert asm.kvs == (kp, kp) and asm.pair is None
    asm.patch.close()


def test_one_space_forms_are_unchanged(golden):
    """A vector-valued form on ONE space ('div(u) * v * dx', `_VEC_FORMS['divp']` of tests/test_gpu_parity.py) gives the values
    it gave before forms over two spaces existed, bit for bit: golden_pair_onespace.npz holds the output of the commit before."""
    g = golden('pair_onespace')
    mk = bspline.make_knots
    kvs2 = (mk(2, 0., 1., 5), mk(3, 0., 1., 4))
    for layout in ('blocked', 'packed'):
        A = assemble.assemble('div(u) * v * dx', kvs2, geo=geometry.quarter_annulus(), bfuns=[('u', 2), ('v', 1)], layout=layout)
        ref = golden_csr(g, 'divp_' + layout)
        assert A.shape == ref.shape and np.array_equal(A.indptr, ref.indptr) and np.array_equal(A.indices, ref.indices)
        assert np.array_equal(A.data, ref.data), layout


def test_asym_1d_helpers_on_the_device(golden):
    g = golden('pair')
    kv1, kv2 = bspline.make_knots(3, 0., 1., 4, mult=2), bspline.make_knots(2, 0., 1., 4)
    for du in (0, 1):
        for dv in (0, 1):
            ref = g['asym_%d%d' % (du, dv)]
            A = assemble.bsp_mixed_deriv_biform_1d_asym(kv1, kv2, du, dv).toarray()
            assert A.shape == ref.shape and abs(A - ref).max() <= RTOL * abs(ref).max(), (du, dv)
    assert abs(assemble.bsp_mass_1d_asym(kv1, kv2).toarray() - g['asym_00']).max() <= RTOL * abs(g['asym_00']).max()
    assert abs(assemble.bsp_stiffness_1d_asym(kv1, kv2).toarray() - g['asym_11']).max() <= RTOL * abs(g['asym_11']).max()


def test_stokes_notebook(golden):
    """The cells of the reference's solve-stokes notebook at n_el = (6, 4), p = 3 (328 unknowns) on this package: both blocks
    assembled on the device, scipy.sparse.bmat, RestrictedLinearSystem, spsolve.  Accepted:
    max |u - u_gold| / max |u_gold| <= 10 * stokes_amp * 1e-12 -- stokes_amp (golden file; 30.2) is the largest relative change of
    u, over five seeded perturbations of the stored matrix values by 1 + 1e-13 N(0, 1), divided by 1e-13; the matrices are
    accepted at 1e-12, and the factor 10 covers the gap between five samples and the worst case."""
    g = golden('pair')
    amp = float(g['stokes_amp'])
    assert amp < 1e3
    geo = geometry.quarter_annulus()
    p, n_el = 3, (6, 4)
    kvs_u = tuple(bspline.make_knots(p, 0.0, 1.0, n, mult=2) for n in n_el)
    kvs_p = tuple(bspline.make_knots(p - 1, 0.0, 1.0, n, mult=1) for n in n_el)
    m_u = tuple(kv.numdofs for kv in kvs_u)
    m_p = tuple(kv.numdofs for kv in kvs_p)
    A_grad = assemble.assemble('inner(grad(u), grad(v)) * dx', kvs_u, bfuns=[('u', 2), ('v', 2)], geo=geo)
    A_div = assemble.assemble('div(u) * p * dx', (kvs_u, kvs_p), bfuns=[('u', 2, 0), ('p', 1, 1)], geo=geo)
    assert rel_maxdiff(A_grad, golden_csr(g, 'stokes_A_grad')) <= RTOL and rel_maxdiff(A_div, golden_csr(g, 'stokes_A_div')) <= RTOL
    A_stokes = scipy.sparse.bmat([[A_grad, A_div.T], [A_div, None]], format='csr')

    def g_lid(x, y):
        return (x * y * -y, x * y * x)

    def g_zero(x, y):
        return (0.0, 0.0)
    bcs = assemble.compute_dirichlet_bcs(kvs_u, geo, [('bottom', g_zero), ('top', g_zero), ('left', g_lid), ('right', g_zero)])
    N = np.prod(m_u)
    bcs = (np.append(bcs[0], 2 * N), np.append(bcs[1], 0.0))
    o, og = np.argsort(bcs[0], kind='stable'), np.argsort(g['stokes_bcs_idx'], kind='stable')      # (the same dofs; the order is free)
    assert np.array_equal(bcs[0][o], g['stokes_bcs_idx'][og])
    assert abs(bcs[1][o] - g['stokes_bcs_val'][og]).max() <= RTOL * abs(g['stokes_bcs_val']).max()
    LS = assemble.RestrictedLinearSystem(A_stokes, 0.0, bcs)
    u = LS.complete(scipy.sparse.linalg.spsolve(LS.A, LS.b))
    ref = g['stokes_u']
    err = abs(u - ref).max() / abs(ref).max()
    print('Stokes, 328 unknowns: max |u - u_gold| / max |u_gold| = %.2e (allowed %.2e, stokes_amp %.1f)' % (err, 10 * amp * 1e-12, amp))
    assert u.shape == ref.shape == (2 * N + np.prod(m_p),) and err <= 10 * amp * 1e-12
    # the last cells: velocity and pressure as spline functions, evaluated on a grid
    velocity = bspline.BSplineFunc(kvs_u, np.stack((u[:N].reshape(m_u), u[N:2 * N].reshape(m_u)), axis=-1))
    pressure = bspline.BSplineFunc(kvs_p, u[2 * N:].reshape(m_p))
    grid = (np.linspace(0, 1, 9),) * 2
    assert velocity.grid_eval(grid).shape == (9, 9, 2) and pressure.grid_eval(grid).shape == (9, 9)

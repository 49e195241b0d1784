#!/usr/bin/env python3
"""Golden Robin / Neumann boundary terms from the REAL reference (c-f-h/pyiga).

Build the unmodified reference outside the repository as the header of make_golden.py describes, then

    PYTHONPATH=/tmp/pyiga_oracle python3 tests/golden/make_golden_robin.py

Writes `tests/golden/golden_robin.npz`: inputs and outputs of the reference's public API only (assemble.assemble with
boundary=, boundary_dofs, stiffness / mass, inner_products, compute_dirichlet_bcs, Multipatch, RestrictedLinearSystem,
solvers.sdirk3 / crank_nicolson, approx.project_L2; no reference source).  A boundary term is what the reference does on the host:

    R = assemble(form, kvs, geo=geo, boundary=bd, **inputs);  dofs = boundary_dofs(kvs, bd, ravel=True)
    A[dofs[:, None], dofs] += R;  b[dofs] += assemble(load, kvs, geo=geo, boundary=bd, **inputs).ravel()

Per case (prefix_) the file holds the volume matrix `A0_*`, every face matrix `R<k>` (dense, face dofs x face dofs) with its
`R<k>_dofs`, the summed matrix `A_*`, the load vector `b` with the face loads, the Dirichlet dofs and values `bc_idx`, `bc_val`
and the `spsolve` solution `u` of the restricted system, completed.  Cases:
  robin2_   2D quarter annulus, p = 3, n = 8, stiffness; alpha = 1 + x on 'right', the constant 2 on 'top' (they share a corner
            dof), a load g on 'right', Dirichlet data on 'left'
  robin2n_  the same without any Dirichlet side (pure Robin)
  robin3_   3D quarter-annulus cylinder, p = (2, 2, 2), n = 4; matrix terms on 'front' (axis 0), 'top' (axis 1, a function
            coefficient) and 'right' (axis 2), a load on 'back', Dirichlet data on 'left'
  cd2_      the convection-diffusion form of make_golden_parabolic.py, alpha = 1 + x on 'right' with a load, Dirichlet on 'left'
  heat2_    M u' = b - (K + R) u, no Dirichlet dof, schemes sdirk3 and cn, 5 steps; driven as make_golden_parabolic.py drives the
            reference, with its self-checks (every stage starts above the Newton threshold; a direct numpy DIRK agrees to 1e-10)
  mp_       the L-shape of make_golden_mpvec.py (3 patches, p = 2, n = 4, joined in the same order): matrix terms on 'bottom' of
            patch 0 (its corner dof is shared with patch 1) and on 'right' of patch 2, a load on the former, Dirichlet data on
            'left' of patch 0; the terms are glued with the reference's patch_to_global
"""
import os

import numpy as np
import scipy.sparse
import scipy.sparse.linalg

import pyiga
from pyiga import approx, assemble, bspline, geometry, solvers, vform

pyiga.set_max_threads(1)
OUT = os.path.dirname(os.path.abspath(__file__))
G = {}
TAU = 2.0 ** -6
NSTEPS = 5
CD2_FORM = '(inner(diff_coeff*grad(u),grad(v))+inner((x[1],-x[0]),grad(u))*v)*dx'


def kappa2(x, y):
    return 0.2 + 0.1 * x * y


def alpha2(x, y):
    return 1.0 + x


def g2(x, y):
    return np.cos(x) * y + 0.5


def f2(x, y):
    return 5.0 * (1.0 + x * y)


def dir2(x, y):
    return 1.0 + 0.3 * x - 0.2 * y


def alpha3(x, y, z):
    return 1.0 + 0.5 * x + z


def g3(x, y, z):
    return np.sin(x) + y * z


def f3(x, y, z):
    return 3.0 * (1.0 + x - np.sin(z))


def dir3(x, y, z):
    return np.cos(x + 0.5 * y) + 0.3 * z


def put_csr(name, A):
    A = scipy.sparse.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    G[name + '_data'], G[name + '_indices'], G[name + '_indptr'], G[name + '_shape'] = A.data, A.indices, A.indptr, np.array(A.shape)


def face_terms(prefix, kvs, geo, terms, n, X=None, k0=0):
    """[E R E^T] and [E r] of the terms (bd, matrix form | None, load form | None, inputs), in order; X: patch_to_global.  They are
    added to the volume matrix and load one after the other (solve_case), so that an entry two faces reach is (a + r_1) + r_2."""
    RA, rb = [], []
    for k, (bd, mform, lform, inputs) in enumerate(terms):
        dofs = assemble.boundary_dofs(kvs, bd, ravel=True)
        N = int(np.prod([kv.numdofs for kv in kvs]))
        E = scipy.sparse.csr_matrix((np.ones(len(dofs)), (dofs, np.arange(len(dofs)))), shape=(N, len(dofs)))
        if X is not None:
            E = X @ E
        G['%sR%d_dofs' % (prefix, k0 + k)] = np.asarray(dofs)
        if mform is not None:
            R = scipy.sparse.csr_matrix(assemble.assemble(mform, kvs, geo=geo, boundary=bd, **inputs))
            assert R.shape == (len(dofs), len(dofs)), R.shape
            G['%sR%d' % (prefix, k0 + k)] = R.toarray()
            RA.append((E @ R @ E.T).tocsr())
        if lform is not None:
            r = np.asarray(assemble.assemble(lform, kvs, geo=geo, boundary=bd, **inputs)).ravel()
            assert r.shape == (len(dofs),), r.shape
            G['%sr%d' % (prefix, k0 + k)] = r
            rb.append(E @ r)
    return RA, rb


def solve_case(prefix, A0, b0, RA, rb, bcs):
    A = scipy.sparse.csr_matrix(A0)
    for T in RA:
        A = (A + T).tocsr()
    b = b0.copy()
    for t in rb:
        b = b + t
    put_csr(prefix + 'A0', A0)
    put_csr(prefix + 'A', A)
    G[prefix + 'b0'], G[prefix + 'b'] = b0, b
    G[prefix + 'bc_idx'], G[prefix + 'bc_val'] = np.asarray(bcs[0], dtype=np.int64), np.asarray(bcs[1], dtype=np.float64)
    if len(bcs[0]):
        LS = assemble.RestrictedLinearSystem(A, b, bcs)
        u = LS.complete(scipy.sparse.linalg.spsolve(LS.A.tocsc(), LS.b))
    else:
        u = scipy.sparse.linalg.spsolve(A.tocsc(), b)
    G[prefix + 'u'] = np.asarray(u).ravel()
    print(prefix, 'n', A.shape[0], 'nnz', A.nnz, 'fixed', len(bcs[0]), '|u|max %.3f' % np.abs(u).max())
    return A, b


NOBC = (np.zeros(0, dtype=np.int64), np.zeros(0))

# ---- 2D Poisson with Robin sides
geo2 = geometry.quarter_annulus()
kvs2 = 2 * (bspline.make_knots(3, 0.0, 1.0, 8),)
n2 = int(np.prod([kv.numdofs for kv in kvs2]))
TERMS2 = [('right', 'alpha*u*v*ds', 'g*v*ds', dict(alpha=alpha2, g=g2)), ('top', '2.0*u*v*ds', None, {})]
K2 = assemble.stiffness(kvs2, geo2)
b2 = assemble.inner_products(kvs2, f2, f_physical=True, geo=geo2).ravel()
RA2, rb2 = face_terms('robin2_', kvs2, geo2, TERMS2, n2)
solve_case('robin2_', K2, b2, RA2, rb2, assemble.compute_dirichlet_bcs(kvs2, geo2, [('left', dir2)]))
RA2n, rb2n = face_terms('robin2n_', kvs2, geo2, TERMS2, n2)
solve_case('robin2n_', K2, b2, RA2n, rb2n, NOBC)

# ---- 3D: every orientation of a face
geo3 = geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.quarter_annulus())
kvs3 = 3 * (bspline.make_knots(2, 0.0, 1.0, 4),)
n3 = int(np.prod([kv.numdofs for kv in kvs3]))
TERMS3 = [('front', '1.5*u*v*ds', None, {}), ('top', 'alpha*u*v*ds', None, dict(alpha=alpha3)), ('right', '0.7*u*v*ds', None, {}),
          ('back', None, 'g*v*ds', dict(g=g3))]
RA3, rb3 = face_terms('robin3_', kvs3, geo3, TERMS3, n3)
solve_case('robin3_', assemble.stiffness(kvs3, geo3), assemble.inner_products(kvs3, f3, f_physical=True, geo=geo3).ravel(), RA3, rb3,
           assemble.compute_dirichlet_bcs(kvs3, geo3, [('left', dir3)]))

# ---- convection-diffusion with a Robin side (non-symmetric: BiCGStab on the device)
TERMSC = [('right', 'alpha*u*v*ds', 'g*v*ds', dict(alpha=alpha2, g=g2))]
RAc, rbc = face_terms('cd2_', kvs2, geo2, TERMSC, n2)
solve_case('cd2_', assemble.assemble(CD2_FORM, kvs2, geo=geo2, diff_coeff=kappa2), b2, RAc, rbc,
           assemble.compute_dirichlet_bcs(kvs2, geo2, [('left', dir2)]))


# ---- heat conduction with convective cooling: M u' = b - (K + R) u, no Dirichlet dof
def direct_dirk(A, M, K, b, x, tau, nsteps):
    """The DIRK of the system with dense solves; also the smallest absolute residual any stage starts with."""
    s = A.shape[1]
    F = lambda z: b - K @ z
    out, rmin = [x], np.inf
    Fx = None
    for _ in range(nsteps):
        ys, Fy = [], []
        for i in range(s):
            aii = A[i, i]
            if aii == 0:
                ys.append(x)
                Fy.append(Fx if Fx is not None else F(x))
                continue
            rhs = M @ x + tau * sum(A[i, j] * Fy[j] for j in range(i))
            z = x if i == 0 else ys[-1]
            rmin = min(rmin, np.linalg.norm(M @ z - tau * aii * F(z) - rhs))
            y = np.linalg.solve(M + tau * aii * K, rhs + tau * aii * b)
            ys.append(y)
            Fy.append(F(y))
        x, Fx = ys[-1], Fy[-1]
        out.append(x)
    return out, rmin


g3s = 0.43586652150845899942
bb2 = (6 * g3s * g3s - 20 * g3s + 5) / 4
SDIRK3 = np.array([[g3s, 0, 0], [(1 - g3s) / 2, g3s, 0], [1 - bb2 - g3s, bb2, g3s], [1 - bb2 - g3s, bb2, g3s]])
CN = np.array([[0, 0], [0.5, 0.5], [0.5, 0.5]])

RAh, rbh = face_terms('heat2_', kvs2, geo2, TERMS2, n2)
Kh = scipy.sparse.csr_matrix(K2)
for T in RAh:
    Kh = (Kh + T).tocsr()
Mh = scipy.sparse.csr_matrix(assemble.mass(kvs2, geo2))
bh0 = 4.0 * b2
bh = bh0.copy()
for t in rbh:
    bh = bh + t
u0 = approx.project_L2(kvs2, lambda x, y: np.sin(2 * x) * np.cos(y) + 0.5, f_physical=True, geo=geo2).ravel()
put_csr('heat2_A0', K2)
put_csr('heat2_A', Kh)
G['heat2_b0'], G['heat2_b'], G['heat2_u0'] = bh0, bh, u0
G['heat2_tau'], G['heat2_t_end'] = np.array(TAU), np.array(NSTEPS * TAU)
for name, method, A in (('sdirk3', solvers.sdirk3, SDIRK3), ('cn', solvers.crank_nicolson, CN)):
    times, sols = method(Mh, lambda x: bh - Kh @ x, lambda x: -Kh, u0, TAU, NSTEPS * TAU)
    assert len(sols) == NSTEPS + 1, (name, len(sols))
    ref, rmin = direct_dirk(A, Mh.toarray(), Kh.toarray(), bh, u0, TAU, NSTEPS)
    assert rmin > 1e-3, (name, 'a stage starts below the Newton threshold', rmin)
    err = max(np.abs(a - b).max() for a, b in zip(sols, ref)) / max(np.abs(b).max() for b in ref)
    assert err < 1e-10, (name, err)
    G['heat2_' + name + '_times'] = np.array(times)
    G['heat2_' + name + '_u'] = np.array([np.asarray(x).ravel() for x in sols])
    print('heat2_', name, 'steps', len(sols) - 1, 'min stage residual %.2e' % rmin, 'vs direct DIRK %.1e' % err)


# ---- multipatch: the L-shape of make_golden_mpvec.py
def lshape(p, n):
    kvs = 2 * (bspline.make_knots(p, 0.0, 1.0, n),)
    squ = geometry.unit_square()
    geos = (squ, squ.translate((1, 0)), squ.scale((-1, 1)).translate((2, 1)))
    MP = assemble.Multipatch([(kvs, g) for g in geos])
    MP.join_boundaries(0, 'right', 1, 'left')
    MP.join_boundaries(1, 'top', 2, 'bottom', flip=(True,))
    MP.finalize()
    return MP


def fmp(x, y):
    return 2.0 + np.sin(x) * y


MP = lshape(2, 4)
A0, b0 = MP.assemble_system(vform.stiffness_vf(2), vform.L2functional_vf(2, physical=True), f=fmp)
nd = MP.numdofs
MPTERMS = [(0, ('bottom', 'alpha*u*v*ds', 'g*v*ds', dict(alpha=alpha2, g=g2))), (2, ('right', '1.25*u*v*ds', None, {}))]
RAm, rbm = [], []
for k, (p, term) in enumerate(MPTERMS):
    kvs, geo = MP.patches[p]
    Rk, rk = face_terms('mp_', kvs, geo, [term], nd, X=MP.patch_to_global(p), k0=k)
    RAm, rbm = RAm + Rk, rbm + rk
    G['mp_R%d_patch' % k] = np.array(p)
for p in range(MP.numpatches):
    G['mp_p2g%d' % p] = MP.patch_to_global_idx(p)
bcm = MP.compute_dirichlet_bcs([(0, 'left', dir2)])
solve_case('mp_', A0, np.asarray(b0).ravel(), RAm, rbm, bcm)

path = os.path.join(OUT, 'golden_robin.npz')
np.savez_compressed(path, **G)
print('wrote', path, os.path.getsize(path), 'bytes')

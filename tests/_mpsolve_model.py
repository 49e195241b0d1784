"""Host-side pieces shared by the multipatch solver tests: domains joined by hand (no interface detection, so no device is
needed to number them), their Dirichlet dofs, and a numpy model of the additive Schwarz preconditioner
z = sum_p X_p M_p B_p M_p X_p^T r  with the per-patch fast-diagonalization inverses B_p built from np.kron factors."""
import numpy as np

from pyiga_amd import assemble, bspline, geometry

NOTEBOOK_DIRICHLET = [(0, 'bottom'), (0, 'right'), (1, 'top'), (2, 'left'), (2, 'bottom'), (3, 'bottom')]


def notebook(p=3, n=15):
    """The domain of the reference's multipatch notebook, joined as interface detection joins it."""
    kvs = 2 * (bspline.make_knots(p, 0.0, 1.0, n),)
    geos = [geometry.quarter_annulus(),
            geometry.unit_square().translate((-1, 1)),
            geometry.quarter_annulus().rotate_2d(np.pi).translate((-1, 3)),
            geometry.quarter_annulus().rotate_2d(-np.pi / 2).translate((-2, 1))]
    MP = assemble.Multipatch([(kvs, g) for g in geos])
    MP.join_boundaries(0, (0, 1), 1, (1, 1), flip=(False,))
    MP.join_boundaries(1, (1, 0), 2, (0, 1), flip=(True,))
    MP.join_boundaries(1, (0, 0), 3, (0, 1), flip=(False,))
    MP.finalize()
    return MP


def lshape(p=2, n=8):
    kvs = 2 * (bspline.make_knots(p, 0.0, 1.0, n),)
    squ = geometry.unit_square()
    geos = (squ, squ.translate((1, 0)), squ.scale((-1, 1)).translate((2, 1)))
    MP = assemble.Multipatch([(kvs, g) for g in geos])
    MP.join_boundaries(0, 'right', 1, 'left')
    MP.join_boundaries(1, 'top', 2, 'bottom', flip=(True,))
    MP.finalize()
    return MP


def three_cubes(p=2, n=4):
    """Three unit cubes along the edge x = 1, y = 1, the third mirrored in x so that its joins need flips (interface
    detection: needs the device)."""
    kvs = 3 * (bspline.make_knots(p, 0.0, 1.0, n),)
    cube = geometry.unit_cube()
    geos = [cube, cube.translate((1, 0, 0)), cube.scale((-1, 1, 1)).translate((1, 1, 0))]
    return assemble.Multipatch([(kvs, g) for g in geos], automatch=True)


def fixed_dofs(MP, sides):
    """Global indices of the dofs on the sides ``[(patch, bdspec), ...]``, sorted and unique."""
    out = [MP.patch_to_global_idx(p)[assemble.boundary_dofs(MP.patches[p][0], bd, ravel=True)] for p, bd in sides]
    return np.unique(np.concatenate(out)) if out else np.zeros(0, dtype=np.int64)


def shapes_maps(MP):
    shapes = [tuple(kv.numdofs for kv in kvs) for kvs, _ in MP.patches]
    return shapes, [MP.patch_to_global_idx(p) for p in range(MP.numpatches)]


def mats1d_oracle(orc, kind='stiffness'):
    """(K, M) of a knot vector from the oracle's 1D forms (host only)."""
    def mats(kv):
        okv = orc.KnotVector(kv.kv, kv.p)
        K = orc.bsp_mixed_deriv_biform_1d(okv, 1, 1) if kind == 'stiffness' else None
        return K, orc.bsp_mixed_deriv_biform_1d(okv, 0, 0)
    return mats


class SchwarzModel:
    """The Schwarz operator in numpy: per patch, gather the box of the free part of r, apply
    (x)U_k . D^-1 . (x)U_k^T with D the sum (IGX_KRON_SUM) or product of the lam_k, add back on the free dofs."""

    def __init__(self, nglobal, shapes, maps, fixed, boxes, U, lam, mode):
        self.n = int(nglobal)
        self.free = np.ones(self.n, dtype=bool)
        self.free[np.asarray(fixed, dtype=np.int64)] = False
        self.parts = []
        for shape, l2g, (lo, hi), Up, Lp in zip(shapes, maps, boxes, U, lam):
            nb = tuple(b - a for a, b in zip(lo, hi))
            if min(nb) <= 0:
                continue
            grids = np.meshgrid(*[np.arange(a, b) for a, b in zip(lo, hi)], indexing='ij')
            g = np.asarray(l2g)[np.ravel_multi_index([x.ravel() for x in grids], shape)]
            D = Lp[0]
            for l in Lp[1:]:
                D = np.add.outer(D, l) if mode == 1 else np.multiply.outer(D, l)
            self.parts.append((g, nb, Up, D))

    def apply(self, r):
        r = np.where(self.free, r, 0.0)
        z = np.zeros(self.n)
        for g, nb, Up, D in self.parts:
            x = r[g].reshape(nb)
            for k, u in enumerate(Up):
                x = np.moveaxis(np.tensordot(u.T, x, axes=(1, k)), 0, k)
            x = x / D
            for k, u in enumerate(Up):
                x = np.moveaxis(np.tensordot(u, x, axes=(1, k)), 0, k)
            z[g] += x.ravel()
        return np.where(self.free, z, 0.0)

    def dense(self):
        """The matrix on all global dofs (zero rows and columns at the fixed dofs)."""
        P = np.zeros((self.n, self.n))
        for g, nb, Up, D in self.parts:
            K = Up[0]
            for u in Up[1:]:
                K = np.kron(K, u)
            B = K @ np.diag(1.0 / D.ravel()) @ K.T
            m = self.free[g]
            P[np.ix_(g[m], g[m])] += B[np.ix_(m, m)]
        return P


def cg_iterations(A, b, M, tol, maxiter=2000):
    """Iterations scipy's CG takes to ||r|| <= tol ||b|| from x0 = 0 with preconditioner M (a callable or None)."""
    import scipy.sparse.linalg as sla
    count = [0]

    def cb(xk):
        count[0] += 1
    Mop = None if M is None else sla.LinearOperator(A.shape, matvec=M, dtype=np.float64)
    x, info = sla.cg(A, b, rtol=tol, atol=0.0, maxiter=maxiter, M=Mop, callback=cb)
    return count[0], x, info

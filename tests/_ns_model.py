"""Host model of the device Navier-Stokes solver (solvers.NavierStokesSystem): plain NumPy / SciPy and the
oracle, no GPU, no library load.

* the wind and its physical gradient at the Gauss nodes by dense collocation (as tests/test_spline_eval_gpu.py builds its
  collocation matrices) and the geometry Jacobian of the oracle;
* the table rule of the device: the convection term ``grad(u).dot(w).dot(v)`` adds ``P[0][1 + j] = w_j`` to block (p, p), the
  Newton term ``grad(w).dot(u).dot(v)`` adds ``P[0][0] = d w_p / d x_q`` to block (p, q); the matrices of these tables by the
  oracle's entry sums;
* Picard and Newton in correction form with the bookkeeping of solvers.newton_loop, the linear solves either exact (spsolve) or
  by the GMRES model of the device (_gmres_model.py: triangular Kronecker preconditioner, restart 128) stopped at `lin_tol`.

T is the tolerance of the device tests on every iterate, relative to max|u| of the golden iterate: 10 times the largest deviation
between the run with every linear solve (the Stokes start included) stopped at lin_tol = 1e-10 and the run with exact solves,
over the four golden runs; the factor 10 allows for the device's different summation order.  tests/test_ns_cpu.py measures the
deviation again and asserts that the numbers below are what it finds.
"""
import numpy as np
import scipy.sparse
import scipy.sparse.linalg

import _gmres_model as gm
import _saddle_cases as sc

CASES = ('ns2', 'ns3')
BASE = {'ns2': 'stokes', 'ns3': 'stokes3'}
METHODS = ('picard', 'newton')
GOLDEN_STEPS = {('ns2', 'picard'): 7, ('ns2', 'newton'): 3, ('ns3', 'picard'): 25, ('ns3', 'newton'): 4}
RTOL = 1e-10                    # the stop of the golden runs: ||R F|| < RTOL ||R F(x0)||
LIN_TOL = 1e-10
RESTART = 128

# measured by test_ns_cpu.py::test_tolerance_of_the_device_runs (python3 tests/test_ns_cpu.py prints them): the largest deviation
# of an iterate of the inexact run from the exact one, relative to max|u|, per (case, method)
# (on ns2 the largest is the Stokes start's: GMRES stops on the 2-norm of the residual, 2.0e-10 on `stokes` at tol 1e-12 already)
MEASURED_DEVIATION = {
    ('ns2', 'picard'): 5.65e-10,
    ('ns2', 'newton'): 5.65e-10,
    ('ns3', 'picard'): 4.95e-11,
    ('ns3', 'newton'): 4.51e-11,
}
T = 10 * 5.65e-10


def golden_wind_file(name, tag):
    """The golden file that holds A_conv / A_newt of case `name` at wind `tag` ('stokes', 'rand')."""
    return 'ns' if name == 'ns2' else 'ns3_' + tag


def conv_tables(w, nc):
    """The table rule of the convection term for the wind components `w` (dim arrays): ``tables[p][q]`` a 4x4 table, None for
    an absent block -- block (p, p) holds ``P[0][1 + j] = w_j``."""
    out = [[None] * nc for _ in range(nc)]
    for p in range(nc):
        t = [[None] * 4 for _ in range(4)]
        for j in range(len(w)):
            t[0][1 + j] = w[j]
        out[p][p] = t
    return out


def newt_tables(dw, nc):
    """... of the Newton term for ``dw[p][q] = d w_p / d x_q``: block (p, q) holds ``P[0][0] = dw[p][q]``."""
    out = [[None] * nc for _ in range(nc)]
    for p in range(nc):
        for q in range(nc):
            t = [[None] * 4 for _ in range(4)]
            t[0][0] = dw[p][q]
            out[p][q] = t
    return out


class Case:
    """A golden case with the oracle's knot vectors and geometry."""

    def __init__(self, golden, orc, name):
        g = golden('ns')
        self.name, self.g, self.orc = name, g, orc
        self.spaces = sc.system(golden, BASE[name]).spaces
        self.kvs_u, self.kvs_p = [[orc.make_knots(p, 0.0, 1.0, n, mult=m) for p, n, m in sp] for sp in self.spaces]
        self.geo = orc.geo_quarter_annulus() if name == 'ns2' else orc.geo_twisted_box()
        self.nc = self.dim = len(self.kvs_u)
        self.ndofs = tuple(kv.numdofs for kv in self.kvs_u)
        self.N = int(np.prod(self.ndofs))
        self.nv = self.nc * self.N
        self.A_grad, self.B = sc.golden_csr(g, name + '_A_grad'), sc.golden_csr(g, name + '_A_div')
        self.n = self.nv + self.B.shape[0]
        self.bcs = (np.asarray(g[name + '_bcs_idx'], dtype=np.int64), np.asarray(g[name + '_bcs_val'], dtype=np.float64))
        self.nu = float(g[name + '_nu'])
        self.free = np.ones(self.n, dtype=bool)
        self.free[self.bcs[0]] = False
        nqp = max(kv.p for kv in self.kvs_u) + 1
        self.grid, self.gw = orc.make_tensor_quadrature([kv.mesh for kv in self.kvs_u], nqp)
        self.JI = np.linalg.inv(orc.grid_jacobian(self.geo, self.grid))          # [param (x, y, z order)][physical]
        self._P = None

    def iterates(self, method):
        return np.asarray(self.g['%s_%s_iterates' % (self.name, method)]), np.asarray(self.g['%s_%s_norms' % (self.name, method)])

    def golden_matrix(self, golden, which, tag):
        return sc.golden_csr(golden(golden_wind_file(self.name, tag)), '%s_A_%s_%s' % (self.name, which, tag))

    def random_wind(self, golden):
        return np.asarray(golden(golden_wind_file(self.name, 'rand'))[self.name + '_w_rand'])

    # -- the wind at the Gauss nodes
    def coefficients(self, x):
        return np.stack([x[c * self.N:(c + 1) * self.N].reshape(self.ndofs) for c in range(self.nc)], axis=-1)

    def wind_fields(self, x):
        """(w, dw): w[j] the component j, dw[p][q] = d w_p / d x_q (physical), arrays over the Gauss grid."""
        U = self.coefficients(np.asarray(x)[:self.nv])
        val = self.orc.bspline_grid_eval(self.kvs_u, U, self.grid)                # G + (nc,)
        par = self.orc.bspline_grid_jacobian(self.kvs_u, U, self.grid)            # G + (nc, dim): parametric, (x, y, z) order
        phys = np.einsum('...pc,...cr->...pr', par, self.JI)
        return [val[..., j] for j in range(self.nc)], [[phys[..., p, q] for q in range(self.dim)] for p in range(self.nc)]

    def matrix(self, tables):
        blocks = [[None if t is None else self.orc.assemble_nonsymmetric('form', self.kvs_u, self.geo, table=t) for t in row]
                  for row in tables]
        zero = scipy.sparse.csr_matrix((self.N, self.N))
        return scipy.sparse.bmat([[zero if b is None else b for b in row] for row in blocks], format='csr')

    def conv(self, x):
        return self.matrix(conv_tables(self.wind_fields(x)[0], self.nc))

    def newt(self, x):
        return self.matrix(newt_tables(self.wind_fields(x)[1], self.nc))

    # -- the linear solves
    def saddle(self, A):
        return scipy.sparse.bmat([[A, self.B.T], [self.B, None]], format='csr')

    def preconditioner(self):
        if self._P is None:
            self._P = sc.model_preconditioner(self, self.free, self.orc, viscosity=self.nu)
        return self._P

    def solve_exact(self, A, r, bcs_values=None):
        """K^-1 r on the free dofs with the fixed ones at `bcs_values` (default zero)."""
        K = self.saddle(A)
        g = np.zeros(self.n)
        if bcs_values is not None:
            g[self.bcs[0]] = bcs_values
        f = self.free
        rhs = (r - K @ g)[f]
        x = g.copy()
        x[f] = scipy.sparse.linalg.spsolve(K[f][:, f].tocsc(), rhs)
        return x, None

    def solve_model(self, A, r, bcs_values=None, lin_tol=LIN_TOL):
        vals = np.zeros_like(self.bcs[1]) if bcs_values is None else bcs_values
        x, info = gm.solve(A, self.B, self.nc, (self.bcs[0], vals), b=r, P=self.preconditioner(), tol=lin_tol, maxiter=1000,
                           restart=RESTART, triangular=True)
        return x, info

    def stokes(self, solve):
        return solve(self.nu * self.A_grad, np.zeros(self.n), self.bcs[1])

    def run(self, method, x0, solve, atol=0.0, rtol=RTOL, maxiter=50, picard_steps=0):
        """The loop of solvers.newton_loop on host matrices.  Returns (iterates, info): info as the device's, `solves` the
        infos of the linear solves."""
        x = np.array(x0, dtype=np.float64)
        iterates, norms, solves, blocks = [x.copy()], [], [], 0

        def residual():
            Ap = self.nu * self.A_grad + self.conv(x)
            r = np.where(self.free, -(self.saddle(Ap) @ x), 0.0)
            return Ap, r
        Ap, r = residual()
        blocks += self.nc
        norms.append(float(np.linalg.norm(r)))
        target = max(atol, rtol * norms[0])
        converged = False
        for it in range(maxiter):
            if norms[-1] < target:
                converged = True
                break
            A = Ap
            if method == 'newton' and it >= picard_steps:
                A = Ap + self.newt(x)
                blocks += self.nc * self.nc
            dx, info = solve(A, r)
            solves.append(info)
            x = x + dx
            iterates.append(x.copy())
            Ap, r = residual()
            blocks += self.nc
            norms.append(float(np.linalg.norm(r)))
        return np.array(iterates), dict(iterations=len(iterates) - 1, residual_norms=norms, converged=converged, target=target,
                                        blocks_assembled=blocks, solves=solves)


def blocks_assembled(nc, method, steps, picard_steps=0):
    """What info['blocks_assembled'] of the device must be after `steps` steps: the diagonal blocks for every residual (steps + 1
    of them), all blocks for every Newton step."""
    newton = max(0, steps - picard_steps) if method == 'newton' else 0
    return nc * (steps + 1) + nc * nc * newton

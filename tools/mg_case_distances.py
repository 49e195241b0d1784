#!/usr/bin/env python3
"""How far the float64 host models lie from the long-double references on the inputs of tests/test_mg_kernels_gpu.py: the figures
written next to the cases of tests/_mg_cases.py, which decide whether a case keeps the project's bound (the rule is in that
module's docstring).  No GPU: the stiffness matrices are the oracle's (Kronecker sums on the unit squares and cubes, the
oracle's assembly on the notebook domain's annuli), summed over the patches on the host.

    python tools/mg_case_distances.py [--big]

--big adds lshape_p1_n1024 (3.15 M dofs: a few minutes, most of them in the sequential float64 sweep).
One line per case: the colours of the first-fit colouring under the case's fixed sides, the largest colour, and the distance."""
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import _mg_cases as mc                      # noqa: E402
import _mg_model as G                       # noqa: E402
from oracle import iga_oracle as orc        # noqa: E402
from pyiga_amd import solvers               # noqa: E402


def host_stiffness(MP, domain):
    A = None
    for q, (kvs, _) in enumerate(MP.patches):
        okvs = tuple(orc.KnotVector(kv.kv, kv.p) for kv in kvs)
        if domain == 'notebook' and q != 1:
            Aq = orc.assemble('stiffness', okvs, orc.geo_quarter_annulus())
        else:
            Aq = orc.kron_assemble('stiffness', okvs)
        X = MP.patch_to_global(q)
        T = X @ Aq @ X.T
        A = T if A is None else A + T
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A


def relax_distance(case, sweeps=('forward', 'backward', 'symmetric')):
    MP = case.build()
    A = host_stiffness(MP, case.domain)
    fixed = mc.fixed_dofs(MP, case.sides)
    free = np.ones(MP.numdofs, dtype=bool)
    free[fixed] = False
    colour, nc = solvers.first_fit_colouring(A.indptr, A.indices, free)
    lists = mc.colour_lists(colour)
    order = np.concatenate(lists)
    x0, b = mc.relax_inputs(case.id, MP.numdofs, fixed)
    ref = mc.ColourSweep(A, lists)
    dist = max(mc.relmax(G.gauss_seidel(A, x0, b, order, s), ref.sweep(x0, b, s)) for s in sweeps)
    print('relax    %-16s dofs %8d  gw %2d  colours %3d  largest colour %7d  distance %.2e  (bound %.0e)'
          % (case.id, MP.numdofs, mc.sc.spmv_gw(mc.sc.max_row(A)), nc, max(len(r) for r in lists), dist, mc.RELAX_BOUND))


def transfer_distance(case):
    MPs = case.hierarchy()
    dist = 0.0
    rng = np.random.default_rng(12)
    for F, Cs in zip(MPs[:-1], MPs[1:]):
        P, _, _ = G.global_prolongation(F, Cs)
        Pl = mc._ld(P)
        xc, rf = rng.standard_normal(Cs.numdofs), rng.standard_normal(F.numdofs)
        dist = max(dist, mc.relmax(P @ xc, Pl @ xc.astype(np.longdouble)), mc.relmax(P.T @ rf, Pl.T @ rf.astype(np.longdouble)))
    print('transfer %-16s dofs %s  distance %.2e  (bound %.0e)' % (case.id, [M.numdofs for M in MPs], dist, mc.TRANSFER_BOUND))


if __name__ == '__main__':
    orc.build()
    for case in mc.GS_CASES:
        relax_distance(case)
    for case in mc.TRANSFER_CASES:
        transfer_distance(case)
    if '--big' in sys.argv[1:]:
        relax_distance(mc.GS_BIG_CASE, sweeps=('forward', 'backward'))

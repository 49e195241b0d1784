#!/usr/bin/env python3
"""Records of the boundary terms, written to profiles/robin_timing.txt, one JSON line each:

  face_add   3D p = 3, 64^3 spans on the quarter-annulus cylinder: device time (igx_last_timing: events around the kernel) of
             k_face_add for one face of every orientation -- 'front' (axis 0: contiguous segments), 'top' (axis 1: runs) and
             'right' (axis 2: single values at a stride) -- with the face patch's mass matrix on the device, the best of `reps`
             adds, beside the device time of the stiffness assembly of the same patch and of the face patch's own assembly
  pure_robin iteration counts of the pure-Robin solve (no fixed dof) with the shifted Kronecker preconditioner and with Jacobi,
             PCG to 1e-8: the 2D golden case (quarter annulus, p = 3, n = 8), the same at n = 64, and the 3D cylinder p = 3, n = 32

These are records, not thresholds.  `--small` runs reduced sizes (a smoke run of the script itself)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pyiga_amd import assemblers, bspline, geometry, solvers  # noqa: E402
from pyiga_amd.form_assemblers import _identity_geo  # noqa: E402

OUT = os.path.join(ROOT, 'profiles', 'robin_timing.txt')


def cylinder():
    return geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.quarter_annulus())


def face_add(p, n, reps, emit):
    kvs = 3 * (bspline.make_knots(p, 0.0, 1.0, n),)
    vol = assemblers.DevicePatch(kvs, cylinder())
    try:
        vol.assemble('stiffness', to_host=False)                  # warm-up (tables, workspaces)
        vol.assemble('stiffness', to_host=False)
        asm_ms = vol.timing()['total_ms']
        emit({'record': 'assembly', 'p': p, 'spans': n, 'nnz': vol.nnz, 'stiffness_ms': round(asm_ms, 4)})
        for name, axis in (('front', 0), ('top', 1), ('right', 2)):
            tkvs = tuple(kv for k, kv in enumerate(kvs) if k != axis)
            face = assemblers.DevicePatch(tkvs, _identity_geo(tkvs), nqp=vol.nqp)
            try:
                face.assemble('mass', to_host=False)
                face.assemble('mass', to_host=False)
                face_ms = face.timing()['total_ms']
                best, wall = np.inf, np.inf
                for _ in range(reps):
                    t0 = time.perf_counter()
                    vol.add_face(axis, 1, face)
                    wall = min(wall, 1e3 * (time.perf_counter() - t0))
                    best = min(best, vol.timing()['total_ms'])
                emit({'record': 'face_add', 'side': name, 'axis': axis, 'face_nnz': face.nnz, 'k_face_add_ms': round(best, 4),
                      'call_wall_ms': round(wall, 4), 'face_assembly_ms': round(face_ms, 4), 'volume_assembly_ms': round(asm_ms, 4),
                      'add_over_assembly': round(best / asm_ms, 6)})
            finally:
                face.close()
    finally:
        vol.close()


def pure_robin(tag, kvs, geo, emit):
    d = len(kvs)
    if d == 2:
        terms = [solvers.BoundaryTerm('right', matrix='alpha*u*v*ds', rhs='g*v*ds', alpha=lambda x, y: 1.0 + x, g=lambda x, y: np.cos(x) * y + 0.5),
                 solvers.BoundaryTerm('top', matrix='2.0*u*v*ds')]
        f = lambda x, y: 5.0 * (1.0 + x * y)                      # noqa: E731
    else:
        terms = [solvers.BoundaryTerm('front', matrix='1.5*u*v*ds'),
                 solvers.BoundaryTerm('top', matrix='alpha*u*v*ds', alpha=lambda x, y, z: 1.0 + 0.5 * x + z),
                 solvers.BoundaryTerm('right', matrix='0.7*u*v*ds', rhs='g*v*ds', g=lambda x, y, z: np.sin(x) + y * z)]
        f = lambda x, y, z: 3.0 * (1.0 + x - np.sin(z))           # noqa: E731
    S = solvers.PatchSystem(kvs, geo, f, None, boundary_terms=terms)
    try:
        rec = {'record': 'pure_robin', 'case': tag, 'dofs': S.n, 'tol': 1e-8}
        sols = {}
        for precond in ('kron', 'jacobi'):
            sols[precond] = S.solve(tol=1e-8, maxiter=20000, precond=precond)
            rec[precond] = {'iterations': S.info['iterations'], 'converged': S.info['converged'], 'total_ms': round(S.info['total_ms'], 3)}
        rec['rel_diff_of_solutions'] = float(np.abs(sols['kron'] - sols['jacobi']).max() / np.abs(sols['jacobi']).max())
        emit(rec)
    finally:
        S.close()


def main():
    small = '--small' in sys.argv[1:]
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    face_add(3, 8 if small else 64, 3 if small else 10, emit)
    qa = geometry.quarter_annulus()
    pure_robin('2d_p3_n8', 2 * (bspline.make_knots(3, 0.0, 1.0, 8),), qa, emit)
    if not small:
        pure_robin('2d_p3_n64', 2 * (bspline.make_knots(3, 0.0, 1.0, 64),), qa, emit)
        pure_robin('3d_p3_n32', 3 * (bspline.make_knots(3, 0.0, 1.0, 32),), cylinder(), emit)
    if not small:
        with open(OUT, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

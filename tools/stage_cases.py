#!/usr/bin/env python3
"""The case table of the stage chain (tests/_stage_cases.py), one line per case: what stage_keys says the patch launches and
the shape quantities of its final kernel; with --time also the wall time of the CPU oracle on every case (8 threads).
No GPU needed."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import _stage_cases as st       # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('--time', action='store_true', help='run the oracle on every case and sweep size')
    args = ap.parse_args()
    if args.time:
        import test_stage_kernels_gpu as tg
    total = worst = 0.0
    for c in st.STAGE_CASES:
        k = st.stage_keys(c.axes, c.kind, c.knobs, c.table, c.geo)
        rows, nnz = st.patch_size(c.axes)
        line = '%-90s A %-32s B %-14s NTERM %-28s %s%s rows %d nnz %d%s' % (
            c.id, 'geoA' if k.stageA == 'geoA' else tuple(k.stageA), k.stageB and tuple(k.stageB), k.nterm and [n for _, n in k.nterm],
            k.final.kernel, k.final.args, rows, nnz, ' slabs' if c.slabs else '')
        if args.time:
            t = time.perf_counter()
            tg.oracle_matrix(c.axes, c.geo, c.kind, c.table)
            dt = time.perf_counter() - t
            total, worst = total + dt, max(worst, dt)
            line += ' oracle %.3f s' % dt
        print(line)
    if args.time:
        print('ledger: %.1f s, largest case %.2f s' % (total, worst))
        sweeps = 0.0
        for tag, axes, kind, knobs, table in st.sweep_patches():
            t = time.perf_counter()
            tg.oracle_matrix(axes, (st.GEOS_3D if len(axes) == 3 else st.GEOS_2D)[0], kind, table)
            sweeps += time.perf_counter() - t
        print('edge sweeps (%d sizes): %.1f s' % (len(st.sweep_patches()), sweeps))
    print('unreachable:')
    for key, why, _ in st.UNREACHABLE:
        print('  %s: %s' % (key, why))


if __name__ == '__main__':
    main()

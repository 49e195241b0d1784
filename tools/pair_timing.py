#!/usr/bin/env python3
"""Device time of the rectangular assembly over two spline spaces (`igx_pair_assemble`, csrc/pair.hip):
the scalar mass block 'u * p * dx' of a Taylor-Hood pair, velocity p = 3 with interior knots of multiplicity 2 against pressure
p = 2, on
  th2d  the quarter annulus, n = 256 spans per axis
  th3d  the quarter-annulus cylinder, n = 32 spans per axis
  th0   a small smoke case (printed only)
and beside it the kernel it was modelled on: the entry-wise `IGX_FORM` assembly (`IGX_ALGO_ENTRYWISE`, k_entries_csr, unchanged
by the pair code) of the SQUARE velocity-space patch of the same size with the same one-term table (P_00 = 1) and the same Gauss
rule.  Both are one thread per entry in the reference's summation order; the figure to compare is ns per entry (the entries of
the square matrix sum over the larger supports of two velocity functions).  Device events of the library (`igx_pair_last_timing`,
`igx_last_timing`), warm-up, then the median of REPS assemblies.  One JSON line per measurement, appended to
profiles/pair_timing.txt (`--out PATH`: elsewhere).  A record, not a threshold.

One case per process, each under its own time limit, the steps chained so that a failure ends the run:
  timeout -k 10 300 python tools/pair_timing.py th2d && timeout -k 10 600 python tools/pair_timing.py th3d
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyiga_amd import assemblers, bspline, geometry  # noqa: E402

REPS, WARMUP = 7, 2
CASES = {'th2d': (2, 256), 'th3d': (3, 32), 'th0': (2, 8)}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'pair_timing.txt')
    if '--out' in sys.argv:
        out = sys.argv[sys.argv.index('--out') + 1]
        args.remove(out)
    name = args[0] if args else 'th0'
    dim, n = CASES[name]
    ku = dim * (bspline.make_knots(3, 0.0, 1.0, n, mult=2),)
    kp = dim * (bspline.make_knots(2, 0.0, 1.0, n),)
    geo = geometry.quarter_annulus()
    if dim == 3:
        geo = geometry.tensor_product(geometry.line_segment(0.0, 1.0), geo)
    patch = assemblers.DevicePatch(ku, geo, nqp=4)
    pair = assemblers.DevicePair(patch, kp)
    one = [[None] * 4 for _ in range(4)]
    one[0][0] = np.ones(patch.resident_grid())
    patch.set_form(one)
    recs = []

    def measure(what, run, timing, entries, shape):
        ms = []
        for k in range(WARMUP + REPS):
            run()
            if k >= WARMUP:
                ms.append(timing()['entry_ms'])
        med = float(np.median(ms))
        recs.append({'case': name, 'what': what, 'shape': list(shape), 'entries': int(entries), 'kernel_ms_median': round(med, 4),
                     'kernel_ms_min': round(min(ms), 4), 'kernel_ms_max': round(max(ms), 4), 'ns_per_entry': round(med * 1e6 / entries, 4), 'reps': REPS})
        print(json.dumps(recs[-1]), flush=True)
    measure('igx_pair_assemble IGX_MASS (k_pair_entries_csr)', lambda: pair.assemble('mass'), pair.timing, pair.nnz, pair.shape)
    measure('igx_pair_assemble IGX_FORM, P_00 = 1 (k_pair_entries_csr)', lambda: pair.assemble('form'), pair.timing, pair.nnz, pair.shape)
    # (IGX_STAGE_EVENTS decides whether igx_assemble times its kernels apart; total_ms holds the field kernel too, so it is set)
    measure('igx_assemble IGX_FORM, P_00 = 1, IGX_ALGO_ENTRYWISE on the velocity patch (k_entries_csr)',
            lambda: patch.assemble('form', algo='entrywise', to_host=False), patch.timing, patch.nnz, patch.shape)
    pair.close()
    patch.close()
    if name != 'th0':
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, 'a') as f:
            for r in recs:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    if 'IGX_STAGE_EVENTS' not in os.environ:          # read when the patch is created: per-kernel events of igx_assemble
        os.environ['IGX_STAGE_EVENTS'] = '1'
    main()

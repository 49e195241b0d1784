#!/usr/bin/env python3
"""Times of the assembly over a hierarchical spline space (`pyiga_amd.hierarchical`, csrc/hier.hip):
stiffness on the B-spline quarter annulus, 2D p = 3, HB-splines with disparity 1, refined towards the diagonal with
`refine_region(lv, lambda *X: abs(X[0] - X[-1]) < 0.5 ** (lv + 1))` for lv = 0 .. L-1:

  diag32  base 32 x 32 spans, L = 4
  diag64  base 64 x 64 spans, L = 5
  diag8   base 8 x 8 spans, L = 2 (smoke case)

Per case: the host time to build the space, the host time of the index structures (pattern, positions, level layouts), the
set-up of the level assemblers with the upload of their index pairs, the device time of the level entries (`igx_entries_d`,
wall clock around the synchronised call), the upload of the tables and work items, the device time of the contraction from
events, and the download of the values.  A warm-up assembly, then the median of REPS.  `--thb` adds the THB variant of the
case: the same device work plus T' A T on the host, whose share is reported.

The reference (c-f-h/pyiga, unmodified, scipy triple products on the host) took 3.1 s (diag32) and 35.2 s (diag64) for the
same matrices -- measured ONCE, on ANOTHER machine (a CPU box without a GPU), with ONE thread; they are printed beside the
device figures as a landmark, not as a ratio anybody promised.

One JSON line per case on standard output; `--out PATH` also appends it to a file (profiles/hier_timing.txt was written that
way).  A record, not a threshold.

  timeout -k 10 300 python tools/bench_hier.py diag32 && timeout -k 10 600 python tools/bench_hier.py diag64
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyiga_amd import bspline, geometry  # noqa: E402
from pyiga_amd.hierarchical import HDiscretization, HSpace  # noqa: E402

REPS = 3
CASES = {'diag32': (32, 4, 3.1), 'diag64': (64, 5, 35.2), 'diag8': (8, 2, None)}
FORM = 'inner(grad(u),grad(v))*dx'


def build(n0, L, truncate):
    kv = bspline.make_knots(3, 0.0, 1.0, n0)
    hs = HSpace((kv, kv), truncate=truncate, disparity=1)
    for lv in range(L):
        hs.refine_region(lv, lambda *X: abs(X[0] - X[-1]) < 0.5 ** (lv + 1))
    return hs


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    out = None
    if '--out' in sys.argv:
        out = sys.argv[sys.argv.index('--out') + 1]
        args.remove(out)
    name = args[0] if args else 'diag8'
    n0, L, ref_s = CASES[name]
    geo = geometry.bspline_quarter_annulus()
    for truncate in ([False, True] if '--thb' in sys.argv else [False]):
        t0 = time.perf_counter()
        hs = build(n0, L, truncate)
        t_space = time.perf_counter() - t0
        runs = []
        for rep in range(1 + REPS):
            disc = HDiscretization(hs, FORM, {'geo': geo}, timed=True)           # (a new one every time: the plan is part of what is timed)
            t0 = time.perf_counter()
            A = disc.assemble_matrix()
            total = time.perf_counter() - t0
            disc.close()
            if rep:
                runs.append(dict(disc.timing, total_s=total))
        med = {k: float(np.median([r[k] for r in runs])) for k in runs[0] if k.endswith('_s')}
        rec = {'case': name, 'basis': 'THB' if truncate else 'HB', 'numdofs': hs.numdofs, 'numactive': list(hs.numactive), 'nnz': int(A.nnz),
               'hb_nnz': runs[0]['nnz'], 'level_entries': runs[0]['level_entries'], 'space_build_s': round(t_space, 4), 'reps': REPS}
        rec.update({k: round(v, 5) for k, v in med.items()})
        rec['contract_ns_per_value'] = round(med['contract_s'] * 1e9 / max(runs[0]['nnz'], 1), 3)
        if truncate:
            rec['thb_host_share'] = round(med['thb_host_s'] / med['total_s'], 3)
        if ref_s is not None and not truncate:
            rec['reference_cpu_s_other_machine_one_thread'] = ref_s
        print(json.dumps(rec), flush=True)
        if out is not None:
            with open(out, 'a') as fh:
                fh.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()

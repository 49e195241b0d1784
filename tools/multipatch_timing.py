#!/usr/bin/env python3
"""Times of the multipatch path: per-patch assembly, the one-time global pattern build (igx_multipatch_create) and the scatter of
each patch (igx_multipatch_scatter_patch), for the four-patch domain of the reference's notebooks/multipatch.ipynb at p = 3,
n = 256 and for two 3D p = 3 patches of 64^3 spans.  Host wall times around calls that end with a stream synchronisation;
run it under `rocprofv3 --kernel-trace --stats -- python3 tools/multipatch_timing.py` for the device times of k_scatter.
Prints one JSON line per case: the scatter bytes follow the layout of DESIGN.md section 11."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyiga_amd import assemble, bspline, geometry  # noqa: E402


def notebook(p, n):
    kvs = 2 * (bspline.make_knots(p, 0.0, 1.0, n),)
    geos = [geometry.quarter_annulus(), geometry.unit_square().translate((-1, 1)),
            geometry.quarter_annulus().rotate_2d(np.pi).translate((-1, 3)),
            geometry.quarter_annulus().rotate_2d(-np.pi / 2).translate((-2, 1))]
    return [(kvs, g) for g in geos]


def cylinders(p, n):
    kvs = 3 * (bspline.make_knots(p, 0.0, 1.0, n),)
    geo = geometry.tensor_product(geometry.line_segment(0.0, 1.0), geometry.bspline_quarter_annulus())
    return [(kvs, geo), (kvs, geo.scale((1, 1, -1)))]


def scatter_bytes(info, nrows_local):
    e = info['entries']
    # value read + value write (direct), + 4-byte position (store), + value read-back (read-add-write, atomic); 16-byte row plan
    return 16 * e['direct'] + 20 * e['store'] + 28 * (e['rmw'] + e['atomic']) + 16 * nrows_local


def run(name, patches, problem, rhs, reps, **kw):
    t0 = time.perf_counter()
    MP = assemble.Multipatch(patches, automatch=True)
    t_match = (time.perf_counter() - t0) * 1e3
    MP.pattern()
    pattern_ms = MP.timings['pattern_ms']
    res = []
    for _ in range(reps):
        A, b = MP.assemble_system(problem, rhs, **kw)
        res.append((list(MP.timings['assemble_ms']), list(MP.timings['scatter_ms'])))
    asm = np.min([r[0] for r in res], axis=0)
    sc = np.min([r[1] for r in res], axis=0)
    info = MP.info()
    nb = scatter_bytes(info, sum(MP.N))
    out = {'case': name, 'numdofs': MP.numdofs, 'nnz': info['nnz'], 'paths': [sorted(p) for p in MP.last_paths],
           'sources': MP.last_sources, 'automatch_ms': round(t_match, 1), 'pattern_build_ms': round(pattern_ms, 2),
           'assemble_ms_per_patch': [round(x, 3) for x in asm], 'scatter_ms_per_patch': [round(x, 3) for x in sc],
           'entries': info['entries'], 'scatter_bytes_total': nb,
           'scatter_GBps_host_timed': round(nb / (sc.sum() * 1e-3) / 1e9, 1)}
    print(json.dumps(out), flush=True)
    MP.close()


if __name__ == '__main__':
    reps = int(os.environ.get('MP_REPS', '3'))
    f2 = lambda x, y: np.exp(-5 * ((x - 0.3) ** 2 + (y - 1) ** 2))       # noqa: E731
    run('notebook_p3_n256', notebook(3, 256), 'inner(grad(u),grad(v))*dx', 'f*v*dx', reps, f=f2)
    f3 = lambda x, y, z: 1.0 + x * y                                     # noqa: E731
    run('cylinders3d_p3_n64', cylinders(3, 64), 'inner(grad(u),grad(v))*dx', 'f*v*dx', reps, f=f3)

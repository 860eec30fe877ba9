#!/usr/bin/env python3
"""Dense overlap registration (dsss_mosaic_register) of every frame pair with overlapping geo boxes of a synthetic survey, under three
trajectories: dead reckoning, the solved trajectory, the true poses.
    python tools/overlap_register.py --frames 200 --rows 2000 --cols 1024 --cell 0.1 [--radius 8] [--calls 7] [--timeout 900]
Per trajectory: pairs, usable pairs (a peak was found), pairs whose peak lies on the border of the search square, median and 95th
percentile of |offset| in metres over the usable pairs, median ZNCC at zero shift.  Times are wall clock around the synchronised call
under dead reckoning, median of --calls calls after one warm-up: the whole call, the same call at radius 0 (the mean layers plus a
correlation of ONE shift, (2 r + 1)^2 times less than the full one: "layers"), and their difference ("correlation").  evals = the sum
of n over all shifts and pairs, the cell-shift products the correlation accumulated.  Prints one JSON line.
The GPU work runs in a child process under a time limit (--timeout seconds); this process never opens the device."""
import argparse
import json
import os
import subprocess
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=200); ap.add_argument("--rows", type=int, default=2000)
ap.add_argument("--cols", type=int, default=1024); ap.add_argument("--cell", type=float, default=0.1)
ap.add_argument("--radius", type=int, default=8); ap.add_argument("--min-cells", type=int, default=256)
ap.add_argument("--calls", type=int, default=7); ap.add_argument("--timeout", type=float, default=900.0)
ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
a = ap.parse_args()
if a.calls < 5:
    sys.exit("--calls must be at least 5")

if not a.worker:
    try:
        sys.exit(subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"] + sys.argv[1:], timeout=a.timeout).returncode)
    except subprocess.TimeoutExpired:
        sys.exit("overlap_register: the GPU step did not finish within %g s" % a.timeout)

import numpy as np                               # noqa: E402
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diasss_amd import capi                      # noqa: E402
from diasss_amd.pipeline import Pipeline         # noqa: E402
from diasss_amd.synth import Survey              # noqa: E402

F, N, M = a.frames, a.rows, a.cols
sv = Survey(F, N, M, seed=20240601 + 2, device="cuda:0")
raws = [sv.frame(f) for f in range(F)]
ins = [sv.inputs(f) for f in range(F)]
pipe = Pipeline(F, device=0)
pipe.run(raws, [i[0] for i in ins], [i[1] for i in ins], [i[2] for i in ins])
ctx = pipe.ctx
_, rpy, stats = ctx.posegraph_solve(F, F * N, want_rpy=True)
ids = np.arange(F, dtype=np.int32); off = ids * N
true = np.ascontiguousarray(np.concatenate(sv.poses_true))
p = capi.mosaic_grid(ctx.mosaic_bounds(ids), a.cell)              # one grid for every trajectory: the dead-reckoning extent
boxes = [ctx.mosaic_bounds([f]) for f in range(F)]
pairs = [(i, j) for i in range(F) for j in range(i + 1, F)
         if boxes[i][0] <= boxes[j][1] and boxes[j][0] <= boxes[i][1] and boxes[i][2] <= boxes[j][3] and boxes[j][2] <= boxes[i][3]]
reg = capi.RegParams(a.radius, a.min_cells)
res = dict(frames=F, rows=N, cols=M, cell=a.cell, grid=[p.W, p.H], radius=a.radius, min_cells=a.min_cells, pairs=len(pairs), calls=a.calls,
           lm_iterations=int(stats[0]))
if not pairs:
    print(json.dumps(res)); pipe.close(); sys.exit(0)


def timed(r):
    ctx.mosaic_register(ids, p, pairs, reg=r)
    ts = []
    for _ in range(a.calls):
        t0 = time.perf_counter(); ctx.mosaic_register(ids, p, pairs, reg=r); ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), 1e3 * float(min(ts))


ms_all, min_all = timed(reg)
ms_lay, min_lay = timed(capi.RegParams(0, a.min_cells))
for name, traj in (("dr", {}), ("solved", dict(rpy6=rpy, ping_off=off)), ("true", dict(rpy6=true, ping_off=off))):
    out, sums = ctx.mosaic_register(ids, p, pairs, reg=reg, want_sums=True, **traj)
    ok = out["zncc"] > -2.0
    d = np.hypot(out["off_x"][ok], out["off_y"][ok])
    res[name] = dict(usable=int(ok.sum()), on_border=int((out["on_border"][ok] != 0).sum()),
                     offset_median_m=float(np.median(d)) if ok.any() else None, offset_p95_m=float(np.percentile(d, 95)) if ok.any() else None,
                     zncc0_median=float(np.median(out["zncc0"][out["zncc0"] > -2.0])) if (out["zncc0"] > -2.0).any() else None,
                     zncc_peak_median=float(np.median(out["zncc"][ok])) if ok.any() else None)
    if name == "dr":
        evals = float(sums[..., 0].sum(dtype=np.float64))
ms_corr = ms_all - ms_lay
res.update(register_ms=round(ms_all, 3), register_ms_min=round(min_all, 3), layers_ms=round(ms_lay, 3), layers_ms_min=round(min_lay, 3),
           correlation_ms=round(ms_corr, 3), evals=evals, evals_per_s=evals / (ms_corr * 1e-3) if ms_corr > 0 else None)
print(json.dumps(res))
pipe.close()

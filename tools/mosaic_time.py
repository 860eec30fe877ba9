#!/usr/bin/env python3
"""Time of the georeferenced mosaic (dsss_mosaic_render) on a synthetic survey whose images are resident on the device, under the
dead-reckoning poses and under the solved trajectory, and the overlap-consistency score under dead-reckoning, optimised and true poses.
    python tools/mosaic_time.py --frames 200 --rows 2000 --cols 1024 --cell 0.1 [--calls 7]
Prints one JSON line.  Times are wall clock around the call, which ends with a synchronisation of the context's stream and downloads
nothing (download=False): median of --calls calls after one warm-up.  dropped_fraction counts the pixels the filter mask rejects and the
ones that fall outside the grid."""
import argparse
import json
import os
import sys
import time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diasss_amd import capi                      # noqa: E402
from diasss_amd.pipeline import Pipeline         # noqa: E402
from diasss_amd.synth import Survey              # noqa: E402

HBM_PEAK = 8.0e12                                # bytes / s, the roof of DESIGN.md section 4

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=200); ap.add_argument("--rows", type=int, default=2000)
ap.add_argument("--cols", type=int, default=1024); ap.add_argument("--cell", type=float, default=0.1)
ap.add_argument("--calls", type=int, default=7)
a = ap.parse_args()
F, N, M = a.frames, a.rows, a.cols
if a.calls < 5:
    sys.exit("--calls must be at least 5")

sv = Survey(F, N, M, seed=20240601 + 1, device="cuda:0")
raws = [sv.frame(f) for f in range(F)]
ins = [sv.inputs(f) for f in range(F)]
pipe = Pipeline(F, device=0)
pipe.run(raws, [i[0] for i in ins], [i[1] for i in ins], [i[2] for i in ins])
ctx = pipe.ctx
_, rpy, stats = ctx.posegraph_solve(F, F * N, want_rpy=True)
ids = np.arange(F, dtype=np.int32); off = ids * N
true = np.ascontiguousarray(np.concatenate(sv.poses_true))
p = capi.mosaic_grid(ctx.mosaic_bounds(ids), a.cell)              # one grid for every trajectory: the dead-reckoning extent
samples = F * N * M
cells = p.W * p.H


def timed(**traj):
    ctx.mosaic_render(ids, p, download=False, **traj)
    ts = []
    for _ in range(a.calls):
        t0 = time.perf_counter(); ctx.mosaic_render(ids, p, download=False, **traj); ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), 1e3 * float(min(ts))


ms_dr, min_dr = timed()
ms_opt, min_opt = timed(rpy6=rpy, ping_off=off)
_, cnt, _ = ctx.mosaic_render(ids, p)
kept = int(cnt.sum(dtype=np.int64))
# algorithmic bytes: image and mask read once, the 64-bit accumulators cleared and read back once by the check
bytes_total = 2.0 * samples + 16.0 * cells
res = dict(frames=F, rows=N, cols=M, cell=a.cell, grid=[p.W, p.H], samples=samples, calls=a.calls,
           render_ms_dr=round(ms_dr, 3), render_ms_dr_min=round(min_dr, 3), render_ms_solved=round(ms_opt, 3), render_ms_solved_min=round(min_opt, 3),
           samples_per_s_dr=samples / (ms_dr * 1e-3), dropped_fraction=1.0 - kept / samples, fullest_cell=int(cnt.max()),
           bytes_per_sample=bytes_total / samples, hbm_fraction_dr=bytes_total / (ms_dr * 1e-3) / HBM_PEAK, lm_iterations=int(stats[0]))
for name, traj in (("dr", {}), ("solved", dict(rpy6=rpy, ping_off=off)), ("true", dict(rpy6=true, ping_off=off))):
    t0 = time.perf_counter()
    nfr, _, _, score = ctx.mosaic_consistency(ids, p, **traj)
    res["score_" + name] = score
    res["consistency_s_" + name] = round(time.perf_counter() - t0, 3)
res["cells_seen_twice"] = int((nfr >= 2).sum())
print(json.dumps(res))
pipe.close()

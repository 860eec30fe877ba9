#!/usr/bin/env python3
"""Time of the georeferenced mosaic (dsss_mosaic_render) on a synthetic survey whose images are resident on the device, under the
dead-reckoning poses and under the solved trajectory, and the overlap-consistency score under dead-reckoning, optimised and true poses.
    python tools/mosaic_time.py --frames 200 --rows 2000 --cols 1024 --cell 0.1 [--calls 7] [--profile AMP] [--gain] [--composite MODE [--fill R]]
Prints one JSON line.  Times are wall clock around the call, which ends with a synchronisation of the context's stream and downloads
nothing (download=False): median of --calls calls after one warm-up.  dropped_fraction counts the pixels the filter mask rejects and the
ones that fall outside the grid.
--profile AMP multiplies the raw frames by the sensor profile synth.column_profile(M, AMP) before they are set.  --gain adds the
range-gain normalisation: the time of dsss_mosaic_gain_stats (median and fastest of --calls, the bytes per second two bytes a sample
imply, and that as a fraction of the 6.3 TB/s copy ceiling), the render with and without the table of those statistics (default
parameters) in one process, interleaved call by call, and the consistency score under the three trajectories with and without it.
--composite MODE (near, far, mid, first) adds the composite mosaic: dsss_mosaic_composite with nothing downloaded against
dsss_mosaic_render in one process, interleaved call by call (median, fastest and slowest of --calls after a warm-up round), and the
three cell counts; --fill R fills enclosed holes within R cells.  With --gain both run under the table."""
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
from diasss_amd.synth import Survey, column_profile   # noqa: E402

HBM_PEAK = 8.0e12                                # bytes / s, the roof of DESIGN.md section 4
COPY_CEILING = 6.3e12                            # bytes / s a device-to-device copy reaches

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=200); ap.add_argument("--rows", type=int, default=2000)
ap.add_argument("--cols", type=int, default=1024); ap.add_argument("--cell", type=float, default=0.1)
ap.add_argument("--calls", type=int, default=7)
ap.add_argument("--profile", type=float, default=0.0, metavar="AMP"); ap.add_argument("--gain", action="store_true")
ap.add_argument("--composite", choices=sorted(capi.COMP_MODES), default=None, metavar="MODE"); ap.add_argument("--fill", type=int, default=0, metavar="R")
a = ap.parse_args()
F, N, M = a.frames, a.rows, a.cols
if a.calls < 5:
    sys.exit("--calls must be at least 5")

sv = Survey(F, N, M, seed=20240601 + 1, device="cuda:0")
raws = [sv.frame(f) for f in range(F)]
if a.profile:
    import torch
    prof = torch.from_numpy(column_profile(M, a.profile)).to(raws[0].device)
    raws = [(r * prof[None, :]).contiguous() for r in raws]
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
res = dict(frames=F, rows=N, cols=M, cell=a.cell, grid=[p.W, p.H], samples=samples, calls=a.calls, profile=a.profile,
           render_ms_dr=round(ms_dr, 3), render_ms_dr_min=round(min_dr, 3), render_ms_solved=round(ms_opt, 3), render_ms_solved_min=round(min_opt, 3),
           samples_per_s_dr=samples / (ms_dr * 1e-3), dropped_fraction=1.0 - kept / samples, fullest_cell=int(cnt.max()),
           bytes_per_sample=bytes_total / samples, hbm_fraction_dr=bytes_total / (ms_dr * 1e-3) / HBM_PEAK, lm_iterations=int(stats[0]))
trajs = (("dr", {}), ("solved", dict(rpy6=rpy, ping_off=off)), ("true", dict(rpy6=true, ping_off=off)))
for name, traj in trajs:
    t0 = time.perf_counter()
    nfr, _, _, score = ctx.mosaic_consistency(ids, p, **traj)
    res["score_" + name] = score
    res["consistency_s_" + name] = round(time.perf_counter() - t0, 3)
res["cells_seen_twice"] = int((nfr >= 2).sum())

if a.gain:
    ctx.mosaic_gain_stats(ids)
    ts = []
    for _ in range(a.calls):
        t0 = time.perf_counter(); S, C = ctx.mosaic_gain_stats(ids); ts.append(time.perf_counter() - t0)
    ms_stats, min_stats = 1e3 * float(np.median(ts)), 1e3 * float(min(ts))
    table, T = capi.mosaic_gain_table(S, C)
    # render without and with the table, interleaved call by call (the table goes up outside the timed call)
    t_off, t_on = [], []
    for k in range(a.calls + 1):
        for tab, ts in ((None, t_off), (table, t_on)):
            ctx.mosaic_gain_set(tab)
            t0 = time.perf_counter(); ctx.mosaic_render(ids, p, download=False); dt = time.perf_counter() - t0
            if k:                                                 # (the first round warms up)
                ts.append(dt)
    res.update(gain_stats_ms=round(ms_stats, 3), gain_stats_ms_min=round(min_stats, 3), gain_stats_bytes_per_s=2.0 * samples / (ms_stats * 1e-3),
               gain_stats_copy_fraction=2.0 * samples / (ms_stats * 1e-3) / COPY_CEILING,
               gain_stats_copy_fraction_min=2.0 * samples / (min_stats * 1e-3) / COPY_CEILING,
               gain_target=T, gain_min=int(table.min()), gain_max=int(table.max()), gain_kept_samples=int(C.sum(dtype=np.uint64)),
               render_ms_no_table=round(1e3 * float(np.median(t_off)), 3), render_ms_no_table_min=round(1e3 * min(t_off), 3),
               render_ms_no_table_max=round(1e3 * max(t_off), 3),
               render_ms_table=round(1e3 * float(np.median(t_on)), 3), render_ms_table_min=round(1e3 * min(t_on), 3), render_ms_table_max=round(1e3 * max(t_on), 3))
    ctx.mosaic_gain_set(table)
    for name, traj in trajs:
        res["score_" + name + "_gain"] = ctx.mosaic_consistency(ids, p, **traj)[3]
    ctx.mosaic_gain_set(None)

if a.composite:
    if a.gain:
        ctx.mosaic_gain_set(table)
    t_mean, t_comp = [], []
    for k in range(a.calls + 1):
        t0 = time.perf_counter(); ctx.mosaic_render(ids, p, download=False); dt_mean = time.perf_counter() - t0
        t0 = time.perf_counter(); ctx.mosaic_composite(ids, p, mode=a.composite, fill_radius=a.fill, want=()); dt_comp = time.perf_counter() - t0
        if k:                                                     # (the first round warms up)
            t_mean.append(dt_mean); t_comp.append(dt_comp)
    _, info = ctx.mosaic_composite(ids, p, mode=a.composite, fill_radius=a.fill, want=("info",))
    res.update(composite_mode=a.composite, composite_fill=a.fill, composite_under_table=bool(a.gain),
               composite_ms=round(1e3 * float(np.median(t_comp)), 3), composite_ms_min=round(1e3 * min(t_comp), 3), composite_ms_max=round(1e3 * max(t_comp), 3),
               render_ms_beside=round(1e3 * float(np.median(t_mean)), 3), render_ms_beside_min=round(1e3 * min(t_mean), 3),
               render_ms_beside_max=round(1e3 * max(t_mean), 3),
               cells_direct=int(info.direct), cells_filled=int(info.filled), cells_empty=int(info.empty))
    ctx.mosaic_gain_set(None)
print(json.dumps(res))
pipe.close()

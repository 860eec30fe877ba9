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
three cell counts; --fill R fills enclosed holes within R cells.  With --gain both run under the table.
--gain-bands B [--alt-swing METRES] --angle-profile AMP adds the altitude-banded range gain: the raw frames are multiplied by
synth.angle_profile(M, alt, gr, AMP, 6) (--alt-swing replaces the survey's altitudes by 10 + METRES sin(2 pi s / 20 + 0.9 f) first), B bands
of equal width cover the altitudes, and the tool reports the banded statistics and table (min_count 64, smooth 8), the consistency
score under the TRUE poses with no table, the column table and the banded table, and, interleaved call by call in one process (median,
fastest and slowest of --calls after a warm-up round), dsss_mosaic_gain_stats (mosaic_gainstat_kernel at one band) against
dsss_mosaic_gain_stats_banded (the same kernel at B bands) on the same frames and the render under the column against the banded table.
--footprint STEPS [--max-gap METRES] [--ping-stride K] adds the footprint rendering: dsss_mosaic_render_footprint at max_steps STEPS
against dsss_mosaic_render, and with --composite dsss_mosaic_composite_footprint against dsss_mosaic_composite, in one process,
interleaved call by call (median, fastest and slowest of --calls after a warm-up round), with the sub-samples binned, the empty cells
and the enclosed single-cell holes (an empty cell with a cell that holds a sample directly on both sides along x or along y) of both.
--ping-stride K renders both under a trajectory that moves ping r of a frame to K times its distance from the frame's middle ping (the
dead-reckoning rows stretched along the track): a ping spacing of K bins out of the survey's one, on a grid over the stretched extent."""
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
from diasss_amd.synth import Survey, angle_profile, column_profile   # noqa: E402

HBM_PEAK = 8.0e12                                # bytes / s, the roof of DESIGN.md section 4
COPY_CEILING = 6.3e12                            # bytes / s a device-to-device copy reaches

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=200); ap.add_argument("--rows", type=int, default=2000)
ap.add_argument("--cols", type=int, default=1024); ap.add_argument("--cell", type=float, default=0.1)
ap.add_argument("--calls", type=int, default=7)
ap.add_argument("--profile", type=float, default=0.0, metavar="AMP"); ap.add_argument("--gain", action="store_true")
ap.add_argument("--composite", choices=sorted(capi.COMP_MODES), default=None, metavar="MODE"); ap.add_argument("--fill", type=int, default=0, metavar="R")
ap.add_argument("--gain-bands", type=int, default=0, metavar="B"); ap.add_argument("--alt-swing", type=float, default=None, metavar="METRES")
ap.add_argument("--angle-profile", type=float, default=0.0, metavar="AMP")
ap.add_argument("--footprint", type=int, default=0, metavar="STEPS"); ap.add_argument("--max-gap", type=float, default=1.0, metavar="METRES")
ap.add_argument("--ping-stride", type=int, default=1, metavar="K")
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
if a.gain_bands:
    import torch
    if a.alt_swing is not None:
        s_along = (np.arange(N) + 0.5) * sv.res
        ins = [(i[0], 10.0 + a.alt_swing * np.sin(2 * np.pi * s_along / 20.0 + 0.9 * f), i[2]) for f, i in enumerate(ins)]
    raws = [(r * torch.from_numpy(angle_profile(M, ins[f][1], ins[f][2], a.angle_profile, 6.0)).to(r.device)).contiguous() for f, r in enumerate(raws)]
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

if a.gain_bands:
    alts = np.concatenate([i[1] for i in ins])
    lo, hi = float(alts.min()), float(alts.max())
    bands = capi.GainBands(lo, (hi - lo) / a.gain_bands if hi > lo else 1.0, a.gain_bands, 0)
    gp = capi.GainParams(64, 8, 0, 0)
    t_col, t_band = [], []
    for k in range(a.calls + 1):
        t0 = time.perf_counter(); cS, cC = ctx.mosaic_gain_stats(ids); dt_col = time.perf_counter() - t0
        t0 = time.perf_counter(); bS, bC = ctx.mosaic_gain_stats(ids, bands=bands); dt_band = time.perf_counter() - t0
        if k:                                                     # (the first round warms up)
            t_col.append(dt_col); t_band.append(dt_band)
    assert (bS.sum(axis=0) == cS).all() and (bC.sum(axis=0) == cC).all()
    ctab, cT = capi.mosaic_gain_table(cS, cC, gp)
    btab, bT = capi.mosaic_gain_table(bS, bC, gp, nbands=a.gain_bands)
    r_col, r_band = [], []
    for k in range(a.calls + 1):
        for tab, bd, ts in ((ctab, None, r_col), (btab, bands, r_band)):
            ctx.mosaic_gain_set(tab, bands=bd)
            t0 = time.perf_counter(); ctx.mosaic_render(ids, p, download=False); dt = time.perf_counter() - t0
            if k:
                ts.append(dt)
    tt = dict(rpy6=true, ping_off=off)
    for name, tab, bd in (("none", None, None), ("column", ctab, None), ("banded", btab, bands)):
        ctx.mosaic_gain_set(tab, bands=bd)
        res["score_true_bands_" + name] = ctx.mosaic_consistency(ids, p, **tt)[3]
    ctx.mosaic_gain_set(None)

    def mmm(ts):
        return [round(1e3 * float(np.median(ts)), 3), round(1e3 * min(ts), 3), round(1e3 * max(ts), 3)]
    res.update(gain_bands=a.gain_bands, alt_swing=a.alt_swing, angle_profile=a.angle_profile, bands_alt0=bands.alt0, bands_dalt=bands.dalt,
               bands_target=bT, bands_pings=[int(v) for v in np.bincount([capi.gain_band(bands, v) for v in alts], minlength=a.gain_bands)],
               bands_fallback_entries=int((btab == ctab[None, :]).sum()), colstat_ms_med_min_max=mmm(t_col), bandstat_ms_med_min_max=mmm(t_band),
               render_ms_column_med_min_max=mmm(r_col), render_ms_banded_med_min_max=mmm(r_band))

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
if a.footprint:
    fp = capi.FootprintParams(a.footprint, 0, a.max_gap)
    traj, pf = {}, p
    if a.ping_stride > 1:
        rows = [i[0].copy() for i in ins]
        for r in rows:
            mid = r[len(r) // 2, 3:5].copy()
            r[:, 3:5] = mid + a.ping_stride * (r[:, 3:5] - mid)
        traj = dict(rpy6=np.ascontiguousarray(np.concatenate(rows)), ping_off=off)
        pf = capi.mosaic_grid(ctx.mosaic_bounds(ids, **traj), a.cell)

    def mmm(ts):
        return [round(1e3 * float(np.median(ts)), 3), round(1e3 * min(ts), 3), round(1e3 * max(ts), 3)]

    def holes(cnt):
        v = cnt > 0
        h = np.zeros(v.shape, bool)
        h[:, 1:-1] |= v[:, :-2] & v[:, 2:]; h[1:-1, :] |= v[:-2, :] & v[2:, :]
        return int((~v).sum()), int((h & ~v).sum())
    pairs = [("render", lambda: ctx.mosaic_render(ids, pf, download=False, **traj), lambda: ctx.mosaic_render_footprint(ids, pf, download=False, footprint=fp, **traj))]
    if a.composite:
        pairs.append(("composite", lambda: ctx.mosaic_composite(ids, pf, mode=a.composite, fill_radius=a.fill, want=(), **traj),
                      lambda: ctx.mosaic_composite_footprint(ids, pf, mode=a.composite, fill_radius=a.fill, want=(), footprint=fp, **traj)))
    out = dict(footprint_steps=a.footprint, footprint_max_gap=a.max_gap, ping_stride=a.ping_stride, footprint_grid=[pf.W, pf.H])
    for name, point, foot in pairs:
        t_point, t_foot = [], []
        for k in range(a.calls + 1):
            t0 = time.perf_counter(); point(); dt_p = time.perf_counter() - t0
            t0 = time.perf_counter(); foot(); dt_f = time.perf_counter() - t0
            if k:                                                 # (the first round warms up)
                t_point.append(dt_p); t_foot.append(dt_f)
        out[name + "_point_ms_med_min_max"] = mmm(t_point); out[name + "_footprint_ms_med_min_max"] = mmm(t_foot)
    cnt_p = ctx.mosaic_render(ids, pf, **traj)[1]
    cnt_f = ctx.mosaic_render_footprint(ids, pf, footprint=fp, **traj)[1]
    assert (cnt_f >= cnt_p).all()
    out.update(samples_binned=int(cnt_p.sum(dtype=np.int64)), subsamples_binned=int(cnt_f.sum(dtype=np.int64)))
    out["point_empty_cells"], out["point_single_cell_holes"] = holes(cnt_p)
    out["footprint_empty_cells"], out["footprint_single_cell_holes"] = holes(cnt_f)
    res.update(out)
print(json.dumps(res))
pipe.close()

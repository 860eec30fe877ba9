#!/usr/bin/env python3
"""Dense loop closures on a synthetic survey: the segments of every frame pair with overlapping geo boxes are registered under the
solved trajectory (dsss_mosaic_register_segments), the accepted offsets become pose-graph edges (dsss_mosaic_register_edges), the
trajectory is solved again with them next to the feature-based closures, and the segments are registered once more under the result.
    python tools/dense_closures.py --frames 200 --rows 2000 --cols 1024 --cell 0.1 [--seg-pings 80] [--radius 8] [--calls 5] [--timeout 1500]
                                   [--yaw-fan NYAW [--yaw-step RAD]] [--pyramid L [--refine RHO]] [--peaks-ab] [--profile AMP] [--gain [--gain-bands B]]
Steps: 1. pipeline and dsss_posegraph_solve; 2. segments under the solved trajectory; 3. edges; 4. the edges of dsss_posegraph_select
with the new ones behind them; 5. dsss_posegraph_solve_edges on the frames' dead-reckoning rows; 6. segments under the result.
Prints one JSON line: segments and accepted edges; median and 95th percentile of |offset| in metres over the segments with a peak, the
median ZNCC at zero shift and the consistency score, each before (solved trajectory) and after (solved again); the wall time of the
segment call and of dsss_mosaic_register on the same pairs in the same process (the whole-frame form, the only existing code the new
call's time can be set against), each the median of --calls synchronised calls after one warm-up.
--yaw-fan NYAW (odd, above 1) registers every segment under a fan of NYAW rotations --yaw-step radians apart as well
(dsss_mosaic_register_segments_yaw) and turns the rows into edges that measure the heading (dsss_mosaic_register_edges_yaw): the same
report, with the median and 95th percentile of |theta_hat| over the segments with a peak and the rows on the border of the fan, before
and after, and the wall time of the fan call next to the translation-only call's.
--pyramid L (2..4) registers every segment coarse to fine over L levels as well (dsss_mosaic_register_segments_pyr, --refine cells
around twice the shift found above below the top level) and builds the edges from those rows through the unchanged
dsss_mosaic_register_edges.  Under every trajectory that is registered (with --pyramid also the dead-reckoning one, "dr") it reports
the rows per level, the rows with a border bit, the median and 95th percentile of the total shift in cells over the rows that finished at
level 0, and the flat call's on_border count on the same pairs in the same process; and the wall time of the pyramid call next to the
flat segment call's.
--peaks-ab measures where the peaks are decided instead of steps 2 to 6: for each registration call timed here (the flat segment call,
and the fan's or the pyramid's when asked for) it alternates, in this one process, the host path (DSSS_REG_PEAKS=host, read per call)
and the device path: one warm-up of each, then --calls rounds of host, device, host, each call synchronised and timed with a host clock.
It reports median and minimum per path, the host path's spread against itself (the two interleaved host series), and per path the
bytes copied down and the synchronisations (dsss_mosaic_register_info), and asserts the rows of both paths identical as bytes.
--profile AMP multiplies the raw frames by the sensor profile synth.column_profile(M, AMP) before they are set.  --gain runs steps 2 to 6
a second time in the same process under the range-gain table of the frames' own statistics (dsss_mosaic_gain_stats, dsss_mosaic_gain_table
with the default parameters, dsss_mosaic_gain_set) and reports them under "gain": segments with a peak and accepted edges, the median ZNCC
at the peak and at zero shift, and the consistency score before and after solving again, next to the same figures without the table.
--gain-bands B (with --gain) makes that table an altitude-banded one: B bands of equal width over the frames' altitudes
(dsss_mosaic_gain_stats_banded, dsss_mosaic_gain_table_banded, dsss_mosaic_gain_set_banded).
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
ap.add_argument("--seg-pings", type=int, default=80)
ap.add_argument("--radius", type=int, default=8); ap.add_argument("--min-cells", type=int, default=256)
ap.add_argument("--yaw-fan", type=int, default=1); ap.add_argument("--yaw-step", type=float, default=0.01)
ap.add_argument("--pyramid", type=int, default=1); ap.add_argument("--refine", type=int, default=3)
ap.add_argument("--calls", type=int, default=5); ap.add_argument("--timeout", type=float, default=1500.0)
ap.add_argument("--peaks-ab", action="store_true")
ap.add_argument("--profile", type=float, default=0.0, metavar="AMP"); ap.add_argument("--gain", action="store_true")
ap.add_argument("--gain-bands", type=int, default=0, metavar="B")
ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
a = ap.parse_args()
if a.calls < 5:
    sys.exit("--calls must be at least 5")
if a.yaw_fan < 1 or a.yaw_fan > 17 or a.yaw_fan % 2 == 0 or not a.yaw_step > 0:
    sys.exit("--yaw-fan must be odd and in 1..17, --yaw-step positive")

if a.pyramid < 1 or a.pyramid > 4 or a.refine < 1 or a.refine > 16 or (a.pyramid > 1 and a.yaw_fan > 1):
    sys.exit("--pyramid must be in 1..4, --refine in 1..16; the yaw fan over the pyramid is not built")

if not a.worker:
    try:
        sys.exit(subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"] + sys.argv[1:], timeout=a.timeout).returncode)
    except subprocess.TimeoutExpired:
        sys.exit("dense_closures: the GPU step did not finish within %g s" % a.timeout)

import numpy as np                               # noqa: E402
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diasss_amd import capi                      # noqa: E402
from diasss_amd.pipeline import Pipeline         # noqa: E402
from diasss_amd.synth import Survey, column_profile   # noqa: E402

F, N, M = a.frames, a.rows, a.cols
sv = Survey(F, N, M, seed=20240601 + 2, device="cuda:0")
raws = [sv.frame(f) for f in range(F)]
if a.profile:
    import torch                                 # noqa: E402
    prof = torch.from_numpy(column_profile(M, a.profile)).to(raws[0].device)
    raws = [(r * prof[None, :]).contiguous() for r in raws]
ins = [sv.inputs(f) for f in range(F)]
pipe = Pipeline(F, device=0)
pipe.run(raws, [i[0] for i in ins], [i[1] for i in ins], [i[2] for i in ins])
ctx = pipe.ctx
_, rpy, stats = ctx.posegraph_solve(F, F * N, want_rpy=True)                      # 1
ids = np.arange(F, dtype=np.int32); off = (ids * N).astype(np.int32)
p = capi.mosaic_grid(ctx.mosaic_bounds(ids), a.cell)              # one grid for both trajectories: the dead-reckoning extent
boxes = [ctx.mosaic_bounds([f]) for f in range(F)]
pairs = [(i, j) for i in range(F) for j in range(i + 1, F)
         if boxes[i][0] <= boxes[j][1] and boxes[j][0] <= boxes[i][1] and boxes[i][2] <= boxes[j][3] and boxes[j][2] <= boxes[i][3]]
reg = capi.RegParams(a.radius, a.min_cells)
res = dict(frames=F, rows=N, cols=M, cell=a.cell, grid=[p.W, p.H], radius=a.radius, min_cells=a.min_cells, seg_pings=a.seg_pings, pairs=len(pairs),
           calls=a.calls, lm_iterations=int(stats[0]), profile=a.profile)
if not pairs:
    print(json.dumps(res)); pipe.close(); sys.exit(0)


def timed(fn):
    fn()
    ts = []
    for _ in range(a.calls):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return round(1e3 * float(np.median(ts)), 3), round(1e3 * float(min(ts)), 3)


FAN = a.yaw_fan > 1
yaw = capi.RegYawParams(a.yaw_fan, 0, a.yaw_step)
PYR = a.pyramid > 1
pyr = capi.RegPyrParams(a.pyramid, a.refine)


def register(traj):
    if PYR:
        return ctx.mosaic_register_segments_pyr(ids, p, pairs, a.seg_pings, pyr=pyr, reg=reg, rpy6=traj, ping_off=off)
    if FAN:
        return ctx.mosaic_register_segments_yaw(ids, p, pairs, a.seg_pings, yaw=yaw, reg=reg, rpy6=traj, ping_off=off)
    return ctx.mosaic_register_segments(ids, p, pairs, a.seg_pings, reg=reg, rpy6=traj, ping_off=off)


def describe(segs, traj):
    fan = {}
    if PYR:
        done = segs["level"] == 0
        t = np.hypot(segs["lx"][done, 0], segs["ly"][done, 0])
        flat = ctx.mosaic_register_segments(ids, p, pairs, a.seg_pings, reg=reg, rpy6=traj, ping_off=off)["r"]
        fan = dict(rows_per_level={str(l): int((segs["level"] == l).sum()) for l in range(-1, a.pyramid)}, border_rows=int((segs["border_mask"] != 0).sum()),
                   total_shift_median_cells=float(np.median(t)) if done.any() else None, total_shift_p95_cells=float(np.percentile(t, 95)) if done.any() else None,
                   flat_on_border=int((flat["on_border"][flat["zncc"] > -2.0] != 0).sum()), flat_with_peak=int((flat["zncc"] > -2.0).sum()))
        segs = segs["s"]
    if FAN:
        ok = segs["s"]["r"]["zncc"] > -2.0
        t = np.abs(segs["theta_hat"][ok])
        fan = dict(theta_hat_median_rad=float(np.median(t)) if ok.any() else None, theta_hat_p95_rad=float(np.percentile(t, 95)) if ok.any() else None,
                   on_yaw_border=int((segs["yaw_on_border"][ok] != 0).sum()), zncc_median=float(np.median(segs["s"]["r"]["zncc"][ok])) if ok.any() else None,
                   zncc_unrotated_median=float(np.median(segs["zncc_k0"][segs["zncc_k0"] > -2.0])) if (segs["zncc_k0"] > -2.0).any() else None)
        segs = segs["s"]
    return dict(_describe(segs, traj), **fan)


def _describe(segs, traj):
    r = segs["r"]
    ok = r["zncc"] > -2.0
    d = np.hypot(r["off_x"][ok], r["off_y"][ok])
    z0 = r["zncc0"][r["zncc0"] > -2.0]
    return dict(with_peak=int(ok.sum()), on_border=int((r["on_border"][ok] != 0).sum()),
                offset_median_m=float(np.median(d)) if ok.any() else None, offset_p95_m=float(np.percentile(d, 95)) if ok.any() else None,
                zncc_peak_median=float(np.median(r["zncc"][ok])) if ok.any() else None, zncc0_median=float(np.median(z0)) if len(z0) else None, consistency=float(ctx.mosaic_consistency(ids, p, rpy6=traj, ping_off=off)[3]))


def rows_of(poses12):
    """total x 12 (R row-major, t) -> "r p y x y z" (Rot3::rpy, as dsss_posegraph_solve writes its rpy6 rows)"""
    P = poses12
    return np.ascontiguousarray(np.stack([np.arctan2(P[:, 7], P[:, 8]), np.arctan2(-P[:, 6], np.hypot(P[:, 7], P[:, 8])), np.arctan2(P[:, 3], P[:, 0]),
                                          P[:, 9], P[:, 10], P[:, 11]], 1))


def peaks_ab(fn):
    """host path against device path of one registration call, interleaved in this process"""
    def run(host):
        if host:
            os.environ["DSSS_REG_PEAKS"] = "host"
        try:
            t0 = time.perf_counter(); rows = fn(); dt = time.perf_counter() - t0
        finally:
            os.environ.pop("DSSS_REG_PEAKS", None)
        return dt, rows.tobytes(), ctx.mosaic_register_info()
    _, want, ih = run(True)
    _, got, idv = run(False)
    assert ih.tables_device == 0 and idv.tables_host == 0 and idv.tables_device == ih.tables_host
    ts = dict(host_a=[], device=[], host_b=[])
    for _ in range(a.calls):
        for key in ("host_a", "device", "host_b"):
            dt, rows, _i = run(key != "device")
            assert rows == want, "peaks-ab: the rows of the %s path differ" % key
            ts[key].append(1e3 * dt)
    assert got == want
    out = dict(runs=a.calls, tables=int(ih.tables_host))
    for key, v in ts.items():
        out[key + "_ms_median"] = round(float(np.median(v)), 3); out[key + "_ms_min"] = round(min(v), 3)
    out["host_spread_ms"] = round(abs(out["host_a_ms_median"] - out["host_b_ms_median"]), 3)
    out.update(host_bytes_down=int(ih.bytes_down), device_bytes_down=int(idv.bytes_down), host_syncs=int(ih.syncs), device_syncs=int(idv.syncs))
    return out


if a.peaks_ab:
    ab = dict(segments=peaks_ab(lambda: ctx.mosaic_register_segments(ids, p, pairs, a.seg_pings, reg=reg, rpy6=rpy, ping_off=off)))
    if PYR or FAN:
        ab["segments_pyr" if PYR else "segments_yaw"] = peaks_ab(lambda: register(rpy))
    res["peaks_ab"] = ab
    print(json.dumps(res)); pipe.close(); sys.exit(0)

res["segments_ms"], res["segments_ms_min"] = timed(lambda: ctx.mosaic_register_segments(ids, p, pairs, a.seg_pings, reg=reg, rpy6=rpy, ping_off=off))
res["whole_frame_ms"], res["whole_frame_ms_min"] = timed(lambda: ctx.mosaic_register(ids, p, pairs, reg=reg, rpy6=rpy, ping_off=off))
if PYR:
    res["pyramid"], res["refine"] = a.pyramid, a.refine
    res["segments_pyr_ms"], res["segments_pyr_ms_min"] = timed(lambda: register(rpy))
if FAN:
    res["yaw_fan"], res["yaw_step"] = a.yaw_fan, a.yaw_step
    res["segments_yaw_ms"], res["segments_yaw_ms_min"] = timed(lambda: register(rpy))
dr = np.ascontiguousarray(np.concatenate([i[0] for i in ins]))
true = np.ascontiguousarray(np.concatenate(sv.poses_true))
old = ctx.posegraph_select(F)                                                                            # 4 (the feature-based closures)


def closures():
    """steps 2 to 6 under whatever range-gain table the context holds"""
    before = register(rpy)                                                                               # 2
    if FAN:                                                                                              # 3
        new, src = ctx.mosaic_register_edges_yaw(ids, p, pairs, before, edge_params=capi.RegEdgeYawParams(capi.reg_edge_params_default(), yaw, 1.0),
                                                 rpy6=rpy, ping_off=off)
    else:
        new, src = ctx.mosaic_register_edges(ids, p, pairs, np.ascontiguousarray(before["s"]) if PYR else before, rpy6=rpy, ping_off=off)
    t0 = time.perf_counter()
    poses, stats2 = ctx.posegraph_solve_edges(dr, np.concatenate([old, new]))                            # 5
    solve_ms = 1e3 * (time.perf_counter() - t0)
    again = rows_of(poses)
    after = register(again)                                                                             # 6
    return dict(segments=len(before), feature_edges=len(old), accepted_edges=len(new), lm_iterations_again=int(stats2[0]), solve_again_ms=round(solve_ms, 3),
                before=describe(before, rpy), after=describe(after, again),
                consistency_dr=float(ctx.mosaic_consistency(ids, p)[3]), consistency_true=float(ctx.mosaic_consistency(ids, p, rpy6=true, ping_off=off)[3]))


res.update(closures())
if a.gain:
    alts = np.concatenate([i[1] for i in ins])
    bands = capi.GainBands(float(alts.min()), float(np.ptp(alts)) / a.gain_bands or 1.0, a.gain_bands, 0) if a.gain_bands else None
    S, C = ctx.mosaic_gain_stats(ids, bands=bands)
    table, T = capi.mosaic_gain_table(S, C, nbands=a.gain_bands or None)
    ctx.mosaic_gain_set(table, bands=bands)
    res["gain"] = dict(closures(), target=T, gain_min=int(table.min()), gain_max=int(table.max()))
    ctx.mosaic_gain_set(None)
if PYR:                                          # the same counts under dead reckoning, where the legs lie furthest from where they belong
    res["dr"] = describe(register(dr), dr)
print(json.dumps(res))
pipe.close()

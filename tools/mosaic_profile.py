#!/usr/bin/env python3
"""The per-ping disagreement profile (include/dsss_profile.h) on a synthetic survey whose images are resident on the device:
    python tools/mosaic_profile.py --frames 200 --rows 2000 --cols 1024 --cell 0.1 [--calls 7] [--from K --count W --shift D] [--min-count C] [--top T] [--residual PATH.npy]
  - every frame profiled against the mosaic of the others under the TRUE poses: rms and compared share (compared / binned) per frame;
  - the same under the same poses with the frames K .. K + W - 1 shifted by (D, -D / 2) metres, and the frames ranked by rms (the first
    --top of them; * marks a shifted frame);
  - the residual waterfall of frame K under the shifted poses: how many of its samples are compared and their mean |d|; --residual saves
    the int16 layer (-32768 where a sample is not compared);
  - times: the profile of all frames (records downloaded, no residual layers) beside dsss_mosaic_render (nothing downloaded) and
    dsss_mosaic_consistency on the same inputs, and the canvas profile of the W frames beside the fresh profile of the same W.
The timed variants alternate call by call; every figure is [median, fastest, slowest] in ms of --calls calls after a warm-up round, wall
clock around the call, which ends with a synchronisation of the context's stream.  Prints the tables, then one JSON line."""
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

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=200); ap.add_argument("--rows", type=int, default=2000)
ap.add_argument("--cols", type=int, default=1024); ap.add_argument("--cell", type=float, default=0.1)
ap.add_argument("--calls", type=int, default=7)
ap.add_argument("--from", dest="first", type=int, default=None, metavar="K"); ap.add_argument("--count", type=int, default=8, metavar="W")
ap.add_argument("--shift", type=float, default=0.5, metavar="D"); ap.add_argument("--min-count", type=int, default=1, metavar="C")
ap.add_argument("--top", type=int, default=12, metavar="T"); ap.add_argument("--residual", default=None, metavar="PATH.npy")
a = ap.parse_args()
F, N, M = a.frames, a.rows, a.cols
W = max(1, min(a.count, F))
K = F - W if a.first is None else max(0, min(a.first, F - W))
if a.calls < 5:
    sys.exit("--calls must be at least 5")

sv = Survey(F, N, M, seed=20240601 + 1, device="cuda:0")
raws = [sv.frame(f) for f in range(F)]
ins = [sv.inputs(f) for f in range(F)]
pipe = Pipeline(F, device=0)
pipe.set_frames(raws, [i[0] for i in ins], [i[1] for i in ins], [i[2] for i in ins])
pipe.extract()
ctx = pipe.ctx
ids = np.arange(F, dtype=np.int32); off = (ids * N).astype(np.int32)
true = np.ascontiguousarray(np.concatenate(sv.poses_true))
moved = true.copy()
moved[K * N:(K + W) * N, 3] += a.shift; moved[K * N:(K + W) * N, 4] -= a.shift / 2
grow = abs(a.shift) + 1.0
p = capi.mosaic_grid(ctx.mosaic_bounds(ids, rpy6=true, ping_off=off) + np.array([-grow, grow, -grow, grow]), a.cell)
window = np.arange(K, K + W, dtype=np.int32)


def per_frame(stats):
    """rows of PING_DTYPE over all frames -> (rms, compared share, compared) per frame"""
    n = stats["n"].astype(np.int64).sum(1).reshape(F, N).sum(1)
    b = stats["binned"].astype(np.int64).sum(1).reshape(F, N).sum(1)
    ssd = stats["ssd"].astype(np.int64).sum(1).reshape(F, N).sum(1)
    rms = np.where(n > 0, np.sqrt(ssd / np.maximum(n, 1)), 0.0)
    return rms, np.where(b > 0, n / np.maximum(b, 1), 0.0), n


def mmm(ts):
    return [round(1e3 * float(np.median(ts)), 3), round(1e3 * min(ts), 3), round(1e3 * max(ts), 3)]


def rounds(variants):
    """variants: {name: callable}; one warm-up round, then --calls rounds, the variants in turn within a round"""
    ts = {k: [] for k in variants}
    for r in range(a.calls + 1):
        for k, fn in variants.items():
            t0 = time.perf_counter(); fn(); dt = time.perf_counter() - t0
            if r:
                ts[k].append(dt)
    return {k: mmm(v) for k, v in ts.items()}


st_true, _, info_true = ctx.profile_mosaic(ids, p, min_count=a.min_count, rpy6=true, ping_off=off, want=("stats", "info"))
st_moved, _, info_moved = ctx.profile_mosaic(ids, p, min_count=a.min_count, rpy6=moved, ping_off=off, want=("stats", "info"))
rms_t, share_t, n_t = per_frame(st_true)
rms_m, share_m, n_m = per_frame(st_moved)
print("frame   rms true  share true   rms shifted  share shifted   (frames %d .. %d shifted by (%g, %g) m; * = shifted)" % (K, K + W - 1, a.shift, -a.shift / 2))
for f in range(F):
    print("%4d%s  %9.3f  %10.4f  %12.3f  %13.4f" % (f, "*" if K <= f < K + W else " ", rms_t[f], share_t[f], rms_m[f], share_m[f]))
order = np.lexsort((np.arange(F), -rms_m))
print("rank  frame   rms shifted   rms true   compared")
for r, f in enumerate(order[:a.top]):
    print("%4d  %4d%s  %11.3f  %9.3f  %9d" % (r + 1, f, "*" if K <= f < K + W else " ", rms_m[f], rms_t[f], n_m[f]))
ranks = {int(f): r + 1 for r, f in enumerate(order)}
# the residual waterfall of the first shifted frame
_, diff, _ = ctx.profile_mosaic(ids, p, prof=[K], min_count=a.min_count, rpy6=moved, ping_off=off, want=("diff",))
res_layer = diff[0]
cmp = res_layer != capi.PROFILE_NONE
if a.residual:
    np.save(a.residual, res_layer)
print("residual waterfall of frame %d: %d x %d int16, %d samples compared, mean |d| %.3f" % (
    K, res_layer.shape[0], res_layer.shape[1], int(cmp.sum()), float(np.abs(res_layer[cmp].astype(np.int64)).mean()) if cmp.any() else 0.0))

# ---- times: the profile of all frames beside the render and the consistency map
t_all = rounds({"profile_all": lambda: ctx.profile_mosaic(ids, p, min_count=a.min_count, rpy6=true, ping_off=off, want=("stats",)),
                "render": lambda: ctx.mosaic_render(ids, p, rpy6=true, ping_off=off, download=False),
                "consistency": lambda: ctx.mosaic_consistency(ids, p, rpy6=true, ping_off=off)})
# ---- the canvas profile of the W frames beside the fresh profile of the same W
cv = ctx.canvas(p)
cv.put(ids, rpy6=moved, ping_off=off)
t_win = rounds({"canvas_profile": lambda: cv.profile(window, min_count=a.min_count, want=("stats",)),
                "fresh_profile": lambda: ctx.profile_mosaic(ids, p, prof=window, min_count=a.min_count, rpy6=moved, ping_off=off, want=("stats",))})
same = cv.profile(window, min_count=a.min_count)[0].tobytes() == st_moved[K * N:(K + W) * N].tobytes()
cv.close()
shifted_rms = rms_m[K:K + W]; others = np.delete(rms_m, np.arange(K, K + W))
res = dict(frames=F, rows=N, cols=M, cell=a.cell, grid=[p.W, p.H], calls=a.calls, min_count=a.min_count, shifted_from=K, shifted_count=W, shift=a.shift,
           rms_true_all=info_true.rms, rms_shifted_all=info_moved.rms, compared_share_true=info_true.n / max(info_true.binned, 1),
           rms_true_min_med_max=[float(rms_t.min()), float(np.median(rms_t)), float(rms_t.max())],
           rms_shifted_frames_min_med_max=[float(shifted_rms.min()), float(np.median(shifted_rms)), float(shifted_rms.max())],
           rms_other_frames_min_med_max=[float(others.min()), float(np.median(others)), float(others.max())] if len(others) else None,
           ranks_of_shifted_frames=[ranks[int(f)] for f in window], residual_compared=int(cmp.sum()),
           profile_all_ms=t_all["profile_all"], render_ms=t_all["render"], consistency_ms=t_all["consistency"],
           canvas_profile_window_ms=t_win["canvas_profile"], fresh_profile_window_ms=t_win["fresh_profile"], canvas_equals_fresh=bool(same))
print(json.dumps(res))
pipe.close()
if not same:
    sys.exit("the canvas profile differs from the fresh one")

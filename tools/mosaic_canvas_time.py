#!/usr/bin/env python3
"""Times of the mosaic canvas (include/dsss_canvas.h) against the fresh render, in one process on one synthetic survey whose images are
resident on the device:
    python tools/mosaic_canvas_time.py --frames 200 --rows 2000 --cols 1024 --cell 0.1 [--window 8] [--calls 7] [--footprint S]
  - put of all frames into an empty canvas against dsss_mosaic_render without download;
  - move of the last --window frames by 0.01 m and by 0.3 m, DSSS_CANVAS_MOVE_AUTO against DSSS_CANVAS_MOVE_SPLIT (two canvases that
    hold the same frames; a call moves the frames from the base rows to the shifted ones, the next one back: both are moves by d);
  - remove of the last --window frames (put back outside the timed call);
  - read of the dirty window of such a move against a read of the whole grid;
  - the fresh render of the whole survey beside each.
The variants alternate call by call; every figure is [median, fastest, slowest] in ms of --calls calls after a warm-up round, wall clock
around the call, which ends with a synchronisation of the context's stream.  Prints one JSON line."""
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
ap.add_argument("--window", type=int, default=8, metavar="W"); ap.add_argument("--calls", type=int, default=7)
ap.add_argument("--footprint", type=int, default=0, metavar="S"); ap.add_argument("--max-gap", type=float, default=1.0, metavar="METRES")
a = ap.parse_args()
F, N, M, W = a.frames, a.rows, a.cols, min(a.window, a.frames)

sv = Survey(F, N, M, seed=20240601 + 1, device="cuda:0")
raws = [sv.frame(f) for f in range(F)]
ins = [sv.inputs(f) for f in range(F)]
pipe = Pipeline(F, device=0)
pipe.set_frames(raws, [i[0] for i in ins], [i[1] for i in ins], [i[2] for i in ins])
pipe.extract()
ctx = pipe.ctx
ids = np.arange(F, dtype=np.int32); off = (ids * N).astype(np.int32)
base = np.ascontiguousarray(np.concatenate([i[0] for i in ins]))
p = capi.mosaic_grid(ctx.mosaic_bounds(ids) + np.array([-1.0, 1.0, -1.0, 1.0]), a.cell)
fp = (a.footprint, a.max_gap) if a.footprint else None
last = ids[F - W:]; last_off = np.arange(W, dtype=np.int32) * N


def mmm(ts):
    return [round(1e3 * float(np.median(ts)), 3), round(1e3 * min(ts), 3), round(1e3 * max(ts), 3)]


def timed(fn):
    t0 = time.perf_counter(); fn(); return time.perf_counter() - t0


def fresh():
    if fp is None:
        ctx.mosaic_render(ids, p, rpy6=base, ping_off=off, download=False)
    else:
        ctx.mosaic_render_footprint(ids, p, rpy6=base, ping_off=off, download=False, footprint=fp)


def rounds(variants):
    """variants: {name: callable}; one warm-up round, then --calls rounds, the variants in turn within a round"""
    ts = {k: [] for k in variants}
    for r in range(a.calls + 1):
        for k, fn in variants.items():
            dt = timed(fn)
            if r:
                ts[k].append(dt)
    return {k: mmm(v) for k, v in ts.items()}


auto = ctx.canvas(p, footprint=fp, move=capi.CANVAS_MOVE_AUTO)
split = ctx.canvas(p, footprint=fp, move=capi.CANVAS_MOVE_SPLIT)
res = dict(frames=F, rows=N, cols=M, cell=a.cell, grid=[p.W, p.H], window=W, calls=a.calls, footprint=a.footprint)

# ---- put of all frames into an empty canvas (the clear is outside the timed call)
ts = {"put_all": [], "fresh_render": []}
for r in range(a.calls + 1):
    auto.clear()
    dt_put = timed(lambda: auto.put(ids, rpy6=base, ping_off=off)); dt_fresh = timed(fresh)
    if r:
        ts["put_all"].append(dt_put); ts["fresh_render"].append(dt_fresh)
res["put_all_ms"] = mmm(ts["put_all"]); res["fresh_render_ms"] = mmm(ts["fresh_render"])
split.put(ids, rpy6=base, ping_off=off)

# ---- move of the last W frames, AUTO against SPLIT, the fresh render beside them
for d in (0.01, 0.3):
    rows = [base[F * N - W * N:].copy(), base[F * N - W * N:].copy()]
    rows[1][:, 3] += d; rows[1][:, 4] -= d / 2
    turn = {"auto": 0, "split": 0}
    info = {}

    def move(cv, name):
        turn[name] ^= 1
        info[name] = cv.put(last, rpy6=rows[turn[name]], ping_off=last_off)
    out = rounds({"auto": lambda: move(auto, "auto"), "split": lambda: move(split, "split"), "fresh": fresh})
    assert info["auto"].moved == W and info["split"].moved == W
    res["move_%g" % d] = dict(auto_ms=out["auto"], split_ms=out["split"], fresh_render_ms=out["fresh"], pings_auto=int(info["auto"].pings),
                              pings_split=int(info["split"].pings), window_cells=int(info["auto"].win[2]) * int(info["auto"].win[3]))
    for cv, name in ((auto, "auto"), (split, "split")):                          # back on the base rows
        if turn[name]:
            move(cv, name)

# ---- remove of the last W frames (put back outside the timed call)
ts = {"remove": [], "put_back": [], "fresh_render": []}
for r in range(a.calls + 1):
    dt_rm = timed(lambda: auto.remove(last)); dt_put = timed(lambda: auto.put(last, rpy6=base[F * N - W * N:], ping_off=last_off)); dt_fresh = timed(fresh)
    if r:
        ts["remove"].append(dt_rm); ts["put_back"].append(dt_put); ts["fresh_render"].append(dt_fresh)
res["remove_ms"] = mmm(ts["remove"]); res["put_window_ms"] = mmm(ts["put_back"]); res["fresh_render_beside_remove_ms"] = mmm(ts["fresh_render"])

# ---- read of the dirty window of a move against a read of the whole grid
auto.dirty()
shifted = base[F * N - W * N:].copy(); shifted[:, 3] += 0.01
auto.put(last, rpy6=shifted, ping_off=last_off)
win = auto.dirty()
out = rounds({"window": lambda: auto.read(win), "full": lambda: auto.read(), "fresh": fresh})
res["read_dirty_window_ms"] = out["window"]; res["read_full_ms"] = out["full"]; res["dirty_window"] = list(win); res["fresh_render_beside_read_ms"] = out["fresh"]
auto.put(last, rpy6=base[F * N - W * N:], ping_off=last_off)

# ---- both canvases still read what the fresh render gives
want = ctx.mosaic_render(ids, p, rpy6=base, ping_off=off) if fp is None else ctx.mosaic_render_footprint(ids, p, rpy6=base, ping_off=off, footprint=fp)
want = b"".join(x.tobytes() for x in want)
res["canvases_equal_fresh_render"] = all(b"".join(x.tobytes() for x in cv.read()) == want for cv in (auto, split))
print(json.dumps(res))
auto.close(); split.close()
pipe.close()
if not res["canvases_equal_fresh_render"]:
    sys.exit("a canvas differs from the fresh render")

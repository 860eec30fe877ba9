#!/usr/bin/env python3
"""The mosaic canvas (include/dsss_canvas.h) beside an online survey: the frames of a seeded synthetic survey arrive one at a time, at
each arrival the last W frames get a seeded correction of about --shift metres, and ALL frames that have arrived are put under the
whole trajectory -- the frames outside the window are skipped (their rows are bytewise the stored ones), so the put costs the window.
    python tools/mosaic_online.py --frames 200 --rows 2000 --cols 1024 --cell 0.1 --window 8 --shift 0.01 [--footprint S] [--move auto|split] [--every K]
Every K-th arrival a fresh render of the same state is timed beside the put (dsss_mosaic_render, or dsss_mosaic_render_footprint with
--footprint, nothing downloaded).  At the end the canvas is compared byte for byte with the fresh render of the final state.  Prints one
JSON line: medians of the put and of the fresh render (wall clock around the synchronised call, ms), the fresh render by arrival (to
see it grow with the survey where the put does not), the workgroups launched per put and the window sizes in cells."""
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
ap.add_argument("--window", type=int, default=8, metavar="W"); ap.add_argument("--shift", type=float, default=0.01, metavar="METRES")
ap.add_argument("--footprint", type=int, default=0, metavar="S"); ap.add_argument("--max-gap", type=float, default=1.0, metavar="METRES")
ap.add_argument("--move", choices=("auto", "split"), default="auto"); ap.add_argument("--every", type=int, default=20, metavar="K")
a = ap.parse_args()
F, N, M, W = a.frames, a.rows, a.cols, max(1, a.window)

sv = Survey(F, N, M, seed=20240601 + 1, device="cuda:0")
raws = [sv.frame(f) for f in range(F)]
ins = [sv.inputs(f) for f in range(F)]
pipe = Pipeline(F, device=0)
pipe.set_frames(raws, [i[0] for i in ins], [i[1] for i in ins], [i[2] for i in ins])
pipe.extract()
ctx = pipe.ctx
ids = np.arange(F, dtype=np.int32); off = (ids * N).astype(np.int32)
traj = np.ascontiguousarray(np.concatenate([i[0] for i in ins]))
bb = ctx.mosaic_bounds(ids)
pad = 4.0 * a.shift * W + a.cell
p = capi.mosaic_grid(bb + np.array([-pad, pad, -pad, pad]), a.cell)
fp = (a.footprint, a.max_gap) if a.footprint else None
cv = ctx.canvas(p, footprint=fp, move=capi.CANVAS_MOVE_AUTO if a.move == "auto" else capi.CANVAS_MOVE_SPLIT)


def fresh(n, download=False):
    if fp is None:
        return ctx.mosaic_render(ids[:n], p, rpy6=traj, ping_off=off[:n], download=download)
    return ctx.mosaic_render_footprint(ids[:n], p, rpy6=traj, ping_off=off[:n], download=download, footprint=fp)


rng = np.random.default_rng(7)
t_put, t_fresh, pings, wins, moved = [], [], [], [], []
fresh(1); cv.put(ids[:1], rpy6=traj, ping_off=off[:1]); cv.clear()                # warm-up: scratch, row store
for f in range(F):
    for g in range(max(0, f - W + 1), f + (1 if f else 0)):                      # the window's correction: the frames that had arrived move
        d = rng.normal(size=2); d *= a.shift / max(np.hypot(*d), 1e-12)
        traj[g * N:(g + 1) * N, 3:5] += d
    t0 = time.perf_counter(); info = cv.put(ids[:f + 1], rpy6=traj, ping_off=off[:f + 1]); t_put.append(time.perf_counter() - t0)
    assert info.added == 1 and info.moved + info.skipped == f
    pings.append(int(info.pings)); wins.append(int(info.win[2]) * int(info.win[3])); moved.append(int(info.moved))
    if (f + 1) % a.every == 0 or f == F - 1:
        t0 = time.perf_counter(); fresh(f + 1); t_fresh.append((f + 1, round(1e3 * (time.perf_counter() - t0), 3)))
same = b"".join(x.tobytes() for x in cv.read()) == b"".join(x.tobytes() for x in fresh(F, download=True))
steady = t_put[W:] or t_put
res = dict(frames=F, rows=N, cols=M, cell=a.cell, grid=[p.W, p.H], window=W, shift=a.shift, footprint=a.footprint, move=a.move,
           put_ms_median=round(1e3 * float(np.median(steady)), 3), put_ms_min=round(1e3 * min(steady), 3), put_ms_max=round(1e3 * max(steady), 3),
           put_ms_first_half=round(1e3 * float(np.median(steady[:len(steady) // 2] or steady)), 3),
           put_ms_second_half=round(1e3 * float(np.median(steady[len(steady) // 2:])), 3),
           fresh_render_ms_by_arrival=t_fresh, fresh_render_ms_median=round(float(np.median([t for _, t in t_fresh])), 3),
           moved_per_put_median=int(np.median(moved[W:] or moved)), pings_per_put_median=int(np.median(pings[W:] or pings)), pings_total=int(sum(pings)),
           window_cells_median=int(np.median(wins)), window_cells_max=int(max(wins)), grid_cells=p.W * p.H, canvas_equals_fresh_render=bool(same))
print(json.dumps(res))
cv.close()
pipe.close()
if not same:
    sys.exit("the canvas differs from the fresh render")

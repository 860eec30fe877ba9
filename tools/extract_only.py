#!/usr/bin/env python3
"""Wall time of frame set-up + extraction (set_frames starts the extraction, extract finishes it; device-resident frames), for A/B runs of its switches
(DSSS_LIB = another build of the library): python tools/extract_only.py [frames=200] [repeats=10] [--dtype f64|f32|u16|u8[,...]]
--dtype: the sample type of the resident frames (default f64).  A comma-separated list runs the types interleaved in one process, each on
a context of its own, and prints per type the wall time and, from the profile scopes of a last profiled repeat, the time of the two kernels
that read the raw image with the rate of their algorithmic bytes (row reduce: esize per pixel; normalise: esize in, 1 out)."""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from diasss_amd.synth import Survey
from diasss_amd.pipeline import Pipeline
NAMES = {"f64": "float64", "f32": "float32", "u16": "uint16", "u8": "uint8"}
ap = argparse.ArgumentParser()
ap.add_argument("frames", nargs="?", type=int, default=200)
ap.add_argument("repeats", nargs="?", type=int, default=10)
ap.add_argument("--dtype", default="f64")
a = ap.parse_args()
F, reps, types = a.frames, a.repeats, a.dtype.split(",")
if any(t not in NAMES for t in types):
    sys.exit("--dtype: f64, f32, u16 or u8")
N, M = 2000, 1024
sv = Survey(F, N, M, seed=20240602, device="cuda:0")
ins = [sv.inputs(f) for f in range(F)]
poses = [i[0] for i in ins]; alts = [i[1] for i in ins]; grs = [i[2] for i in ins]
raws = {t: [] for t in types}
for f in range(F):
    img = sv.frame(f)
    for t in types: raws[t].append(img if t == "f64" else sv.frame(f, NAMES[t]))
pipes = {t: Pipeline(F) for t in types}
ts = {t: [] for t in types}


def step(t):
    pipe = pipes[t]
    torch.cuda.synchronize(); pipe.ctx.sync()
    t0 = time.perf_counter()
    pipe.set_frames(raws[t], poses, alts, grs)              # (starts the extraction of device-resident frames itself)
    pipe.extract(); pipe.ctx.sync()
    return 1e3 * (time.perf_counter() - t0)


for s in range(reps + 2):
    for t in types: ts[t].append(step(t))
for t in types:
    v = sorted(ts[t][2:])
    print("set_frames + extract, %d %s frames: median %.3f ms, min %.3f | %s %s" % (F, t, v[len(v) // 2], v[0], os.environ.get("DSSS_LIB", "<tree>")[-18:],
          " ".join("%s=%s" % (k, v) for k, v in sorted(os.environ.items()) if k.startswith("DSSS_EX_"))))
if len(types) > 1 or types[0] != "f64":
    for t in types:                                         # one profiled repeat per type: the scopes of the two kernels that read the raw image
        ctx = pipes[t].ctx
        ctx.profile(True); ctx.profile_reset(); step(t); prof = ctx.profile_get(); ctx.profile(False)
        print("%s profile: " % t + ", ".join("%s %.3f ms (%.2f TB/s of %.2f GB)" % (k, prof[k][0], prof[k][2] / prof[k][0] / 1e9, prof[k][2] / 1e9) for k in ("row_reduce", "normalize")))
for t in types: pipes[t].close()

"""PCIe-inclusive rate of the hot path: the raw waterfalls start in HOST memory, so every step uploads them before it can
normalise (200 x 16.4 MB as float64).  Never the `value` of bench.py (that one starts with the frames resident in HBM);
DESIGN.md section 2 quotes this figure.

    python tools/pcie_inclusive.py [C3|C2] [--dtype f64|f32|u16|u8[,...]] [--pinned] [--steps K]

--dtype   the sample type the frames have on the host (default f64).  A comma-separated list runs the types INTERLEAVED in one process
          (step 0 of every type, then step 1 of every type, ...), so that the f64 leg is the yardstick of the same run.
--pinned  page-locked host frames: dsss_extract_many streams them in on the copy stream under the kernels; default is pageable
          memory, which dsss_frames_set copies before it returns.
The first step of every type is the warm-up (allocations); the line of a step prints the bytes that actually cross."""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from diasss_amd.pipeline import Pipeline
from diasss_amd.synth import Survey
NAMES = {"f64": "float64", "f32": "float32", "u16": "uint16", "u8": "uint8"}
ap = argparse.ArgumentParser()
ap.add_argument("workload", nargs="?", default="C3", choices=("C2", "C3"))
ap.add_argument("--dtype", default="f64")
ap.add_argument("--pinned", action="store_true")
ap.add_argument("--steps", type=int, default=3, help="measured steps per type, after one warm-up step")
a = ap.parse_args()
types = a.dtype.split(",")
if any(t not in NAMES for t in types):
    sys.exit("--dtype: f64, f32, u16 or u8")
types = sorted(set(types), key=list(NAMES).index)              # widest first: a context keeps the block of a frame's owned copy when the type narrows
F, N, M = {"C2": (50, 1000, 512), "C3": (200, 2000, 1024)}[a.workload]
sv = Survey(F, N, M, seed=20240601 + 1, device="cuda:0")
ins = [sv.inputs(f) for f in range(F)]
poses, alts, grs = [i[0] for i in ins], [i[1] for i in ins], [i[2] for i in ins]
host = {t: [] for t in types}                                    # host resident, in the sample type
for f in range(F):
    img = sv.frame(f)
    for t in types:
        h = sv.frame(f, NAMES[t]).cpu() if t != "f64" else img.cpu()
        host[t].append(h.pin_memory() if a.pinned else h.numpy())
    del img
pipe = Pipeline(F)
ms = {t: [] for t in types}
for it in range(a.steps + 1):
    for t in types:
        nbytes = sum(int(np.prod(h.shape)) * h.element_size() if a.pinned else h.nbytes for h in host[t])
        torch.cuda.synchronize(); t0 = time.perf_counter()
        pipe.run(host[t], poses, alts, grs)
        dt = time.perf_counter() - t0
        if it: ms[t].append(dt * 1e3)
        print("%s step %d%s: %.1f ms  -> %.0f frames/s with the upload of %.2f GB of %s host-resident %s frames inside the step"
              % (t, it, " (warm-up)" if it == 0 else "", dt * 1e3, F / dt, nbytes / 1e9, "page-locked" if a.pinned else "pageable", NAMES[t]), flush=True)
for t in types:
    v = sorted(ms[t])
    print("%s: median %.1f ms, min %.1f, max %.1f over %d steps" % (t, v[len(v) // 2], v[0], v[-1], len(v)))
pipe.close()

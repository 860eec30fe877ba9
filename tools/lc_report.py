#!/usr/bin/env python3
"""What the loop closures of a synthetic survey say about the trajectory they produced: the survey through the pipeline, then the residual
report (dsss_posegraph_edge_report) and the chi-square gated solve (dsss_posegraph_solve_gated) on the selected closures.
    python tools/lc_report.py --frames 200 --rows 2000 --cols 1024 [--gate 22.458] [--cell 0.1] [--calls 7]
Prints a chi2 histogram by decade (at the plain solve's result), the closures dropped per solve of the gated one, wall-clock times of the
report alone and of the gated solve next to the plain one (median of --calls synchronised calls after a warm-up), the mosaic consistency
score before and after gating, and one JSON line with all of it."""
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
ap.add_argument("--gate", type=float, default=None); ap.add_argument("--calls", type=int, default=7)
a = ap.parse_args()
F, N, M = a.frames, a.rows, a.cols

sv = Survey(F, N, M, seed=20240601 + 1, device="cuda:0")          # the survey of tools/mosaic_time.py
raws = [sv.frame(f) for f in range(F)]
ins = [sv.inputs(f) for f in range(F)]
pipe = Pipeline(F, device=0)
pipe.run(raws, [i[0] for i in ins], [i[1] for i in ins], [i[2] for i in ins])
ctx = pipe.ctx
dr = np.ascontiguousarray(np.concatenate([np.asarray(i[0].cpu() if hasattr(i[0], "cpu") else i[0], np.float64) for i in ins]))
edges = ctx.posegraph_select(F)
ne = len(edges)
gp = ctx.gate_params_default()
if a.gate is not None:
    gp.gate = a.gate


def rpy_rows(poses12):
    """the trajectory rows "r p y x y z" (Rot3::rpy, as dsss_posegraph_solve writes them) of poses12"""
    R = poses12
    out = np.empty((len(R), 6))
    out[:, 0] = np.arctan2(R[:, 7], R[:, 8]); out[:, 1] = np.arctan2(-R[:, 6], np.sqrt(R[:, 7] ** 2 + R[:, 8] ** 2)); out[:, 2] = np.arctan2(R[:, 3], R[:, 0])
    out[:, 3:] = R[:, 9:]
    return out


def median_ms(fn):
    fn(); ctx.sync()
    ts = []
    for _ in range(a.calls):
        ctx.sync(); t0 = time.perf_counter(); fn(); ctx.sync(); ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


plain, pstats = ctx.posegraph_solve_edges(dr, edges)
chi2, r6, sums = ctx.posegraph_edge_report(dr, edges, plain)
gated, gstats, keep, gchi2, n_solves = ctx.posegraph_solve_gated(dr, edges, gp)

print("%d poses, %d loop closures; plain solve: %d LM iterations, objective %.6g -> %.6g (chain %.6g + closures %.6g)"
      % (len(dr), ne, pstats[0], pstats[1], pstats[2], sums[0], sums[1]))
print("chi2 of the closures at the plain solve's result, by decade (gate %.3f):" % gp.gate)
hist = {}
if ne:
    dec = np.where(np.isfinite(chi2) & (chi2 > 0), np.floor(np.log10(np.maximum(chi2, 1e-300))), np.where(chi2 > 0, np.inf, -np.inf))
    for d in sorted(set(dec.tolist())):
        hist["1e%g" % d] = int((dec == d).sum())
        print("   [1e%g, 1e%g): %d" % (d, d + 1, hist["1e%g" % d]))
print("   above the gate: %d of %d" % (int((chi2 > gp.gate).sum()), ne))

# closures dropped per solve: the rule replayed with the report on the plain solver (the gated solve's own rounds, same bits)
dropped_per_solve = []
k = np.ones(ne, bool)
for s in range(n_solves - 1):
    p, _ = ctx.posegraph_solve_edges(dr, np.ascontiguousarray(edges[k]))
    c2, _, _ = ctx.posegraph_edge_report(dr, np.ascontiguousarray(edges[k]), p)
    c2 = np.where(np.isfinite(c2), c2, np.inf)
    thr = max(gp.gate, c2.max() / gp.decade)
    idx = np.flatnonzero(k); drop = idx[c2 > thr]
    k[drop] = False; dropped_per_solve.append(int(len(drop)))
assert (k == keep).all(), "the replayed rule and dsss_posegraph_solve_gated disagree"
print("gated solve: %d solves, dropped per solve %s, kept %d of %d; objective %.6g -> %.6g; largest chi2 kept %.4g"
      % (n_solves, dropped_per_solve, int(keep.sum()), ne, gstats[1], gstats[2], gchi2[keep].max() if keep.any() else 0.0))

ms_report = median_ms(lambda: ctx.posegraph_edge_report(dr, edges, plain))
ms_plain = median_ms(lambda: ctx.posegraph_solve_edges(dr, edges))
ms_gated = median_ms(lambda: ctx.posegraph_solve_gated(dr, edges, gp))
print("wall clock, median of %d after a warm-up: report %.3f ms, plain solve %.3f ms, gated solve %.3f ms (%d solves)"
      % (a.calls, ms_report, ms_plain, ms_gated, n_solves))

ids = np.arange(F, dtype=np.int32); off = ids * N
grid = capi.mosaic_grid(ctx.mosaic_bounds(ids), a.cell)
scores = {}
for name, traj in (("dr", {}), ("plain", dict(rpy6=rpy_rows(plain), ping_off=off)), ("gated", dict(rpy6=rpy_rows(gated), ping_off=off)),
                   ("true", dict(rpy6=np.ascontiguousarray(np.concatenate(sv.poses_true)), ping_off=off))):
    scores[name] = ctx.mosaic_consistency(ids, grid, **traj)[3]
print("mosaic consistency score (grey levels): dead reckoning %.2f, plain solve %.2f, gated solve %.2f, true poses %.2f"
      % (scores["dr"], scores["plain"], scores["gated"], scores["true"]))
print(json.dumps(dict(frames=F, rows=N, cols=M, poses=len(dr), closures=ne, gate=gp.gate, decade=gp.decade, max_solves=gp.max_solves, calls=a.calls,
                      chi2_hist=hist, above_gate=int((chi2 > gp.gate).sum()), solves=n_solves, dropped_per_solve=dropped_per_solve, kept=int(keep.sum()),
                      objective_plain=float(pstats[2]), objective_gated=float(gstats[2]), report_ms=round(ms_report, 3), plain_solve_ms=round(ms_plain, 3),
                      gated_solve_ms=round(ms_gated, 3), score_dr=scores["dr"], score_plain=scores["plain"], score_gated=scores["gated"], score_true=scores["true"],
                      max_pose_shift=float(np.abs(gated[:, 9:] - plain[:, 9:]).max()))))
pipe.close()

"""Numpy reference of the per-ping disagreement profile (include/dsss_profile.h), written from the definition and from nothing else.
Nothing in it calls the library.  Frames are the records tests/mosaic_footprint_ref.py takes (gx, gy, norm, mask, optional val for
gain-corrected levels), and the mask rule, the binning and the value of a sample are that file's _kept, _cells and _val, so a sample is
binned here iff the reference of the render bins it.  A = (S, C) is summed over all frames, A_f is the frame's own, the mosaic of the
others is (S - S_f, C - C_f) in int64, m = ((S - S_f) + (C - C_f) // 2) // (C - C_f) and d = v' - m."""
import math

import numpy as np

from tests.mosaic_footprint_ref import _cells, _kept, _val

REC = np.dtype([("binned", "<u4", (2,)), ("n", "<u4", (2,)), ("sad", "<u4", (2,)), ("ssd", "<u4", (2,)), ("sd", "<i4", (2,))])
NONE = -32768
INFO_FIELDS = ("pings", "binned", "n", "sad", "ssd", "sd", "rms")


def _own(fr, p, use_mask):
    """a frame's samples: cell and whether it is binned (N x M), the corrected values, and its own sum and count per cell"""
    cells = p.W * p.H
    ones = np.ones(fr["norm"].shape, bool)
    cell, ok = _cells(fr["gx"], fr["gy"], ones & _kept(fr, use_mask), p)
    val = _val(fr).astype(np.int64)
    s = np.bincount(cell[ok], weights=val[ok], minlength=cells).astype(np.int64)
    n = np.bincount(cell[ok], minlength=cells).astype(np.int64)
    return cell, ok, val, s, n


def summary(stats):
    """the records of a call summed -> dict of INFO_FIELDS; rms = n ? sqrt(ssd / n) : 0, one division and one square root in f64"""
    out = {"pings": int(len(stats))}
    for k in ("binned", "n", "sad", "ssd", "sd"):
        out[k] = int(stats[k].astype(np.int64).sum())
    out["rms"] = math.sqrt(float(out["ssd"]) / float(out["n"])) if out["n"] else 0.0
    return out


def profile(frames, p, use_mask, prof=None, min_count=1):
    """frames under the grid p; prof = indices into frames (None: all, in order) -> (stats, diff, info): the records of the profiled
    frames' pings one frame after the other (REC), their residual layers (a list of N x M int16, NONE where not compared) and the sums
    of the call"""
    assert 1 <= min_count <= 1 << 24
    own = [_own(fr, p, use_mask) for fr in frames]
    S = sum(o[3] for o in own); Cn = sum(o[4] for o in own)
    prof = list(range(len(frames))) if prof is None else list(prof)
    assert len(set(prof)) == len(prof) and all(0 <= k < len(frames) for k in prof)
    stats, diff = [], []
    for k in prof:
        cell, ok, val, s, n = own[k]
        oS, oC = S - s, Cn - n
        assert (oS >= 0).all() and (oC >= 0).all()                                 # the subtraction never borrows
        c_at, s_at = oC[cell], oS[cell]
        cmp = ok & (c_at >= min_count)
        m = (s_at + c_at // 2) // np.maximum(c_at, 1)
        d = np.where(cmp, val - m, 0)
        assert np.abs(d).max(initial=0) <= 255
        N, M = val.shape
        half = M // 2
        rec = np.zeros(N, REC)
        for side, sl in ((0, slice(0, half)), (1, slice(half, M))):
            rec["binned"][:, side] = ok[:, sl].sum(1)
            rec["n"][:, side] = cmp[:, sl].sum(1)
            rec["sad"][:, side] = np.abs(d[:, sl]).sum(1)
            ssd = (d[:, sl] * d[:, sl]).sum(1)
            assert ssd.max(initial=0) < 1 << 32
            rec["ssd"][:, side] = ssd
            rec["sd"][:, side] = d[:, sl].sum(1)
        stats.append(rec)
        diff.append(np.where(cmp, d, NONE).astype(np.int16))
    stats = np.concatenate(stats)
    return stats, diff, summary(stats)

"""The survey of the range-gain effect tests, shared by tests/test_mosaic_gain_cpu.py (the precondition, on the references alone) and
tests/test_gpu_mosaic_gain.py (the device against the same numbers): synth.Survey(2, 640, 400, seed=7) whose raw frames carry the
sensor profile of mosaic_gain_ref.profile(M, 0.6), binned under the TRUE poses at cell 0.1 with the mask on.  Everything expected is
the oracle's (normalize, mask, geo_img) and the numpy references'; nothing here calls the library.  Computed once per session."""
import math
import types

import numpy as np

from tests import mosaic_gain_ref as G
from tests import mosaic_register_ref as R

F, N, M, SEED, AMP, CELL = 2, 640, 400, 7, 0.6, 0.1
MIN_COUNT, SMOOTH, TARGET = 64, 0, 0
_CACHE = {}


def grid(xmin, xmax, ymin, ymax, cell, use_mask=1):
    """dsss_mosaic_grid's rule, restated: the grid that covers the box"""
    x0 = math.floor(xmin / cell) * cell; y0 = math.floor(ymin / cell) * cell
    return types.SimpleNamespace(x0=x0, y0=y0, cell=cell, W=int(math.floor((xmax - x0) / cell)) + 1, H=int(math.floor((ymax - y0) / cell)) + 1,
                                 use_mask=use_mask)


def consistency(frames, p, use_mask):
    """the consistency layers and score of frames = [(gx, gy, norm, mask), ...] from mean layers (mosaic_register_ref.mean_layer)"""
    nfr = np.zeros((p.H, p.W), np.int64); s1 = np.zeros_like(nfr); s2 = np.zeros_like(nfr)
    for gx, gy, norm, mask in frames:
        m, v = R.mean_layer(gx, gy, norm, mask, p, use_mask)
        nfr += v; s1 += np.where(v, m, 0); s2 += np.where(v, m * m, 0)
    sel = nfr >= 2
    num = (s2[sel].astype(np.float64) - s1[sel].astype(np.float64) ** 2 / nfr[sel].astype(np.float64)).sum()
    den = float((nfr[sel] - 1).sum())
    return nfr, s1, s2, (float(np.sqrt(num / den)) if den > 0 and num > 0 else 0.0)


def zncc0(frames, p, use_mask, min_cells=1):
    """the score at zero shift of frame 1 against frame 0"""
    (ma, va), (mb, vb) = (R.mean_layer(gx, gy, norm, mask, p, use_mask) for gx, gy, norm, mask in frames[:2])
    return R.score(R.shift_sums(ma, va, mb, vb, 0)[0, 0], min_cells)[0]


def effect_case(orc):
    """dict(sv, raws (with the profile), flat (the same frames without), legs = [dict(gx, gy, norm, mask)] for both, p = the grid,
    S, C, gain, T = the statistics and the table of the profiled frames by the reference, corrected = their corrected grey levels)"""
    if "case" in _CACHE:
        return _CACHE["case"]
    from diasss_amd.synth import Survey
    sv = Survey(F, N, M, seed=SEED)
    prof = G.profile(M, AMP)
    flat = [sv.frame(f).numpy() for f in range(F)]
    raws = [np.ascontiguousarray(r * prof[None, :]) for r in flat]
    geo = [orc.geo_img(sv.poses_true[f], sv.gr, M) for f in range(F)]

    def legs_of(rs):
        return [dict(gx=geo[f][0], gy=geo[f][1], norm=orc.normalize(rs[f]), mask=orc.mask(rs[f])) for f in range(F)]
    legs, legs_flat = legs_of(raws), legs_of(flat)
    gx = np.concatenate([g[0].ravel() for g in geo]); gy = np.concatenate([g[1].ravel() for g in geo])
    p = grid(gx.min(), gx.max(), gy.min(), gy.max(), CELL)
    S, C = G.col_stats([(L["norm"], L["mask"]) for L in legs], 1)
    gain, T = G.table(S, C, M, MIN_COUNT, SMOOTH, TARGET)
    out = dict(sv=sv, raws=raws, flat=flat, legs=legs, legs_flat=legs_flat, p=p, S=S, C=C, gain=gain, T=T,
               corrected=[G.apply(L["norm"], gain) for L in legs])
    _CACHE["case"] = out
    return out


def frames_of(legs, norms=None):
    return [(L["gx"], L["gy"], L["norm"] if norms is None else norms[i], L["mask"]) for i, L in enumerate(legs)]

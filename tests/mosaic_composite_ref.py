"""Numpy reference of the composite mosaic (include/dsss.h, "composite mosaic"), written from the definition and from nothing else.
Nothing in it calls the library: geo coordinates, grey levels and masks are handed in (the oracle's), the binning is
np.floor((g - origin) / cell) as in tests/test_gpu_mosaic.py, the winner of a cell comes from np.lexsort over (q, g, col), the gain
correction is tests/mosaic_gain_ref.apply, and the fill walks the offsets of the square in the order (d2, dy, dx)."""
import numpy as np

from tests import mosaic_gain_ref as G

NEAR, FAR, MID, FIRST = 0, 1, 2, 3
MODES = (NEAR, FAR, MID, FIRST)
LAYERS = ("img", "src_frame", "src_ping", "src_col", "fill")


def ground_index(M, col):
    """the ground-range index of a column: bins of a side counted from the nadir; the port columns 0 and 1 share the last one"""
    half = M // 2
    return col - half if col >= half else min(half - col, half - 1)


def rank(mode, M, col):
    """the priority rank q of a column, smaller wins"""
    half, idx = M // 2, ground_index(M, col)
    return {NEAR: idx, FAR: half - 1 - idx, MID: abs(2 * idx - (half - 1)), FIRST: 0}[mode]


def ranks(mode, M):
    return np.array([rank(mode, M, c) for c in range(M)], np.int64)


def samples(frames, p, use_mask, mode, gain=None):
    """frames: dicts with id, gx, gy, norm, mask and optionally keep (bool per ping: False drops the ping, as a non-finite pose row
    does) -> the samples that fall on the grid, one array per attribute: cell, q, g, col, val, frame, ping.  g is counted over the
    frames in the order of their ids, whatever the order of the list."""
    out = {k: [] for k in ("cell", "q", "g", "col", "val", "frame", "ping")}
    g0 = 0
    for fr in sorted(frames, key=lambda f: f["id"]):
        N, M = fr["norm"].shape
        with np.errstate(invalid="ignore", over="ignore"):
            fx = np.floor((fr["gx"] - p.x0) / p.cell); fy = np.floor((fr["gy"] - p.y0) / p.cell)
            ok = (fx >= 0) & (fx < p.W) & (fy >= 0) & (fy < p.H)
        if use_mask:
            ok &= fr["mask"] != 0
        if fr.get("keep") is not None:
            ok &= fr["keep"][:, None]
        rows, cols = np.nonzero(ok)
        val = fr["norm"] if gain is None else G.apply(fr["norm"], gain)
        out["cell"].append(fy[ok].astype(np.int64) * p.W + fx[ok].astype(np.int64))
        out["q"].append(ranks(mode, M)[cols]); out["g"].append(g0 + rows); out["col"].append(cols)
        out["val"].append(val[ok].astype(np.int64)); out["frame"].append(np.full(len(rows), fr["id"], np.int64)); out["ping"].append(rows)
        g0 += N
    return {k: np.concatenate(v).astype(np.int64) for k, v in out.items()}


def winners(frames, p, use_mask, mode, gain=None):
    """-> (layers, stats): layers img, src_frame, src_ping, src_col (int64, H x W; 0 / -1 where empty) and valid (bool); stats:
    ties_q = the cells whose runner-up has the winner's q (g decides there), ties_qg = those where it has the winner's g too (col
    decides), contended = the cells with more than one sample, fullest = the most samples of a cell"""
    S = samples(frames, p, use_mask, mode, gain)
    o = np.lexsort((S["col"], S["g"], S["q"], S["cell"]))
    cs = S["cell"][o]
    first = np.ones(len(o), bool); first[1:] = cs[1:] != cs[:-1]
    w = o[first]
    second = np.nonzero(~first & np.r_[False, first[:-1]])[0]                  # the runner-up of every cell that has one
    sq = S["q"][o[second]] == S["q"][o[second - 1]]
    sg = sq & (S["g"][o[second]] == S["g"][o[second - 1]])
    cells = p.W * p.H
    lay = dict(img=np.zeros(cells, np.int64), src_frame=np.full(cells, -1, np.int64), src_ping=np.full(cells, -1, np.int64),
               src_col=np.full(cells, -1, np.int64), valid=np.zeros(cells, bool))
    c = S["cell"][w]
    lay["img"][c] = S["val"][w]; lay["src_frame"][c] = S["frame"][w]; lay["src_ping"][c] = S["ping"][w]; lay["src_col"][c] = S["col"][w]
    lay["valid"][c] = True
    stats = dict(ties_q=int(sq.sum()), ties_qg=int(sg.sum()), contended=len(second),
                 fullest=int(np.bincount(S["cell"]).max()) if len(o) else 0, samples=len(o))
    return {k: v.reshape(p.H, p.W) for k, v in lay.items()}, stats


def fill(valid, R):
    """the gap fill of a layer of validity flags (bool H x W) -> (donor, fill): donor = the cell index iy W + ix a cell takes its value
    from (its own in V0, -1 where it stays empty), fill = 0 in V0, the donor's dx^2 + dy^2 for a filled cell, 255 for one left empty"""
    valid = np.asarray(valid) != 0
    H, W = valid.shape
    V = np.zeros((H + 2 * R, W + 2 * R), bool); V[R:R + H, R:R + W] = valid          # cells outside the grid are not in V0

    def at(dx, dy):
        return V[R + dy:R + dy + H, R + dx:R + dx + W]
    none = np.zeros((H, W), bool)
    left = none.copy(); right = none.copy(); up = none.copy(); down = none.copy()
    for a in range(1, R + 1):
        left |= at(-a, 0); right |= at(a, 0); up |= at(0, -a); down |= at(0, a)
    todo = ~valid & ((left & right) | (up & down))
    index = np.arange(H * W, dtype=np.int64).reshape(H, W)
    donor = np.where(valid, index, -1); fl = np.where(valid, 0, 255).astype(np.int64)
    for d2, dy, dx in sorted((dx * dx + dy * dy, dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)):
        hit = todo & at(dx, dy)
        donor[hit] = index[hit] + dy * W + dx; fl[hit] = d2
        todo &= ~hit
    assert not todo.any(), "an enclosed cell without a donor"
    return donor, fl


def composite(frames, p, use_mask, mode, R=0, gain=None):
    """-> (layers, info, stats): the five layers of dsss_mosaic_composite (int64), info = (direct, filled, empty)"""
    lay, stats = winners(frames, p, use_mask, mode, gain)
    donor, fl = fill(lay["valid"], R)
    take = donor >= 0
    out = {}
    for k, empty in (("img", 0), ("src_frame", -1), ("src_ping", -1), ("src_col", -1)):
        out[k] = np.where(take, lay[k].ravel()[np.maximum(donor, 0)], empty)
    out["fill"] = fl
    direct = int(lay["valid"].sum()); filled = int((take & ~lay["valid"]).sum())
    return out, (direct, filled, p.W * p.H - direct - filled), stats

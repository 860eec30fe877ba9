"""Numpy / Python-integer reference of the dense loop closures over a cell pyramid (include/dsss.h, "dense loop closures over a cell
pyramid"), written from the definition and from nothing else: the level-0 accumulators binned as tests/mosaic_register_ref.py bins
them, pooled by reshape, the shift sums around a centre by slicing, peak, centroid and edges from tests/mosaic_register_ref.py and
tests/register_edges_ref.py, the level rule written again here."""
import numpy as np

from tests import mosaic_register_ref as R
from tests import register_edges_ref as E

REFINE = 3                                  # the default of dsss_reg_pyr_params.refine

# the moved survey of the tests: legs 0 and 1 of synth.Survey(2, 640, 400, seed=7) under their true poses on a grid of CELL metres,
# leg 1 moved by MOVE metres (inside the capture range of three levels, radius 8: 32 cells) or by FAR (beyond the top level's radius)
CELL, SEG, RADIUS, MIN_CELLS = 0.1, 80, 8, 256
MOVE, MOVE_CELLS = (2.3, -1.7), (23, -17)
FAR, FAR_CELLS = (-3.1, 2.6), (-31, 26)


def accumulators(gx, gy, norm, mask, p, use_mask, keep_rows=None):
    """the level-0 accumulators of one frame (or of the pings keep_rows of it) over the grid p -> (cnt, sum), int64 H x W"""
    W, H = p.W, p.H
    with np.errstate(invalid="ignore", over="ignore"):
        fx = np.floor((gx - p.x0) / p.cell); fy = np.floor((gy - p.y0) / p.cell)
        ok = (fx >= 0) & (fx < W) & (fy >= 0) & (fy < H)
    if use_mask:
        ok &= mask != 0
    if keep_rows is not None:
        ok &= keep_rows[:, None]
    idx = fy[ok].astype(np.int64) * W + fx[ok].astype(np.int64)
    s = np.zeros(W * H, np.int64); c = np.zeros(W * H, np.int64)
    np.add.at(s, idx, norm[ok].astype(np.int64)); np.add.at(c, idx, 1)
    return c.reshape(H, W), s.reshape(H, W)


def segment_accumulators(gx, gy, norm, mask, p, p0, p1):
    """accumulators() of the pings [p0, p1) alone"""
    keep = np.zeros(gx.shape[0], bool); keep[p0:p1] = True
    return accumulators(gx, gy, norm, mask, p, p.use_mask, keep_rows=keep)


def pool(cnt, sm, l):
    """level l: the sums of cnt and of sum over the cells with ix >> l == jx, iy >> l == jy -> (cnt_l, sum_l), ceil(H / 2^l) x ceil(W / 2^l)"""
    f = 1 << l
    H, W = cnt.shape
    Hl, Wl = -(-H // f), -(-W // f)
    out = []
    for a in (cnt, sm):
        big = np.zeros((Hl * f, Wl * f), np.int64); big[:H, :W] = a
        out.append(big.reshape(Hl, f, Wl, f).sum(axis=(1, 3)))
    return out[0], out[1]


def layer(cnt, sm):
    """(m, valid): m = (sum + cnt // 2) // cnt where cnt > 0"""
    return np.where(cnt > 0, (sm + cnt // 2) // np.maximum(cnt, 1), 0), cnt > 0


def pyramid(cnt, sm, levels):
    """[(m, valid) of level 0, 1, ...]"""
    return [layer(*pool(cnt, sm, l)) for l in range(levels)]


def centred_sums(ma, va, mb, vb, cx, cy, radius):
    """(2 r + 1, 2 r + 1, 6) int64, [dy + r, dx + r] = n, Sa, Sb, Sab, Saa, Sbb over the cells (ix, iy) where a is valid and b is valid at
    (ix + cx + dx, iy + cy + dy); cells outside the layers are invalid.  a is cut to the cells that can meet a valid cell of b at all."""
    H, W = ma.shape
    S = 2 * radius + 1
    out = np.zeros((S, S, 6), np.int64)
    ys, xs = np.nonzero(vb)
    if len(ys) == 0:
        return out
    ax0, ax1 = max(0, xs.min() - cx - radius), min(W, xs.max() - cx + radius + 1)
    ay0, ay1 = max(0, ys.min() - cy - radius), min(H, ys.max() - cy + radius + 1)
    ma = ma.astype(np.int64); mb = mb.astype(np.int64)
    for dy in range(-radius, radius + 1):
        ty = cy + dy
        y0, y1 = max(ay0, -ty), min(ay1, H - ty)
        for dx in range(-radius, radius + 1):
            tx = cx + dx
            x0, x1 = max(ax0, -tx), min(ax1, W - tx)
            if y1 <= y0 or x1 <= x0:
                continue
            V = va[y0:y1, x0:x1] & vb[y0 + ty:y1 + ty, x0 + tx:x1 + tx]
            A = ma[y0:y1, x0:x1][V]; B = mb[y0 + ty:y1 + ty, x0 + tx:x1 + tx][V]
            out[dy + radius, dx + radius] = (int(V.sum()), int(A.sum()), int(B.sum()), int((A * B).sum()), int((A * A).sum()), int((B * B).sum()))
    return out


def step(sums, radius, min_cells, cell, level, cx, cy):
    """the level rule on the table of level `level` around the centre (cx, cy) -> (record, usable, next centre or None); min_cells and
    cell are the level-0 values.  Without a usable shift the record is R.peak's, unchanged."""
    cell_l = cell * float(2 ** level)
    rec = R.peak(sums, radius, max(1, min_cells >> (2 * level)), cell_l)
    if rec["zncc"] == -2.0:
        return rec, False, None
    out = dict(rec)
    out["dx"] = cx + rec["dx"]; out["dy"] = cy + rec["dy"]
    out["off_x"] = rec["off_x"] + float(cx) * cell_l; out["off_y"] = rec["off_y"] + float(cy) * cell_l
    return out, True, ((2 * out["dx"], 2 * out["dy"]) if level > 0 else None)


def register_row(pyr_a, pyr_b, cell, radius, min_cells, levels, refine):
    """one (a, segment) row from the two pyramids -> dict: sums (the top level's table, then those of the levels below, one behind the
    other as rows of six; zero where a level was not reached), level, border_mask, lx, ly, lz, r, sx, sy"""
    nt, nr = (2 * radius + 1) ** 2, (2 * refine + 1) ** 2
    sums = np.zeros((nt + (levels - 1) * nr, 6), np.int64)
    row = dict(level=-1, border_mask=0, lx=[0] * 4, ly=[0] * 4, lz=[-2.0] * 4, sx=0, sy=0)
    cx = cy = 0
    at = 0
    for l in range(levels - 1, -1, -1):
        r = radius if l == levels - 1 else refine
        (ma, va), (mb, vb) = pyr_a[l], pyr_b[l]
        T = centred_sums(ma, va, mb, vb, cx, cy, r)
        sums[at:at + (2 * r + 1) ** 2] = T.reshape(-1, 6); at += (2 * r + 1) ** 2
        rec, usable, nxt = step(T, r, min_cells, cell, l, cx, cy)
        if not usable:
            if l == levels - 1:
                row["r"] = rec
            break
        row["r"] = rec; row["level"] = l
        row["lx"][l], row["ly"][l], row["lz"][l] = rec["dx"], rec["dy"], rec["zncc"]
        row["border_mask"] |= rec["on_border"] << l
        if l > 0:
            cx, cy = nxt
    if row["level"] >= 0:
        row["r"] = dict(row["r"], on_border=int(row["border_mask"] != 0 or row["level"] != 0))
    if row["level"] == 0:
        n, row["sx"], row["sy"] = E.centroid_sums(pyr_a[0][1], pyr_b[0][1], row["r"]["dx"], row["r"]["dy"])
        assert n == row["r"]["n"]
    row["sums"] = sums
    return row


def register_segments_pyr(acc_a, gx, gy, norm, mask, p, seg_pings, radius, min_cells, levels, refine):
    """frame b (geo gx, gy; grey levels; mask) cut into segments, each against the whole frame a with the accumulators acc_a = (cnt, sum)
    -> one dict per segment: seg, p0, p1 and the fields of register_row()"""
    pyr_a = pyramid(acc_a[0], acc_a[1], levels)
    out = []
    for s, (p0, p1) in enumerate(E.segments(gx.shape[0], seg_pings)):
        pyr_b = pyramid(*segment_accumulators(gx, gy, norm, mask, p, p0, p1), levels)
        out.append(dict(register_row(pyr_a, pyr_b, p.cell, radius, min_cells, levels, refine), seg=s, p0=p0, p1=p1))
    return out


def best_other(sums, radius, min_cells, dx, dy):
    """the largest ZNCC of a usable shift of the table other than (dx, dy) (relative to the table's centre), -2 when there is none"""
    z = R.scores(sums, radius, min_cells)
    return max([z[j][i][0] for j in range(2 * radius + 1) for i in range(2 * radius + 1) if z[j][i][1] and (i - radius, j - radius) != (dx, dy)], default=-2.0)


def segment_windows(gx, gy, p, seg_pings):
    """per segment the first cell (ox, oy) of the grid its geo extremes reach (clipped to the grid), as the library cuts its windows"""
    out = []
    for p0, p1 in E.segments(gx.shape[0], seg_pings):
        x, y = gx[p0:p1], gy[p0:p1]
        ok = np.isfinite(x) & np.isfinite(y)
        out.append((max(0, int(np.floor((x[ok].min() - p.x0) / p.cell))), max(0, int(np.floor((y[ok].min() - p.y0) / p.cell)))))
    return out


def awkward_grid(make, bbox, cell, gx, gy, seg_pings):
    """the grid of the bounding box moved and cut so that W and H are no multiples of 4 and some segment of the frame with the geo
    coordinates gx, gy starts on an odd cell in x and some segment on an odd cell in y: make(x0, y0, cell, W, H) -> the parameters"""
    x0 = np.floor(bbox[0] / cell) * cell; y0 = np.floor(bbox[2] / cell) * cell
    W = int(np.floor((bbox[1] - x0) / cell)) + 1; H = int(np.floor((bbox[3] - y0) / cell)) + 1
    for kx in range(2):
        for ky in range(2):
            p = make(x0 - kx * cell, y0 - ky * cell, cell, W + kx, H + ky)
            while p.W % 4 == 0:
                p.W -= 1
            while p.H % 4 == 0:
                p.H -= 1
            w = segment_windows(gx, gy, p, seg_pings)
            if any(ox % 2 for ox, _ in w) and any(oy % 2 for _, oy in w):
                return p
    raise AssertionError("no grid with a segment window on an odd cell")

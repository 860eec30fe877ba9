"""Numpy / Python-integer reference of the dense overlap registration (include/dsss.h, "overlap registration"), written from the
definition and from nothing else: binning as in tests/test_gpu_mosaic.py, shift sums with slices, score and peak with Python integers
and math.sqrt (the three integers exact, then float() once each: float() of an int rounds to nearest, ties to even)."""
import math
import numpy as np


def mean_layer(gx, gy, norm, mask, p, use_mask, keep_rows=None):
    """one frame's mean layer over the grid p -> (m int64 H x W, valid bool H x W); m = (sum + cnt // 2) // cnt where cnt > 0"""
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
    m = np.where(c > 0, (s + c // 2) // np.maximum(c, 1), 0)
    return m.reshape(H, W), (c > 0).reshape(H, W)


def shift_sums(ma, va, mb, vb, radius):
    """(2 r + 1, 2 r + 1, 6) int64, [dy + r, dx + r] = n, Sa, Sb, Sab, Saa, Sbb over the cells where a is valid and b is valid at the
    shifted cell; cells outside the layers are invalid"""
    H, W = ma.shape
    S = 2 * radius + 1
    out = np.zeros((S, S, 6), np.int64)
    ma = ma.astype(np.int64); mb = mb.astype(np.int64)
    for dy in range(-radius, radius + 1):
        y0, y1 = max(0, -dy), min(H, H - dy)
        for dx in range(-radius, radius + 1):
            x0, x1 = max(0, -dx), min(W, W - dx)
            if y1 <= y0 or x1 <= x0:
                continue
            V = va[y0:y1, x0:x1] & vb[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
            A = ma[y0:y1, x0:x1][V]; B = mb[y0 + dy:y1 + dy, x0 + dx:x1 + dx][V]
            out[dy + radius, dx + radius] = (int(V.sum()), int(A.sum()), int(B.sum()), int((A * B).sum()), int((A * A).sum()), int((B * B).sum()))
    return out


def score(s6, min_cells):
    """(zncc, usable) of one shift from its six sums, exact integers up to one float() each"""
    n, Sa, Sb, Sab, Saa, Sbb = (int(v) for v in s6)
    num = n * Sab - Sa * Sb; da = n * Saa - Sa * Sa; db = n * Sbb - Sb * Sb
    if n < min_cells or da <= 0 or db <= 0:
        return -2.0, False
    return float(num) / math.sqrt(float(da) * float(db)), True


def scores(sums, radius, min_cells):
    S = 2 * radius + 1
    sums = np.asarray(sums).reshape(S, S, 6)
    return [[score(sums[j, i], min_cells) for i in range(S)] for j in range(S)]


def peak(sums, radius, min_cells, cell):
    """the result record as a dict with the fields of dsss_reg_result"""
    S = 2 * radius + 1
    sums = np.asarray(sums).reshape(S, S, 6)
    z = scores(sums, radius, min_cells)
    usable = [(-z[dy + radius][dx + radius][0], dx * dx + dy * dy, dy, dx)
              for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1) if z[dy + radius][dx + radius][1]]
    res = dict(dx=0, dy=0, off_x=0.0, off_y=0.0, zncc=-2.0, zncc0=z[radius][radius][0], n=int(sums[radius, radius, 0]), n0=int(sums[radius, radius, 0]),
               on_border=0)
    if not usable:
        return res
    _, _, dy, dx = min(usable)
    j, i = dy + radius, dx + radius
    z0 = z[j][i][0]
    res.update(dx=dx, dy=dy, zncc=z0, n=int(sums[j, i, 0]), on_border=int(abs(dx) == radius or abs(dy) == radius))
    px = py = 0.0
    if not res["on_border"]:
        (zm, okm), (zp, okp) = z[j][i - 1], z[j][i + 1]
        if okm and okp and zm - 2.0 * z0 + zp < 0.0:
            px = 0.5 * (zm - zp) / (zm - 2.0 * z0 + zp)
        (zm, okm), (zp, okp) = z[j - 1][i], z[j + 1][i]
        if okm and okp and zm - 2.0 * z0 + zp < 0.0:
            py = 0.5 * (zm - zp) / (zm - 2.0 * z0 + zp)
    res["off_x"] = (float(dx) + px) * cell; res["off_y"] = (float(dy) + py) * cell
    return res


FIELDS = ("dx", "dy", "off_x", "off_y", "zncc", "zncc0", "n", "n0", "on_border")


def same_result(dev, ref):
    """bit equality of a result of the library (a RegResult or a row of REG_DTYPE) with the reference's dict"""
    def get(k):
        return dev[k] if isinstance(dev, (np.void, np.ndarray)) else getattr(dev, k)
    for k in FIELDS:
        d, r = get(k), ref[k]
        if isinstance(r, float):
            if np.float64(d).tobytes() != np.float64(r).tobytes():
                return False
        elif int(d) != r:
            return False
    return True

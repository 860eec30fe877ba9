"""Numpy reference of the footprint rendering (include/dsss.h, "footprint rendering"), written from the definition and from nothing
else.  Nothing in it calls the library: geo coordinates, grey levels and masks are handed in (the oracle's), the steps are single f64
subtractions of them, a sub-sample is x + (i / na) Ax + (j / nc) Bx in separate numpy operations (numpy fuses nothing), the binning is
np.floor((g - origin) / cell) as everywhere in the mosaic tests, the winner of a cell comes from np.lexsort over (q, g, col) and the
fill is tests/mosaic_composite_ref.fill.  Parameters are a pair (max_steps, max_gap)."""
import numpy as np

from tests import mosaic_composite_ref as CR

DEFAULTS = (4, 1.0)


def steps(params, cell, sx, sy):
    """the sub-samples along the step (sx, sy), scalars or arrays -> int64 of their shape"""
    max_steps, max_gap = params
    sx = np.asarray(sx, np.float64); sy = np.asarray(sy, np.float64)
    with np.errstate(all="ignore"):
        finite = np.isfinite(sx) & np.isfinite(sy)
        l = np.maximum(np.abs(sx), np.abs(sy))
        t = np.ceil(l / np.float64(cell))
        one = ~finite | (l > np.float64(max_gap)) | (t < 1.0)
        n = np.where(one, 1.0, np.where(t > float(max_steps), float(max_steps), t))
    return n.astype(np.int64)


def along(g):
    """the along step of one coordinate layer (N x M): to the next ping; the last ping takes the step before it; one ping: 0"""
    N = g.shape[0]
    A = np.zeros_like(g)
    if N > 1:
        with np.errstate(invalid="ignore"):
            A[:-1] = g[1:] - g[:-1]
            A[-1] = g[-1] - g[-2]
    return A


def across(g):
    """the across step of one coordinate layer: outward on the column's own side"""
    N, M = g.shape
    half = M // 2
    B = np.empty_like(g)
    with np.errstate(invalid="ignore"):
        for c in range(M):
            idx = CR.ground_index(M, c)
            if idx < half - 1:
                B[:, c] = g[:, c + 1 if c >= half else c - 1] - g[:, c]
            else:                                                    # the outermost index: starboard M - 1, port 0 and 1
                B[:, c] = g[:, c] - g[:, M - 2 if c >= half else 2]
    return B


def step_counts(gx, gy, cell, params):
    """-> (Ax, Ay, Bx, By, na, nc), each N x M"""
    Ax, Ay, Bx, By = along(gx), along(gy), across(gx), across(gy)
    return Ax, Ay, Bx, By, steps(params, cell, Ax, Ay), steps(params, cell, Bx, By)


def expand(gx, gy, cell, params):
    """-> (layers, na, nc): layers = a generator of (i, j, X, Y, live) over the (i, j) that some sample has, X, Y = the sub-sample points
    (N x M, f64) and live = i < na and j < nc (bool, N x M: where the layer holds a sub-sample); layer (0, 0) is gx, gy themselves"""
    Ax, Ay, Bx, By, na, nc = step_counts(gx, gy, cell, params)

    def layers():
        fa = na.astype(np.float64); fc = nc.astype(np.float64)
        for i in range(int(na.max())):
            for j in range(int(nc.max())):
                live = (i < na) & (j < nc)
                if not live.any():
                    continue
                X, Y = gx, gy
                with np.errstate(all="ignore"):
                    if i > 0:
                        q = np.float64(i) / fa
                        X = X + q * Ax; Y = Y + q * Ay
                    if j > 0:
                        q = np.float64(j) / fc
                        X = X + q * Bx; Y = Y + q * By
                yield i, j, X, Y, live
    return layers(), na, nc


def _cells(X, Y, live, p):
    """the cell of every sub-sample of a layer and whether it is binned: live, finite and on the grid"""
    with np.errstate(invalid="ignore", over="ignore"):
        fx = np.floor((X - p.x0) / p.cell); fy = np.floor((Y - p.y0) / p.cell)
        ok = live & (fx >= 0) & (fx < p.W) & (fy >= 0) & (fy < p.H)
    cell = np.zeros(X.shape, np.int64)
    cell[ok] = fy[ok].astype(np.int64) * p.W + fx[ok].astype(np.int64)
    return cell, ok


def _kept(fr, use_mask):
    keep = (fr["mask"] != 0) if use_mask else np.ones(fr["norm"].shape, bool)
    if fr.get("keep") is not None:
        keep = keep & fr["keep"][:, None]
    return keep


def _val(fr):
    """the grey levels that are binned: fr["val"] (the levels corrected by a gain table, handed in) or the normalised image"""
    return fr["val"] if fr.get("val") is not None else fr["norm"]


def render(frames, p, use_mask, params):
    """frames: dicts with gx, gy, norm, mask (and optionally val, keep) -> (sum, cnt, img), int64 H x W, over the sub-samples;
    img = cnt ? (sum + cnt // 2) // cnt : 0.  Also returns the number of sub-samples binned."""
    cells = p.W * p.H
    s = np.zeros(cells, np.int64); n = np.zeros(cells, np.int64)
    for fr in frames:
        keep = _kept(fr, use_mask); val = _val(fr).astype(np.int64)
        for i, j, X, Y, live in expand(fr["gx"], fr["gy"], p.cell, params)[0]:
            cell, ok = _cells(X, Y, live & keep, p)
            s += np.bincount(cell[ok], weights=val[ok], minlength=cells).astype(np.int64)
            n += np.bincount(cell[ok], minlength=cells)
    img = np.where(n > 0, (s + n // 2) // np.maximum(n, 1), 0)
    return s.reshape(p.H, p.W), n.reshape(p.H, p.W), img.reshape(p.H, p.W), int(n.sum())


def composite(frames, p, use_mask, mode, R, params):
    """frames additionally with id -> (layers, info): the five layers of dsss_mosaic_composite_footprint (int64) and (direct, filled,
    empty).  A sub-sample carries its parent's (q, g, col), value and source; g counts the pings over the frames in the order of their
    ids."""
    out = {k: [] for k in ("cell", "q", "g", "col", "val", "frame", "ping")}
    g0 = 0
    for fr in sorted(frames, key=lambda f: f["id"]):
        N, M = fr["norm"].shape
        keep = _kept(fr, use_mask); val = _val(fr).astype(np.int64); q = CR.ranks(mode, M)
        for i, j, X, Y, live in expand(fr["gx"], fr["gy"], p.cell, params)[0]:
            cell, ok = _cells(X, Y, live & keep, p)
            rows, cols = np.nonzero(ok)
            out["cell"].append(cell[ok]); out["q"].append(q[cols]); out["g"].append(g0 + rows); out["col"].append(cols)
            out["val"].append(val[ok]); out["frame"].append(np.full(len(rows), fr["id"], np.int64)); out["ping"].append(rows)
        g0 += N
    S = {k: np.concatenate(v).astype(np.int64) if v else np.zeros(0, np.int64) for k, v in out.items()}
    o = np.lexsort((S["col"], S["g"], S["q"], S["cell"]))
    cs = S["cell"][o]
    first = np.ones(len(o), bool); first[1:] = cs[1:] != cs[:-1]
    w = o[first]
    cells = p.W * p.H
    lay = dict(img=np.zeros(cells, np.int64), src_frame=np.full(cells, -1, np.int64), src_ping=np.full(cells, -1, np.int64),
               src_col=np.full(cells, -1, np.int64))
    valid = np.zeros(cells, bool)
    c = S["cell"][w]
    lay["img"][c] = S["val"][w]; lay["src_frame"][c] = S["frame"][w]; lay["src_ping"][c] = S["ping"][w]; lay["src_col"][c] = S["col"][w]
    valid[c] = True
    valid = valid.reshape(p.H, p.W)
    donor, fl = CR.fill(valid, R)
    take = donor >= 0
    res = {k: np.where(take, v[np.maximum(donor, 0)], 0 if k == "img" else -1) for k, v in lay.items()}
    res["fill"] = fl
    direct = int(valid.sum()); filled = int((take & ~valid).sum())
    return res, (direct, filled, cells - direct - filled)


def holes(cnt):
    """(empty cells, enclosed single-cell holes) of a count layer: an empty cell with a cell that holds a sample directly on both sides
    of it, along x or along y -- what the composite's fill closes at radius 1"""
    valid = np.asarray(cnt) > 0
    fl = CR.fill(valid, 1)[1]
    return int((~valid).sum()), int(((fl > 0) & (fl < 255)).sum())

"""Numpy reference of the dense loop closures (include/dsss.h, "dense loop closures"), written from the definition and from nothing else:
segment layers and shift sums with tests/mosaic_register_ref.py, the centroid sums with numpy integers, acceptance, anchor pings and
the edge with np.cos / np.sin and the oracle's Rodrigues pose (orc.pose12); 4 x 4 matrices for the pose products."""
import numpy as np

from tests import mosaic_register_ref as R

MIN_ZNCC, SIGMA_XY_CELLS, SIGMA_Z, SIGMA_ROT = 0.5, 1.0, 10.0, 1.0          # the defaults of dsss_reg_edge_params


def segments(N, seg_pings):
    """[(p0, p1), ...]: ceil(N / seg_pings) segments, the last one short when seg_pings does not divide N"""
    return [(s, min(s + seg_pings, N)) for s in range(0, N, seg_pings)]


def segment_layer(gx, gy, norm, mask, p, p0, p1):
    """mean layer of the pings [p0, p1) alone.  keep_rows drops every other ping; the pings far from the segment are cut off before,
    which changes nothing and keeps a frame of many short segments affordable"""
    q0, q1 = max(0, p0 - 1), min(gx.shape[0], p1 + 1)
    keep = np.zeros(q1 - q0, bool); keep[p0 - q0:p1 - q0] = True
    return R.mean_layer(gx[q0:q1], gy[q0:q1], norm[q0:q1], mask[q0:q1], p, p.use_mask, keep_rows=keep)


def shift_sums(ma, va, mb, vb, radius):
    """R.shift_sums, evaluated on the bounding box of b's valid cells dilated by the radius: a cell of a outside that box has no valid
    partner at any shift, so the sums are the same and a short segment costs what its own box costs"""
    S = 2 * radius + 1
    ys, xs = np.nonzero(vb)
    if len(ys) == 0:
        return np.zeros((S, S, 6), np.int64)
    H, W = vb.shape
    y0, y1 = max(0, ys.min() - radius), min(H, ys.max() + radius + 1)
    x0, x1 = max(0, xs.min() - radius), min(W, xs.max() + radius + 1)
    return R.shift_sums(ma[y0:y1, x0:x1], va[y0:y1, x0:x1], mb[y0:y1, x0:x1], vb[y0:y1, x0:x1], radius)


def centroid_sums(va, vb, dx, dy):
    """(n, sx, sy) over V = the cells (ix, iy) where a is valid and b is valid at (ix + dx, iy + dy); cells outside the grid are invalid"""
    H, W = va.shape
    sh = np.zeros((H, W), bool)
    y0, y1 = max(0, -dy), min(H, H - dy); x0, x1 = max(0, -dx), min(W, W - dx)
    if y1 > y0 and x1 > x0:
        sh[y0:y1, x0:x1] = vb[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    iy, ix = np.nonzero(va & sh)
    return len(ix), int(ix.sum(dtype=np.int64)), int(iy.sum(dtype=np.int64))


def register_segments(lay_a, gx, gy, norm, mask, p, seg_pings, radius, min_cells):
    """frame b (geo gx, gy; grey levels; mask) cut into segments, each against the whole layer lay_a = (m, valid) of frame a ->
    one dict per segment: seg, p0, p1, sums, r (the dict of R.peak), sx, sy"""
    out = []
    for s, (p0, p1) in enumerate(segments(gx.shape[0], seg_pings)):
        mb, vb = segment_layer(gx, gy, norm, mask, p, p0, p1)
        sums = shift_sums(lay_a[0], lay_a[1], mb, vb, radius)
        r = R.peak(sums, radius, min_cells, p.cell)
        sx = sy = 0
        if r["zncc"] > -2.0:
            n, sx, sy = centroid_sums(lay_a[1], vb, r["dx"], r["dy"])
            assert n == r["n"]
        out.append(dict(seg=s, p0=p0, p1=p1, sums=sums, r=r, sx=sx, sy=sy))
    return out


def accepted(r, min_zncc=MIN_ZNCC):
    return bool(r["zncc"] >= min_zncc and r["on_border"] == 0)


def scan_distance(rows, px, py):
    """|cos(yaw_i) (px - x_i) + sin(yaw_i) (py - y_i)| per ping: how far the point lies from the ping's scan line"""
    rows = np.asarray(rows, np.float64)
    return np.abs(np.cos(rows[:, 2]) * (px - rows[:, 3]) + np.sin(rows[:, 2]) * (py - rows[:, 4]))


def anchor(rows, r0, r1, px, py):
    """(index, lead): the ping of [r0, r1) whose scan line passes nearest the point, the lowest index among equals, and by how much it
    beats the best ping with another distance (inf when there is none)"""
    d = scan_distance(rows[r0:r1], px, py)
    k = int(np.argmin(d))                       # the first of the minima
    rest = d[d != d[k]]
    return r0 + k, (float(rest.min() - d[k]) if len(rest) else np.inf)


def centre(row, p):
    n = row["r"]["n"]
    return p.x0 + (row["sx"] / n + 0.5) * p.cell, p.y0 + (row["sy"] / n + 0.5) * p.cell


def _mat(orc, p6):
    T = np.eye(4); q = orc.pose12(np.asarray(p6, np.float64))
    T[:3, :3] = q[:9].reshape(3, 3); T[:3, 3] = q[9:]
    return T


def edge(orc, row, p, rows_a, base_a, rows_b, base_b, min_zncc=MIN_ZNCC, sigma_xy_cells=SIGMA_XY_CELLS, sigma_z=SIGMA_Z, sigma_rot=SIGMA_ROT):
    """the pose-graph edge of one segment row -> dict(a, b, rel[12], var[6], i, j, lead) or None when the row is rejected"""
    r = row["r"]
    if not accepted(r, min_zncc):
        return None
    cx, cy = centre(row, p)
    i, lead_i = anchor(rows_a, 0, len(rows_a), cx, cy)
    j, lead_j = anchor(rows_b, row["p0"], row["p1"], cx + r["off_x"], cy + r["off_y"])
    Xa = _mat(orc, rows_a[i])
    moved = np.array(rows_b[j], np.float64); moved[3] -= r["off_x"]; moved[4] -= r["off_y"]
    Xb = _mat(orc, moved)
    ga, gb = base_a + i, base_b + j
    if ga < gb:
        a, b, T = ga, gb, np.linalg.inv(Xa) @ Xb
    else:
        a, b, T = gb, ga, np.linalg.inv(Xb) @ Xa
    sxy = sigma_xy_cells * p.cell
    var = np.array([sigma_rot ** 2] * 3 + [sxy ** 2] * 2 + [sigma_z ** 2])
    return dict(a=int(a), b=int(b), rel=np.concatenate([T[:3, :3].ravel(), T[:3, 3]]), var=var, i=i, j=j, lead=min(lead_i, lead_j))


def edges(orc, rows, p, rows_a, base_a, rows_b, base_b, **kw):
    """edge() over the rows of one pair -> (list of edges, list of the rows' indices they came from)"""
    out, src = [], []
    for k, row in enumerate(rows):
        e = edge(orc, row, p, rows_a, base_a, rows_b, base_b, **kw)
        if e is not None:
            out.append(e); src.append(k)
    return out, src


def lc_edges(orc, es):
    """a list of edge dicts as the oracle's edge records"""
    arr = np.zeros(len(es), orc.LCEDGE_DTYPE)
    for k, e in enumerate(es):
        arr[k]["a"] = e["a"]; arr[k]["b"] = e["b"]; arr[k]["rel"] = e["rel"]; arr[k]["var"] = e["var"]
    return arr


def rows_of_poses12(poses12):
    """total x 12 (R row-major, t) -> the trajectory rows "r p y x y z" (Rot3::rpy: R = Rz(y) Ry(p) Rx(r))"""
    P = np.asarray(poses12, np.float64).reshape(-1, 12)
    out = np.empty((len(P), 6))
    out[:, 0] = np.arctan2(P[:, 7], P[:, 8])
    out[:, 1] = np.arctan2(-P[:, 6], np.sqrt(P[:, 7] ** 2 + P[:, 8] ** 2))
    out[:, 2] = np.arctan2(P[:, 3], P[:, 0])
    out[:, 3:] = P[:, 9:]
    return out


def drift(rows):
    """the drift of the feasibility check added to a leg's rows: x += 0.1 + 0.4 t, y += -0.3 + 0.2 t, t = 0 .. 1 over the pings"""
    t = np.linspace(0.0, 1.0, len(rows))
    out = np.array(rows, np.float64)
    out[:, 3] += 0.1 + 0.4 * t; out[:, 4] += -0.3 + 0.2 * t
    return out

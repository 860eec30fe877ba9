"""Numpy reference of the dense loop closures with a yaw fan (include/dsss.h, "dense loop closures with a yaw fan"), written from the
definition and from nothing else: the rotation with the oracle's orc_sincos and plain numpy arithmetic in the stated order, geo
coordinates from the oracle's geo_img on the rotated rows, layers, sums, peak and centroid from tests/mosaic_register_ref.py and
tests/register_edges_ref.py, the angle rule and the edge written again here."""
import ctypes as C
import numpy as np

from tests import mosaic_register_ref as R
from tests import register_edges_ref as E

STEP, SIGMA_YAW_STEPS = 0.01, 1.0          # the defaults of dsss_reg_yaw_params.step and dsss_reg_edge_yaw_params.sigma_yaw_steps

# the turned survey of the tests: legs 0 and 1 of synth.Survey(2, 640, 400, seed=7) under their true poses on a grid of CELL metres,
# every SEG pings of leg 1 turned by -m step about their pivot and the leg moved by SHIFT whole cells; FANS: name -> (nyaw, step, m)
CELL, SEG, SHIFT = 0.1, 80, (2, -1)
FANS = {"one_step_up": (5, 0.01, 1), "one_wide_step_down": (5, 0.02, -1)}


def thetas(nyaw, step):
    mid = (nyaw - 1) // 2
    return [float(k - mid) * step for k in range(nyaw)]


def sincos(orc, x):
    s = C.c_double(0.0); c = C.c_double(0.0)
    orc.lib().orc_sincos(C.c_double(x), C.byref(s), C.byref(c))
    return np.float64(s.value), np.float64(c.value)


def rotate_rows(orc, rows_b, p0, p1, theta):
    """the pings [p0, p1) turned by theta about the position of ping (p0 + p1) // 2 -> (p1 - p0) x 6; theta == 0 copies"""
    rows_b = np.asarray(rows_b, np.float64)
    out = rows_b[p0:p1].copy()
    if theta == 0.0:
        return out
    cx, cy = rows_b[(p0 + p1) // 2, 3], rows_b[(p0 + p1) // 2, 4]
    s, c = sincos(orc, theta)
    dx = rows_b[p0:p1, 3] - cx; dy = rows_b[p0:p1, 4] - cy
    out[:, 3] = cx + (c * dx - s * dy)
    out[:, 4] = cy + (s * dx + c * dy)
    out[:, 2] = rows_b[p0:p1, 2] + np.float64(theta)
    return out


def yaw_peak(znccs, nyaw, step):
    """the angle rule on the peak znccs of the nyaw angles (-2 = not usable) -> (k, yaw_on_border, theta, theta_hat)"""
    mid = (nyaw - 1) // 2
    usable = [(-float(z), abs(k - mid), k) for k, z in enumerate(znccs) if z > -2.0]
    if not usable:
        return mid, 0, 0.0, 0.0
    k = min(usable)[2]
    border = int(nyaw > 1 and k in (0, nyaw - 1))
    theta = float(k - mid) * step
    q = 0.0
    if not border and nyaw > 1 and znccs[k - 1] > -2.0 and znccs[k + 1] > -2.0:
        zm, z0, zp = float(znccs[k - 1]), float(znccs[k]), float(znccs[k + 1])
        if zm - 2.0 * z0 + zp < 0.0:
            q = 0.5 * (zm - zp) / (zm - 2.0 * z0 + zp)
    return k, border, theta, theta + q * step


def register_segments_yaw(orc, lay_a, rows_b, gr, M, norm, mask, p, seg_pings, radius, min_cells, nyaw, step):
    """frame b (rows, ground ranges, grey levels, mask) cut into segments, each under every angle of the fan against the whole layer
    lay_a = (m, valid) of frame a -> one dict per segment: seg, p0, p1, sums[nyaw] and recs[nyaw] (the dicts of R.peak), k,
    yaw_on_border, theta, theta_hat, zncc_k0, r = recs[k], sx, sy"""
    rows_b = np.ascontiguousarray(rows_b, np.float64)
    out = []
    for s, (p0, p1) in enumerate(E.segments(len(rows_b), seg_pings)):
        sums, recs, valid = [], [], []
        for th in thetas(nyaw, step):
            gx, gy = orc.geo_img(np.ascontiguousarray(rotate_rows(orc, rows_b, p0, p1, th)), gr, M)
            mb, vb = R.mean_layer(gx, gy, norm[p0:p1], mask[p0:p1], p, p.use_mask)
            sm = E.shift_sums(lay_a[0], lay_a[1], mb, vb, radius)
            sums.append(sm); recs.append(R.peak(sm, radius, min_cells, p.cell)); valid.append(vb)
        k, border, theta, theta_hat = yaw_peak([r["zncc"] for r in recs], nyaw, step)
        r = recs[k]
        sx = sy = 0
        if r["zncc"] > -2.0:
            n, sx, sy = E.centroid_sums(lay_a[1], valid[k], r["dx"], r["dy"])
            assert n == r["n"]
        out.append(dict(seg=s, p0=p0, p1=p1, sums=np.stack(sums), recs=recs, k=k, yaw_on_border=border, theta=theta, theta_hat=theta_hat,
                        zncc_k0=recs[(nyaw - 1) // 2]["zncc"], r=r, sx=sx, sy=sy))
    return out


def edge_yaw(orc, row, p, rows_a, base_a, rows_b, base_b, nyaw, step, min_zncc=E.MIN_ZNCC, sigma_xy_cells=E.SIGMA_XY_CELLS, sigma_z=E.SIGMA_Z,
             sigma_rot=E.SIGMA_ROT, sigma_yaw_steps=SIGMA_YAW_STEPS):
    """the pose-graph edge of one fan row -> dict(a, b, rel[12], var[6], i, j, lead) or None when the row is rejected"""
    r = row["r"]
    if not E.accepted(r, min_zncc) or row["yaw_on_border"] != 0:
        return None
    cx, cy = E.centre(row, p)
    p0, p1 = row["p0"], row["p1"]
    i, lead_i = E.anchor(rows_a, 0, len(rows_a), cx, cy)
    jl, lead_j = E.anchor(rotate_rows(orc, rows_b, p0, p1, row["theta"]), 0, p1 - p0, cx + r["off_x"], cy + r["off_y"])
    j = p0 + jl
    Xa = E._mat(orc, rows_a[i])
    moved = rotate_rows(orc, rows_b, p0, p1, row["theta_hat"])[jl]; moved[3] -= r["off_x"]; moved[4] -= r["off_y"]
    Xb = E._mat(orc, moved)
    ga, gb = base_a + i, base_b + j
    if ga < gb:
        a, b, T = ga, gb, np.linalg.inv(Xa) @ Xb
    else:
        a, b, T = gb, ga, np.linalg.inv(Xb) @ Xa
    sxy = sigma_xy_cells * p.cell
    syaw = sigma_rot if nyaw == 1 else sigma_yaw_steps * step
    var = np.array([sigma_rot ** 2] * 2 + [syaw ** 2] + [sxy ** 2] * 2 + [sigma_z ** 2])
    return dict(a=int(a), b=int(b), rel=np.concatenate([T[:3, :3].ravel(), T[:3, 3]]), var=var, i=i, j=j, lead=min(lead_i, lead_j))


def edges_yaw(orc, rows, p, rows_a, base_a, rows_b, base_b, nyaw, step, **kw):
    """edge_yaw() over the rows of one pair -> (list of edges, list of the rows' indices they came from)"""
    out, src = [], []
    for k, row in enumerate(rows):
        e = edge_yaw(orc, row, p, rows_a, base_a, rows_b, base_b, nyaw, step, **kw)
        if e is not None:
            out.append(e); src.append(k)
    return out, src


def rotated_survey(orc, rows, seg_pings, m, step, shift_cells, cell):
    """the rows of a leg with every segment turned by -m step about its pivot and the leg moved by shift_cells whole cells: a fan of
    that step undoes it with k - mid == m, and the leg then lies shift_cells off from where it belongs: the peak (dx, dy)"""
    rows = np.asarray(rows, np.float64)
    out = rows.copy()
    for p0, p1 in E.segments(len(rows), seg_pings):
        out[p0:p1] = rotate_rows(orc, rows, p0, p1, float(-m) * step)
    out[:, 3] += shift_cells[0] * cell; out[:, 4] += shift_cells[1] * cell
    return out

"""The designed inputs of the mosaic-canvas tests (include/dsss_canvas.h), shared by tests/test_mosaic_canvas_cpu.py (the preconditions,
on the reference alone) and tests/test_gpu_mosaic_canvas.py (the device against the same numbers).  Nothing here calls the library.

Frames: 0 and 1 are the two legs of tests/mosaic_composite_cases.py (640 x 400 and 500 x 700), 2 is leg 0 set with the slant-corrected
ground ranges of T2 (tests/mosaic_footprint_cases.py).  Rows are named: "own" = the poses the frame was set with, "t1" = the trajectory of
T1 / T2 (NaN rows 500..502, the 1.5 m jump), "d0.003", "d0.01", "d0.3" = leg 0's own poses shifted by (d, -d / 2).
A script is a list of steps ("put", {id: rows name, ...}) / ("remove", [ids]) / ("clear",); the reference of a script is
tests/mosaic_footprint_ref.render of the frames it leaves on the canvas under the rows they were last put with -- the invariant of the
header, written down: the history does not enter.
Everything is computed once per session and cached; nobody writes into the arrays."""
import types

import numpy as np

from tests import mosaic_composite_cases as CK
from tests import mosaic_footprint_cases as FK
from tests import mosaic_footprint_ref as FR

CELL = 0.05
SHIFTS = (0.003, 0.01, 0.3)
MAX_GAP = FK.MAX_GAP
KINDS = {"point": None, "fp4": (4, MAX_GAP), "fp8": (8, MAX_GAP)}            # canvas kind -> its footprint parameters
T2_GROW = 60                                                                  # cells the T2 grid is grown by on every side
_CACHE = {}
legs = CK.legs


def shifted(rows, d):
    out = rows.copy()
    out[:, 3] += d; out[:, 4] -= d / 2
    return np.ascontiguousarray(out)


def rows_of(orc, fid, name):
    """the N x 6 rows `name` of frame fid"""
    key = ("rows", fid, name)
    if key not in _CACHE:
        own = legs(orc)[1 if fid == 1 else 0]["pose"]
        if name == "own":
            r = np.ascontiguousarray(own)
        elif name == "t1":
            assert fid in (0, 2)
            r = FK.t1_rows(orc)
        elif name.startswith("d"):
            r = shifted(own, float(name[1:]))
        else:
            raise KeyError(name)
        _CACHE[key] = r
    return _CACHE[key]


def gr_of(orc, fid):
    return FK.t2_gr(orc) if fid == 2 else legs(orc)[1 if fid == 1 else 0]["gr"]


def frame_record(orc, fid, name, val=None):
    """the reference's record of frame fid under the rows `name` (val: its corrected grey levels, handed in)"""
    key = ("geo", fid, name)
    if key not in _CACHE:
        l = legs(orc)[1 if fid == 1 else 0]
        _CACHE[key] = orc.geo_img(rows_of(orc, fid, name), gr_of(orc, fid), l["M"])
    l = legs(orc)[1 if fid == 1 else 0]
    gx, gy = _CACHE[key]
    return dict(id=fid, gx=gx, gy=gy, norm=l["norm"], mask=l["mask"], alt=l["alt"], val=val)


def grid(orc, use_mask):
    """the full grid of both legs under their own poses at CELL (641 x 823)"""
    return CK.full_grid(legs(orc), CELL, use_mask)


def t2_grid(orc, use_mask):
    """T2's full grid grown by T2_GROW cells on every side"""
    p = FK.full_grid(orc, "T2", CELL, use_mask)
    return types.SimpleNamespace(x0=p.x0 - T2_GROW * CELL, y0=p.y0 - T2_GROW * CELL, cell=CELL, W=p.W + 2 * T2_GROW, H=p.H + 2 * T2_GROW, use_mask=use_mask)


def final_state(script):
    """{id: rows name} a script leaves on the canvas; asserts what every step presupposes"""
    S = {}
    for step in script:
        if step[0] == "put":
            S.update(step[1])
        elif step[0] == "remove":
            for i in step[1]:
                assert i in S
                del S[i]
        else:
            assert step == ("clear",)
            S = {}
    return S


def reference(orc, state, p, use_mask, kind, vals=None, tag=None):
    """FR.render of a state {id: rows name} on the grid p for a canvas of `kind` -> (sum, cnt, img, sub-samples); vals: {id: corrected
    levels} (then cached under tag)"""
    key = ("ref", tuple(sorted(state.items())), (p.x0, p.y0, p.cell, p.W, p.H), use_mask, kind, tag)
    assert vals is None or tag is not None
    if key not in _CACHE:
        fr = [frame_record(orc, i, n, None if vals is None else vals.get(i)) for i, n in sorted(state.items())]
        if fr:
            _CACHE[key] = FR.render(fr, p, use_mask, KINDS[kind] or (1, MAX_GAP))
        else:
            z = np.zeros((p.H, p.W), np.int64)
            _CACHE[key] = (z, z, z, 0)
    return _CACHE[key]


def point_cells(orc, fid, name, p, use_mask):
    """-> (cell, ok): the cell of every sample of the frame under the rows and whether it is binned"""
    fr = frame_record(orc, fid, name)
    keep = FR._kept(fr, use_mask)
    return FR._cells(fr["gx"], fr["gy"], keep, p)


def stay_share(orc, d, p, use_mask=1):
    """the share of leg 0's kept samples on the grid that fall into the same cell under the rows shifted by (d, -d / 2)"""
    c0, ok0 = point_cells(orc, 0, "own", p, use_mask)
    c1, ok1 = point_cells(orc, 0, "d%g" % d, p, use_mask)
    return float((ok1 & (c1 == c0))[ok0].mean())


def cell_window(gx, gy, p, grow=0.0):
    """the window (ox, oy, bw, bh) of the cells the finite points can reach, their extent grown by `grow` metres on every side; None when
    it misses the grid -- the window rule of the header, restated"""
    out = []
    for g, o, n in ((gx, p.x0, p.W), (gy, p.y0, p.H)):
        lo = np.floor((np.nanmin(g) - grow - o) / p.cell); hi = np.floor((np.nanmax(g) + grow - o) / p.cell)
        if not hi >= 0 or not lo < n:
            return None
        out.append((int(max(lo, 0)), int(min(hi, n - 1))))
    return (out[0][0], out[1][0], out[0][1] - out[0][0] + 1, out[1][1] - out[1][0] + 1)


def union(a, b):
    if a is None or b is None:
        return a or b
    x0, y0 = min(a[0], b[0]), min(a[1], b[1])
    x1, y1 = max(a[0] + a[2], b[0] + b[2]), max(a[1] + a[3], b[1] + b[3])
    return (x0, y0, x1 - x0, y1 - y0)


def frame_window(orc, fid, name, p, kind):
    fr = frame_record(orc, fid, name)
    return cell_window(fr["gx"], fr["gy"], p, 2.0 * MAX_GAP if KINDS[kind] else 0.0)


def outside(cnt, win):
    """the samples of a count layer that lie outside the window"""
    c = np.array(cnt, np.int64)
    if win is not None:
        c[win[1]:win[1] + win[3], win[0]:win[0] + win[2]] = 0
    return c


# ---------------------------------------------------------------- the scripts
ADD_AT_ONCE = [("put", {0: "own", 1: "own"})]
ADD_IN_TURN = [("put", {0: "own"}), ("put", {1: "own"})]
MOVE_T1 = [("put", {0: "own"}), ("put", {0: "t1"})]
MOVE_T1_BACK = MOVE_T1 + [("put", {0: "own"})]
REMOVE_0 = ADD_AT_ONCE + [("remove", [0])]
REMOVE_ALL = REMOVE_0 + [("remove", [1])]
# one call with a new frame (1), a moved frame (0) and an unchanged one (2), then the same in another order of ids and steps
MIXED_A = [("put", {0: "own", 2: "t1"}), ("put", {1: "own", 0: "d0.01", 2: "t1"})]
MIXED_B = [("put", {2: "t1"}), ("put", {0: "d0.3"}), ("put", {2: "t1", 0: "d0.01", 1: "own"})]


def move_script(d):
    return [("put", {0: "own", 1: "own"}), ("put", {0: "d%g" % d})]

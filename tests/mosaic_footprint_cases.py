"""The designed inputs of the footprint-rendering tests, shared by tests/test_mosaic_footprint_cpu.py (the preconditions, on the
reference alone) and tests/test_gpu_mosaic_footprint.py (the device against the same numbers).  The legs are those of the composite
tests (helpers.MOSAIC_SIZES: 640 x 400 and 500 x 700, the smallest frames the extraction accepts) with the oracle's geo_img, normalised
image and mask.  Nothing here calls the library.  Computed once per session; nobody writes into the arrays.
  T0: both legs under their own poses (0.05 m pings, 0.05 m bins): cells 0.05 and 0.02.
  T1: leg 0 under a trajectory override: the ping spacing cycles through 0.03, 0.08, 0.13, 0.18, 0.23 m in blocks of 40 pings, one step
      of 1.5 m sits in front of ping 320, yaw = 0.4 sin(r / 25) so that the outer bins sweep further than the inner ones, and the rows
      500..502 are NaN.
  T2: T1 with the frame set with slant-corrected ground ranges gr[k] = sqrt((9 + 0.05 k)^2 - 81): sparse near the nadir.
Cells 0.05 and 0.1, max_steps 4 and 8, max_gap 1.0 for T1 and T2."""
import numpy as np

from tests import mosaic_composite_cases as CK
from tests import mosaic_footprint_ref as FR

SPACINGS = (0.03, 0.08, 0.13, 0.18, 0.23)
BLOCK, JUMP_AT, JUMP, NAN_ROWS = 40, 320, 1.5, (500, 501, 502)
T0_CELLS, T_CELLS, T_STEPS, MAX_GAP = (0.05, 0.02), (0.05, 0.1), (4, 8), 1.0
_CACHE = {}
legs = CK.legs
grid = CK.grid


def t1_rows(orc):
    """the trajectory rows of T1 and T2 (N x 6, r p y x y z)"""
    if "rows" not in _CACHE:
        l = legs(orc)[0]
        N = l["N"]
        r = np.arange(N)
        step = np.array(SPACINGS)[(r // BLOCK) % len(SPACINGS)]
        step[JUMP_AT] = JUMP                                          # the step INTO ping 320
        rows = l["pose"].copy()
        rows[:, 3] = np.cumsum(step) - step[0]
        rows[:, 2] = 0.4 * np.sin(r / 25.0)
        rows[list(NAN_ROWS), :] = np.nan
        _CACHE["rows"] = np.ascontiguousarray(rows)
    return _CACHE["rows"]


def t2_gr(orc):
    half = legs(orc)[0]["M"] // 2
    return np.sqrt((9.0 + 0.05 * np.arange(half, dtype=np.float64)) ** 2 - 81.0)


def frames(orc, case):
    """the reference's frame records of a case: "T0" -> legs 0 and 1 as frames 0 and 1; "T1" -> leg 0 under t1_rows as frame 0; "T2" ->
    leg 0 with t2_gr under t1_rows as frame 2"""
    if case not in _CACHE:
        L = legs(orc)
        if case == "T0":
            fr = CK.frames(L)
        else:
            l = L[0]
            gr = l["gr"] if case == "T1" else t2_gr(orc)
            gx, gy = orc.geo_img(t1_rows(orc), gr, l["M"])
            fr = [dict(id=0 if case == "T1" else 2, gx=gx, gy=gy, norm=l["norm"], mask=l["mask"], alt=l["alt"])]
        _CACHE[case] = fr
    return _CACHE[case]


def full_grid(orc, case, cell, use_mask):
    """dsss_mosaic_grid's grid over the finite points of the case"""
    fr = frames(orc, case)
    gx = np.concatenate([f["gx"].ravel() for f in fr]); gy = np.concatenate([f["gy"].ravel() for f in fr])
    return grid(np.nanmin(gx), np.nanmax(gx), np.nanmin(gy), np.nanmax(gy), cell, use_mask)


def render_ref(orc, case, cell, use_mask, params):
    """FR.render of a case on its full grid, cached by its arguments; params None: point samples (max_steps 1)"""
    key = ("render", case, cell, use_mask, params)
    if key not in _CACHE:
        _CACHE[key] = FR.render(frames(orc, case), full_grid(orc, case, cell, use_mask), use_mask, params or (1, MAX_GAP))
    return _CACHE[key]


def composite_ref(orc, case, cell, use_mask, mode, R, params):
    key = ("composite", case, cell, use_mask, mode, R, params)
    if key not in _CACHE:
        _CACHE[key] = FR.composite(frames(orc, case), full_grid(orc, case, cell, use_mask), use_mask, mode, R, params)
    return _CACHE[key]

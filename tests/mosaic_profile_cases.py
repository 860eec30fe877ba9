"""The designed inputs of the per-ping profile tests (include/dsss_profile.h), shared by tests/test_mosaic_profile_cpu.py (the
preconditions, on the reference alone) and tests/test_gpu_mosaic_profile.py (the device against the same numbers).  Nothing here calls
the library.  Frames and named rows are those of tests/mosaic_canvas_cases.py: frame 0 is leg 0 (640 x 400), frame 1 leg 1 (500 x 700),
frame 2 leg 0 under T2's ground ranges; rows "own", "t1" (NaN rows 500..502, the 1.5 m jump) and "d0.3"; CELL 0.05.

A case: ids = the listed frames in the order they are handed in, rows = {id: rows name}, use_mask, min_count, prof = indices into ids
(None: all), grid = "full" (both legs' full grid, 641 x 823) or "mid" (its middle third: samples fall off the grid), gain = None, "col"
(a column table) or "two" (a table of two altitude bands); under a table the corrected levels go to the reference as val, as the canvas
tests hand them in.  The gain cases list frames 0 and 2: a table has the M of the frames it corrects, and those two share leg 0's.
Every reference is computed once per session and cached; nobody writes into the arrays."""
import types

import numpy as np

from tests import mosaic_canvas_cases as K
from tests import mosaic_gain_bands_ref as B
from tests import mosaic_gain_ref as G
from tests import mosaic_profile_ref as PR

CELL = K.CELL
BANDS = (8.0, 1.0, 2)                              # the legs' altitudes are 9 + sin(s / 7): both bands hold pings
_CACHE = {}


def _case(ids, rows, use_mask, min_count=1, prof=None, grid="full", gain=None):
    return dict(ids=list(ids), rows=dict(rows), use_mask=use_mask, min_count=min_count, prof=prof, grid=grid, gain=gain)


CASES = {}
for _name, _rows in (("own", {0: "own", 1: "own"}), ("t1", {0: "t1", 1: "own"}), ("d0.3", {0: "d0.3", 1: "own"})):
    for _um in (0, 1):
        CASES["%s_um%d" % (_name, _um)] = _case([0, 1], _rows, _um)
THREE = {0: "own", 1: "own", 2: "t1"}
CASES["three"] = _case([0, 1, 2], THREE, 0)                                     # two of the three from the same images
CASES["three_min3"] = _case([0, 1, 2], THREE, 0, min_count=3)
CASES["two_min3"] = _case([0, 1], {0: "own", 1: "own"}, 0, min_count=3)         # no cell holds three samples of the other leg: nothing is compared
CASES["subset"] = _case([0, 1, 2], THREE, 0, prof=[1])
CASES["reversed"] = _case([0, 1, 2], THREE, 0, prof=[2, 1, 0])
CASES["alone"] = _case([0], {0: "own"}, 0)
CASES["mid"] = _case([0, 1], {0: "own", 1: "own"}, 0, grid="mid")
CASES["gain_col"] = _case([0, 2], {0: "own", 2: "t1"}, 1, gain="col")
CASES["gain_two"] = _case([0, 2], {0: "own", 2: "t1"}, 1, gain="two")


def gain_table(orc, kind):
    """the table of a gain case (None: none): M uint16 for "col", 2 x M for "two" (with BANDS)"""
    if kind is None:
        return None
    M = K.legs(orc)[0]["M"]
    rng = np.random.default_rng(11)
    col = rng.integers(150, 400, M).astype(np.uint16); col[::7] = 0; col[3::11] = 65535
    two = rng.integers(100, 500, (2, M)).astype(np.uint16)
    return col if kind == "col" else two


def corrected(orc, kind):
    """leg 0's levels under the table `kind` by the gain references (frames 0 and 2 hold leg 0's images)"""
    l = K.legs(orc)[0]
    return G.apply(l["norm"], gain_table(orc, kind)) if kind == "col" else B.apply_banded(l["norm"], l["alt"], gain_table(orc, kind), BANDS)


def grid(orc, case):
    p = K.grid(orc, case["use_mask"])
    if case["grid"] == "full":
        return p
    W, H = p.W // 3, p.H // 3
    return types.SimpleNamespace(x0=p.x0 + W * p.cell, y0=p.y0 + H * p.cell, cell=p.cell, W=W, H=H, use_mask=p.use_mask)


def frames(orc, case, ids=None):
    """the reference's records of the case's frames in the order of ids (None: the case's)"""
    val = None if case["gain"] is None else corrected(orc, case["gain"])
    return [K.frame_record(orc, i, case["rows"][i], val) for i in (case["ids"] if ids is None else ids)]


def reference(orc, name):
    """-> (stats, diff, info) of tests/mosaic_profile_ref.profile for the case"""
    if name not in _CACHE:
        case = CASES[name]
        _CACHE[name] = PR.profile(frames(orc, case), grid(orc, case), case["use_mask"], case["prof"], case["min_count"])
    return _CACHE[name]


def state_reference(orc, state, ids, use_mask, min_count=1):
    """the reference of a canvas profile: the frames of `state` = {id: rows name} ascending, profiled in the order of `ids`"""
    key = ("state", tuple(sorted(state.items())), tuple(ids), use_mask, min_count)
    if key not in _CACHE:
        S = sorted(state)
        fr = [K.frame_record(orc, i, state[i]) for i in S]
        _CACHE[key] = PR.profile(fr, K.grid(orc, use_mask), use_mask, [S.index(i) for i in ids], min_count)
    return _CACHE[key]


def pings_of(orc, case):
    """the (first ping, N) of every profiled frame within the case's records"""
    out, o = [], 0
    for k in (range(len(case["ids"])) if case["prof"] is None else case["prof"]):
        N = K.legs(orc)[1 if case["ids"][k] == 1 else 0]["N"]
        out.append((o, N)); o += N
    return out

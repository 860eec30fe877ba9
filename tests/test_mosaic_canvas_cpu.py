"""The mosaic canvas (include/dsss_canvas.h), the part that needs no GPU: the preconditions of the designed cases of
tests/mosaic_canvas_cases.py on the reference alone (what the scripts of tests/test_gpu_mosaic_canvas.py rest on), the defaults, and the
coverage of the new header: every function it declares is exported by libdsss.so and named in the GPU file's table of driven entries."""
import ctypes as C
import os

import numpy as np

from tests import inflight_cases
from tests import mosaic_canvas_cases as K
from tests import mosaic_footprint_cases as FK
from tests import mosaic_footprint_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scripts_are_well_formed():
    for s in (K.ADD_AT_ONCE, K.ADD_IN_TURN, K.MOVE_T1, K.MOVE_T1_BACK, K.REMOVE_0, K.REMOVE_ALL, K.MIXED_A, K.MIXED_B) + tuple(K.move_script(d) for d in K.SHIFTS):
        K.final_state(s)
    assert K.final_state(K.ADD_AT_ONCE) == K.final_state(K.ADD_IN_TURN) == {0: "own", 1: "own"}
    assert K.final_state(K.MOVE_T1_BACK) == {0: "own"} and K.final_state(K.REMOVE_ALL) == {}
    assert K.final_state(K.MIXED_A) == K.final_state(K.MIXED_B) == {0: "d0.01", 1: "own", 2: "t1"}
    # the second put of MIXED_A holds a new frame, a moved frame and an unchanged one
    before, call = K.final_state(K.MIXED_A[:1]), K.MIXED_A[1][1]
    assert sorted(i for i in call if i not in before) == [1]
    assert sorted(i for i in call if i in before and before[i] != call[i]) == [0]
    assert sorted(i for i in call if i in before and before[i] == call[i]) == [2]


def test_the_legs_overlap_and_a_remove_must_leave_the_other_leg(orc):
    p = K.grid(orc, 1)
    assert (p.W, p.H) == (641, 823)
    c0 = K.reference(orc, {0: "own"}, p, 1, "point")[1]
    c1 = K.reference(orc, {1: "own"}, p, 1, "point")[1]
    both = K.reference(orc, {0: "own", 1: "own"}, p, 1, "point")
    print("leg 0 fills %d cells, leg 1 %d, %d hold samples of both" % ((c0 > 0).sum(), (c1 > 0).sum(), ((c0 > 0) & (c1 > 0)).sum()))
    assert int((c0 > 0).sum()) == 24063
    assert int(((c0 > 0) & (c1 > 0)).sum()) == 2046
    assert (both[1] == c0 + c1).all()


def test_shifts_leave_lanes_that_stay_lanes_that_leave_and_a_frame_where_none_stay(orc):
    p = K.grid(orc, 1)
    share = {d: K.stay_share(orc, d, p) for d in K.SHIFTS}
    print("share of leg 0's kept samples that stay in their cell: %s" % {d: "%.1f %%" % (100 * s) for d, s in share.items()})
    assert round(100 * share[0.003], 1) == 97.6
    assert round(100 * share[0.01], 1) == 92.8
    assert share[0.3] == 0.0
    # at least one cell empties completely under a move
    own = K.reference(orc, {0: "own"}, p, 1, "point")[1]
    for d in K.SHIFTS:
        moved = K.reference(orc, {0: "d%g" % d}, p, 1, "point")[1]
        emptied = int(((own > 0) & (moved == 0)).sum())
        print("shift %g: %d cells empty completely, %d fill" % (d, emptied, int(((own == 0) & (moved > 0)).sum())))
        assert emptied >= 1


def test_the_t1_move_has_rows_that_are_not_finite_and_leaves_the_grid(orc):
    p = K.grid(orc, 1)
    rows = K.rows_of(orc, 0, "t1")
    assert np.isnan(rows[500:503]).all() and np.isfinite(rows[:500]).all()
    own = K.reference(orc, {0: "own"}, p, 1, "point")
    t1 = K.reference(orc, {0: "t1"}, p, 1, "point")
    assert 0 < t1[3] < own[3]                                                       # part of the trajectory lies off the legs' grid
    assert (own[1] != t1[1]).any()


def test_t2_sub_samples_leave_the_point_window_and_stay_in_the_grown_one(orc):
    """without the mask: the filter mask rejects the outermost bins, whose outward steps are the ones that leave the window"""
    p = K.t2_grid(orc, 0)
    fr = K.frame_record(orc, 2, "t1")
    pw = K.cell_window(fr["gx"], fr["gy"], p)
    gw = K.frame_window(orc, 2, "t1", p, "fp4")
    assert pw is not None and gw is not None
    print("T2: grid %d x %d, point window %s, footprint window %s" % (p.W, p.H, pw, gw))
    assert gw[2] < p.W and gw[3] < p.H                                             # still smaller than the grid
    assert K.outside(K.reference(orc, {2: "t1"}, p, 0, "point")[1], pw).sum() == 0
    for kind, want in (("fp4", 289), ("fp8", 434)):
        cnt = K.reference(orc, {2: "t1"}, p, 0, kind)[1]
        out = K.outside(cnt, pw)
        grown1 = (pw[0] - 1, pw[1] - 1, pw[2] + 2, pw[3] + 2)
        print("T2 %s: %d sub-samples outside the point window" % (kind, int(out.sum())))
        assert int(out.sum()) == want
        assert K.outside(cnt, grown1).sum() == 0                                   # by one cell
        assert K.outside(cnt, gw).sum() == 0


def test_params_default():
    from diasss_amd import capi
    p = capi.canvas_params_default()
    f = capi.footprint_params_default()
    assert (p.footprint, p.move) == (0, capi.CANVAS_MOVE_AUTO) and (p.fp.max_steps, p.fp.max_gap) == (f.max_steps, f.max_gap) == FR.DEFAULTS
    assert (capi.CANVAS_MOVE_AUTO, capi.CANVAS_MOVE_SPLIT) == (0, 1)
    capi.lib().dsss_canvas_params_default(None)                                    # NULL: nothing happens
    assert C.sizeof(capi.CanvasParams) == 24 and C.sizeof(capi.CanvasPutInfo) == 40


def test_every_entry_of_the_header_is_exported_and_driven():
    from diasss_amd import capi
    from tests import test_gpu_mosaic_canvas as T
    with open(os.path.join(ROOT, "include", "dsss_canvas.h")) as f:
        text = f.read()
    assert '#include "dsss.h"' in text
    declared = inflight_cases.declared_entries(text)
    assert len(declared) == 11 and all(n.startswith("dsss_canvas_") for n in declared), declared
    L = capi.lib()
    for n in declared:
        assert hasattr(L, n), "%s is declared and not exported" % n
    assert sorted(T.DRIVEN) == declared, "declared and not driven: %s; driven and not declared: %s" % (
        sorted(set(declared) - set(T.DRIVEN)), sorted(set(T.DRIVEN) - set(declared)))
    # the move modes the GPU cases run are those the header defines
    import re
    modes = dict((n, int(v)) for n, v in re.findall(r"#define\s+DSSS_CANVAS_MOVE_(\w+)\s+(\d+)", text))
    assert modes == {"AUTO": capi.CANVAS_MOVE_AUTO, "SPLIT": capi.CANVAS_MOVE_SPLIT} and sorted(T.MOVES) == sorted(modes.values())
    # dsss.h itself got no new function
    with open(os.path.join(ROOT, "include", "dsss.h")) as f:
        assert not [n for n in inflight_cases.declared_entries(f.read()) if "canvas" in n]

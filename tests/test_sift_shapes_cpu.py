"""Preconditions of tests/test_gpu_sift_shapes.py, on the oracle alone (no GPU): the frames of tests/sift_shapes_ref.py together hold
keypoints of every window class of sift_desc_kernel and on both sides of the eight equalities of its dword condition; keypoints with an IC
angle of exactly 0; samples whose orientation bin wraps below 0; every octant of ori; rows that the clip at 0.2 changes and rows it leaves
alone.  The two classes that the extraction cannot reach (o0 >= 8, an element above 255 before the clamp: see the docstring of
tests/sift_shapes_ref.py) are asserted ABSENT on every frame, so that the claim stays true when frames change.  A GPU comparison on a table
that fails one of these would go green on the wrong path."""
import numpy as np
import pytest

from tests import sift_shapes_ref as S


def _cases(orc, names):
    return [S.case(orc, n) for n in names]


def test_level_coordinates_are_the_oracles(orc):
    """the integer level coordinates, the blurred levels and the angle that the histogram references are built from give the oracle's own
    128-byte rows: orc_sift_finalize of every reference histogram is the row orc_orb_extract_sift wrote for that keypoint"""
    n = 0
    for c in _cases(orc, S.NAMES + S.BATCH):
        for i in range(len(c["pre"])):
            assert (orc.sift_finalize(c["hist"][i]) == c["pre_d128"][i]).all(), (c["name"], i)
        n += len(c["pre"])
        assert len(c["pre"]) >= len(c["ref"]["kps"]) and c["ref"]["d128"].shape == (len(c["ref"]["kps"]), 128)
    empty = S.case(orc, S.BATCH[3])
    assert len(empty["pre"]) == 0 and len(empty["ref"]["kps"]) == 0, "the flat frame of the batch has no keypoint"
    assert all(len(S.case(orc, b)["pre"]) > 50 for b in S.BATCH[:3])
    print("keypoints with a reference histogram:", n)


def test_window_classes_and_equalities_are_all_present(orc):
    cnt = np.zeros(16, int); surv = np.zeros(16, int)
    eq = {k: 0 for k in S.EQUALITIES}
    for c in _cases(orc, S.PART1):
        cnt += np.bincount(c["cls"], minlength=16)
        for k, fn in S.EQUALITIES.items(): eq[k] += int(fn(c["x"], c["y"], c["rows"], c["cols"]).sum())
        surv += np.bincount(c["surv_cls"], minlength=16)      # behind the mask filter: the keypoints whose 128-byte rows the device test compares
    for k in range(16): print("%-40s %5d keypoints, %5d behind the mask filter" % (S.CLASS_NAME[k], cnt[k], surv[k]))
    for k, v in eq.items(): print("%-18s %4d" % (k, v))
    want = (0,) + S.SINGLE + S.CORNERS + (S.LEFT | S.RIGHT, S.TOP | S.BOTTOM, 15)
    assert all(cnt[k] > 0 for k in want), [S.CLASS_NAME[k] for k in want if cnt[k] == 0]
    assert all(surv[k] > 0 for k in want), [S.CLASS_NAME[k] for k in want if surv[k] == 0]
    assert all(v > 0 for v in eq.values()), eq
    # the rule itself at the equalities: met from inside they are class 0 when nothing else clips, their neighbours never are
    assert S.window_class(35, 35, 71, 71) == 0 and S.window_class(34, 35, 71, 71) == S.LEFT and S.window_class(35, 34, 71, 71) == S.TOP
    assert S.window_class(36, 35, 71, 71) == S.RIGHT and S.window_class(35, 36, 71, 71) == S.BOTTOM and S.window_class(34, 34, 69, 69) == 15
    assert S.window_class(34, 34, 70, 70) == (S.LEFT | S.TOP) and S.window_class(35, 35, 70, 70) == (S.RIGHT | S.BOTTOM)      # 70 px never clip opposite sides


def test_levels_of_the_table(orc):
    """the part-1 frames are the ones the issue names, extracted under SMALL_MASK (the two frames with a 69-column level alone drop the
    static mask's centre columns), and every level below 70 px an axis is there"""
    assert len(S.PART1) == 16 + 1 + 4 + 2 + 2 + 2
    sizes = set()
    for c in _cases(orc, S.PART1):
        assert c["mask"] == (S.ALLFOUR_MASK if c["name"].startswith("allfour") else S.X.SMALL_MASK)
        sizes |= {lv.shape for lv in c["ref"]["levels"]}
    assert {(69, 69), (91, 69), (69, 70), (70, 70), (69, 1236)} <= sizes
    assert sum(len(S.case(orc, n)["pre"]) for n in ("band-8", "band-2")) < 1500


def test_orientation_classes(orc):
    """angle == 0.0 on the axis of the mirror frames (and on the symmetric dots); the restated arithmetic of orc_sift_hist gives the oracle's
    histogram on EVERY keypoint of the table, so what it says about floor(obin) before the wrap holds: below 0 on nearly every keypoint,
    8 or above on none"""
    zero = 0
    for c in _cases(orc, [n for n in S.NAMES if n.startswith("mirror")]):
        k = c["ref"]["kps"]
        on_axis = (k["angle"] == 0.0)
        zero += int(on_axis.sum())
        assert (k["y"][on_axis] == S.MIRROR_SHAPE[0] // 2).all()
    assert zero >= 1, "a surviving keypoint with an IC angle of exactly 0"
    lo = hi = n = n_zero = 0
    octants = set()
    for c in _cases(orc, S.NAMES):
        for i in range(len(c["pre"])):
            ang = float(c["pre"]["angle"][i])
            r = S.hist_restated(orc, c["blur"][c["pre"]["octave"][i]], c["x"][i], c["y"][i], ang)
            assert (r["h"] == c["hist"][i]).all(), "the restatement leaves orc_sift_hist (%s, keypoint %d)" % (c["name"], i)
            lo += int((r["o0"] < 0).any()); hi += int((r["o0"] >= 8).any()); n += 1
            if c["name"] in S.PART1: octants.add(int(r["ori"] // 45.0))
            if ang == 0.0:
                n_zero += 1
                assert r["ori"] == 0.0 and (r["o0"] >= 0).all(), "ori = 360 is reset to 0: no sample is below bin 0"
    print("keypoints restated: %d; with a sample at floor(obin) < 0: %d; at >= 8: %d; with angle == 0: %d; octants of ori: %s" % (n, lo, hi, n_zero, sorted(octants)))
    assert lo > 0 and n_zero >= 1 and octants == set(range(8))
    assert hi == 0, "o0 >= 8 was thought unreachable (tests/sift_shapes_ref.py): a frame of the table reaches it"


def test_the_wrap_below_zero_is_live_and_the_wrap_at_eight_is_not(orc):
    """on the restated arithmetic: without `if (o0 < 0) o0 += 8` the histogram is another one; without `if (o0 >= 8) o0 -= 8` it is the same
    even at a keypoint angle above 360 given to the oracle directly (the only way to o0 = 8), because slots 8 and 9 fold onto 0 and 1"""
    c = S.case(orc, "small-91x92")
    i = int(np.argmax(c["cls"] == 0))
    b, x, y = c["blur"][0], c["x"][i], c["y"][i]
    ang = float(c["pre"]["angle"][i])
    assert (S.hist_restated(orc, b, x, y, ang, wrap_low=False)["h"] != c["hist"][i]).any()
    rr, cc = np.mgrid[0:71, 0:71]
    ramp = (3 * cc + rr // 2).astype(np.uint8)                  # dx = 6, dy = -1 everywhere: Ori = 350.5
    for img, px, py, a in ((b, x, y, 365.5), (ramp, 35, 35, 375.0), (ramp, 30, 40, 400.0)):
        want = orc.sift_hist(img, px, py, a)
        full = S.hist_restated(orc, img, px, py, a)
        assert (full["h"] == want).all() and want.max() > 0
        assert (S.hist_restated(orc, img, px, py, a, wrap_high=False)["h"] == want).all()
        if img is ramp: assert (full["o0"] == 8).all(), "ori = -15 and -40: every sample of the ramp is at 8 before the wrap"


def test_tail_classes(orc):
    """rows that the clip at 0.2 of the norm changes, rows it leaves alone, and the largest element before the clamp per group of frames:
    none above 255 (the designs for a saturating row are in the table; the module docstring says why they fall short)"""
    clipped = unclipped = 0
    top = {}
    for c in _cases(orc, S.NAMES + S.BATCH[:3]):
        for i in range(len(c["pre"])):
            f = S.finalize_restated(c["hist"][i])
            assert (f["out"] == c["pre_d128"][i]).all(), "the restated tail leaves orc_sift_finalize (%s, keypoint %d)" % (c["name"], i)
            clipped += int(f["clipped"].any()); unclipped += int(not f["clipped"].any())
            g = c["name"] if c["name"].startswith("design") else "speckle"
            top[g] = max(top.get(g, 0), int(f["rr"].max()))
    print("rows the clip changes: %d, rows it leaves alone: %d; largest element before the clamp: %s" % (clipped, unclipped, top))
    assert clipped > 100 and unclipped > 10
    assert all(len(S.case(orc, "design-" + k)["pre"]) > 0 for k in S.SATURATION_DESIGNS), "every design has keypoints"
    assert max(top.values()) <= 255, "saturation was thought unreachable (tests/sift_shapes_ref.py): a frame of the table reaches it"
    # the clamp itself, on the oracle's tail alone
    one = np.zeros(128, np.int32); one[0] = 1000
    assert S.finalize_restated(one)["rr"][0] == 512 and orc.sift_finalize(one)[0] == 255


def test_the_dword_condition_is_held_from_both_sides(orc):
    """the two ways of loading the raw window, restated (sift_shapes_ref.raw_window).  Through reflect-101 every keypoint gets the oracle's
    histogram; by flat addresses the keypoints of class 0 do, the four equalities met from inside included, and keypoints outside do not.
    ONE step outside (cx == 34, cx == cols - 35, cy == 34, cy == rows - 35) the histogram moves only at an IC angle on a diagonal, which
    is what the diag frames plant on each side: a dword condition that is off by one on any of its four sides gives another histogram
    on a keypoint the table holds"""
    side = {"cx == 34": S.LEFT, "cx == cols - 35": S.RIGHT, "cy == 34": S.TOP, "cy == rows - 35": S.BOTTOM}
    inside = {k: 0 for k in S.EQUALITIES if k not in side}
    far = {k: [0, 0] for k in S.SINGLE}
    n0 = 0
    for c in _cases(orc, S.PART1 + tuple(S.DIAG_FRAMES)):
        at = {k: fn(c["x"], c["y"], c["rows"], c["cols"]) for k, fn in S.EQUALITIES.items()}
        small = c["name"].startswith(("small", "allfour", "diag"))
        for i in range(len(c["pre"])):
            here = [k for k in at if at[k][i]]
            if not (small or here): continue
            assert (S.hist_from_window(orc, c, i, False) == c["hist"][i]).all(), "reflect-101 window of %s, keypoint %d" % (c["name"], i)
            if c["cls"][i] == 0:
                assert (S.hist_from_window(orc, c, i, True) == c["hist"][i]).all(), "dword window of %s, keypoint %d" % (c["name"], i)
                n0 += 1
                for k in here: inside[k] += 1
            elif c["cls"][i] in S.SINGLE and small:
                far[c["cls"][i]][0] += 1; far[c["cls"][i]][1] += int((S.hist_from_window(orc, c, i, True) != c["hist"][i]).any())
    print("class 0 by flat addresses: %d keypoints the oracle's; at the equalities from inside: %s" % (n0, inside))
    print("clipped on one side, [keypoints, with another histogram by flat addresses]: %s" % {S.CLASS_NAME[k]: v for k, v in far.items()})
    assert all(v > 0 for v in inside.values()) and all(v[1] > 0 for v in far.values())
    # the planted keypoints: on the equalities with a diagonal angle the flat window is right, one step outside it is not
    moved = {b: 0 for b in S.SINGLE}
    for name, (which, _) in S.DIAG_FRAMES.items():
        c = S.case(orc, name)
        for bit, (cx, cy) in zip(S.SINGLE[:1] + S.SINGLE[2:3] + S.SINGLE[1:2] + S.SINGLE[3:], S.DIAG_AT[which]):      # DIAG_AT: left, right, top, bottom
            i = int(np.argmax((c["x"] == cx) & (c["y"] == cy)))
            assert c["x"][i] == cx and c["y"][i] == cy, "%s has no keypoint at (%d, %d)" % (name, cx, cy)
            assert abs(float(c["pre"]["angle"][i]) % 180.0 - 45.0) < 0.6 and c["cls"][i] == (bit if which == "out" else 0), (name, cx, cy)
            assert ((c["ref"]["kps"]["x"] == cx) & (c["ref"]["kps"]["y"] == cy)).any(), "it survives the mask filter"
            differs = bool((S.hist_from_window(orc, c, i, True) != c["hist"][i]).any())
            if which == "out": moved[bit] += int(differs)
            else: assert not differs
    print("one step outside at a diagonal angle, keypoints with another histogram by flat addresses: %s" % {S.CLASS_NAME[k]: v for k, v in moved.items()})
    assert all(v > 0 for v in moved.values()), moved

"""Preconditions of tests/test_gpu_extract_shapes.py, on the oracle alone (no GPU): every frame of tests/extract_shapes_ref.py is in the
class it is named for -- the shape tables cover both FAST strides, the window extremes, the cell counts and the quadtree root counts; the
oracle returns keypoints everywhere; the gain-ramp frame has cells that only minThFAST fills; the border-band frame has surviving keypoints
on the byte-wise path on all four sides; the hot pixels at the borders erase what the eraser's rule says.  A GPU comparison on a frame
that fails one of these would compare nothing."""
import numpy as np
import pytest

from tests import extract_shapes_ref as X


def test_fast_cells_restates_the_oracle(orc):
    """the Python cell arithmetic places every candidate where orc_fast_level does: candidates rebuilt window by window are the level's"""
    for rows, cols in ((69, 70), (91, 272), (122, 122), (160, 272)):
        img = orc.normalize(X.speckle(rows, cols, 5))
        import ctypes as C
        xs = (C.c_int * 1600)(); ys = (C.c_int * 1600)(); sc = (C.c_int * 1600)()
        got = []
        for x0, y0, w, h, ox, oy in X.fast_cells(rows, cols)["windows"]:
            win = img[y0:, x0:]
            k = orc.lib().orc_fast_window(C.c_void_p(win.ctypes.data), cols, h, w, 12, xs, ys, sc, 1600)
            if k == 0: k = orc.lib().orc_fast_window(C.c_void_p(win.ctypes.data), cols, h, w, 7, xs, ys, sc, 1600)
            got += [(xs[q] + ox, ys[q] + oy, sc[q]) for q in range(k)]
        ref = X.oracle_stages(orc, X.speckle(rows, cols, 5), X.SMALL_MASK, dict(nlevels=1))["cands"][0]
        assert len(got) == len(ref[0]) > 0
        assert (np.array(got, np.float32) == np.stack(ref, 1)).all()


def test_small_shape_table_covers_every_cell_class(orc):
    cls = [X.shape_class(orc, *s) for s in X.SMALL_SHAPES]
    assert {c["stride"] for c in cls} == {40, 68}, "both LDS strides of fast_cells_kernel"
    cw = {c["max_cw"] for c in cls}
    assert 40 in cw and any(w >= 41 for w in cw), "the widest window on either side of the stride threshold"
    wins = [w for s in X.SMALL_SHAPES for r, c in X.shape_class(orc, *s)["levels"] for w in X.fast_cells(r, c)["windows"]]
    assert max(w[2] for w in wins) == 59 and max(w[3] for w in wins) == 59, "the largest window there is, on each axis"
    assert min(w[2] for w in wins) >= 30 and min(w[3] for w in wins) >= 30
    assert {1, 2, 3} <= {n for c in cls for n in c["ncols"]} and {1, 2, 3} <= {n for c in cls for n in c["nrows"]}
    assert any(c["max_cw"] == 40 and c["max_ch"] > 40 for c in cls), "stride 40 with a window taller than it is wide"
    # a level of 91 px is one cell of 59 px; a level of 92 px is two of 30 + 6
    assert [w[2:4] for w in X.fast_cells(91, 91)["windows"]] == [(59, 59)]
    assert [w[2:4] for w in X.fast_cells(92, 92)["windows"]] == [(36, 36), (30, 36), (36, 30), (30, 30)]


def test_pyramid_shape_table_names_the_resize_kernel_of_every_level(orc):
    """the strips flag of every level as resize_tables derives it: the two frames the existing device test puts into one batch come out
    as that test says, and the table holds all-flat pyramids at 2.0 and 1.5 and both orders of strips and flat at 1.334, odd level sizes
    among them, every level with candidates"""
    def flags(r, c, nl, sc):
        lv = X.level_sizes(orc, r, c, X.orb_params(orc, nlevels=nl, scale=sc))
        return tuple(X.resize_strips(lv[l - 1][1], lv[l][1]) for l in range(1, nl))
    assert flags(500, 300, 2, 1.334) == (True,) and flags(500, 302, 2, 1.334) == (False,)
    assert flags(501, 334, 4, 1.1) == (True, True, True) and flags(1000, 802, 4, 2.0) == (False, False, False)
    for r, c, nl, sc, want in X.PYRAMID_SHAPES:
        assert flags(r, c, nl, sc) == want, (r, c, sc)
        raw, orb, ref = X.small_case(orc, r, c, nl, sc)
        assert [lv.shape for lv in ref["levels"]] == X.level_sizes(orc, r, c, ref["op"]) and min(min(lv.shape) for lv in ref["levels"]) >= 69
        assert all(len(cd[0]) > 0 for cd in ref["cands"]) and len(ref["kps"]) > 0, (r, c, sc)
    assert {w for s in X.PYRAMID_SHAPES for w in s[4:]} == {(False, False), (False, True), (True, False)}
    assert any(lv.shape[1] % 2 for s in X.PYRAMID_SHAPES for lv in X.small_case(orc, *s[:4])[2]["levels"])


def test_wide_shape_table_covers_the_root_counts(orc):
    roots = [X.n_roots(r, c) for r, c, _, _, _ in X.WIDE_SHAPES]
    assert roots == [s[4] for s in X.WIDE_SHAPES]
    assert {1, 2, 3, 32, 33} <= set(roots) and max(roots) > 50
    ratio = lambda r, c: (c - 32) / (r - 32)
    assert 1.4 < ratio(69, 86) < 1.5 < ratio(69, 88) < 1.6 and 2.4 < ratio(69, 124) < 2.5 < ratio(69, 126) < 2.6
    assert 32.4 < ratio(69, 1234) < 32.5 < ratio(69, 1236) < 32.6
    assert X.shape_class(orc, 100, 700, 2)["roots"] == [10, 11]
    assert X.n_roots(640, 400) == X.n_roots(500, 700) == X.n_roots(2000, 1024) == 1, "the survey-sized tests have one root"


@pytest.mark.parametrize("rows", X.SMALL_ROWS + (100,))
def test_small_frames_have_candidates_and_keypoints(orc, rows):
    for r, c, nl, sc in X.SMALL_SHAPES:
        if r != rows: continue
        raw, orb, ref = X.small_case(orc, r, c, nl, sc)
        assert all(len(cd[0]) > 0 for cd in ref["cands"]), (r, c)
        assert len(ref["kps"]) > 0, (r, c)
        assert set(ref["kps"]["octave"]) == set(range(nl)), (r, c)
        assert 0 < (ref["mask"] == 0).mean() < 0.5, (r, c)
    if rows == 69:          # a 69 x 70 level emits keypoints on [19, 50] x [19, 49] and loads dwords on [24, 42] x [24, 44] only
        raw, orb, ref = X.small_case(orc, 69, 70, 1, 1.2)
        band = X.band_sides(orc, ref["kps"], 69, 70, ref["op"]) != 0
        assert 2 * band.sum() >= len(band) and (~band).sum() > 0


@pytest.mark.parametrize("shape", X.WIDE_SHAPES, ids=lambda s: "%dx%d" % s[:2])
def test_wide_frames_divide_the_tree(orc, shape):
    rows, cols, nl, nf, roots = shape
    raw, orb, ref = X.wide_case(orc, rows, cols, nl, nf)
    ncand = sum(len(c[0]) for c in ref["cands"])
    nk = len(X.unfiltered_keypoints(orc, ref))
    print(shape, "candidates", ncand, "tree keeps", nk, "after the mask", len(ref["kps"]))
    assert ncand > 2 * nk, "the quota is far below the candidate count: the tree divides and culls"
    assert len(ref["kps"]) >= 30
    x = ref["cands"][0][0]
    hx = np.float32(cols - 32) / np.float32(roots)
    assert len(np.unique(np.minimum((x / hx).astype(int), roots - 1))) == roots, "every root holds candidates"


@pytest.mark.parametrize("N,M", X.RAMP_SHAPES)
def test_gain_ramp_has_cells_only_the_retry_fills(orc, N, M):
    raw, orb, ref = X.ramp_case(orc, N, M, 12, 7)
    at12, at7 = X.cell_survivors(orc, ref["norm"], 12), X.cell_survivors(orc, ref["norm"], 7)
    n = len(at12)
    full, retry, empty = int((at12 > 0).sum()), int(((at12 == 0) & (at7 > 0)).sum()), int((at7 == 0).sum())
    print("%d x %d: %d cells, %d with a corner above 12, %d only above 7, %d empty" % (N, M, n, full, retry, empty))
    assert full + retry + empty == n
    assert min(full, retry, empty) * 10 >= n
    same = X.ramp_case(orc, N, M, 12, 12)[2]
    assert len(ref["cands"][0][0]) > len(same["cands"][0][0]) > 0
    for ini, mn in X.THRESHOLDS:
        r = X.ramp_case(orc, N, M, ini, mn)[2]
        print("  thresholds", (ini, mn), "candidates", [len(c[0]) for c in r["cands"]], "keypoints", len(r["kps"]))
    assert len(X.ramp_case(orc, N, M, 40, 3)[2]["kps"]) > len(X.ramp_case(orc, N, M, 20, 20)[2]["kps"]) > 0
    assert [len(c[0]) for c in X.ramp_case(orc, N, M, 7, 12)[2]["cands"]] != [len(c[0]) for c in ref["cands"]]


def test_border_band_frame_has_keypoints_on_both_paths(orc):
    N, M = X.BAND_SHAPE
    raw, orb, ref = X.band_case(orc)
    side = X.band_sides(orc, ref["kps"], N, M, ref["op"])
    band = side != 0
    print("keypoints", len(side), "in the band", int(band.sum()), "per side", [int(((side >> b) & 1).sum()) for b in range(4)],
          "levels with band keypoints", sorted(set(ref["kps"]["octave"][band])))
    assert band.sum() >= 20 and (~band).sum() >= 20
    assert all(((side >> b) & 1).sum() > 0 for b in range(4)), "left, top, right, bottom"
    assert len(set(ref["kps"]["octave"][band])) >= 4
    assert set(ref["kps"]["octave"]) == set(range(8)), "levels 5 to 7 share one launch group: all of them hold keypoints"
    for nl in (1, 2):
        r = X.band_case(orc, nl)[2]
        s = X.band_sides(orc, r["kps"], N, M, r["op"])
        assert (s != 0).sum() >= 5 and (s == 0).sum() >= 20 and set(r["kps"]["octave"]) == set(range(nl))


def test_border_hot_pixels_follow_the_erasers_rule(orc):
    N, M = X.HOT_SHAPE
    mp = X.mask_params(orc, **X.NO_STATIC_MASK)
    for pos, erased in X.HOT_ERASED:
        m = orc.mask(X.flat_with_hot(N, M, 1, [pos]), mp)
        assert int((m == 0).sum()) == erased, pos
    # r = 0 erases nothing; r = 2 erases 4 x 4 from (2, 2) on
    assert (orc.mask(X.flat_with_hot(N, M, 1, [(60, 80)]), X.mask_params(orc, **dict(X.NO_STATIC_MASK, r=0))) == 255).all()
    for pos, erased in (((1, 80), 0), ((2, 2), 16), ((119, 159), 9)):
        assert int((orc.mask(X.flat_with_hot(N, M, 1, [pos]), X.mask_params(orc, **dict(X.NO_STATIC_MASK, r=2))) == 0).sum()) == erased, pos
    # the float factor: a pixel between mean * (double)(float)2.3 and mean * 2.3 is hot
    raw = X.flat_with_hot(N, M, 2, [], knife=(60, 40), factor=2.3, orc=orc)
    m = orc.mask(raw, X.mask_params(orc, **dict(X.NO_STATIC_MASK, factor=2.3)))
    assert int((m == 0).sum()) == 144 and m[60, 40] == 0
    Nw, Mw = X.HOT_WRAP_SHAPE
    assert Mw % 4 == 2 and (Nw * Mw) % 16 != 0


def _twin_keeps_what_the_oracle_keeps(orc, cands, rows, cols, quota):
    """quadtree.cpp on the candidates of a rows x cols level: the oracle's kept candidates in the oracle's order; how many"""
    import ctypes as C
    from diasss_amd import capi
    xs, ys, rs = (np.ascontiguousarray(a) for a in cands)
    n = len(xs)
    k_o = np.zeros(n, np.int32); k_p = np.zeros(n, np.int32); npk = C.c_int(0)
    no = orc.lib().orc_quadtree(orc.fp(xs), orc.fp(ys), orc.fp(rs), n, 16, cols - 16, 16, rows - 16, quota, orc.ip(k_o))
    rc = capi.lib().dsss_host_quadtree(xs.ctypes.data_as(C.c_void_p), ys.ctypes.data_as(C.c_void_p), rs.ctypes.data_as(C.c_void_p), n,
                                       16, cols - 16, 16, rows - 16, quota, k_p.ctypes.data_as(C.c_void_p), C.byref(npk))
    assert rc == 0 and npk.value == no and quota <= no < n
    assert (k_p[:no] == k_o[:no]).all()
    return no


@pytest.mark.parametrize("shape", X.WIDE_SHAPES + X.QUOTA_SHAPES, ids=lambda s: "%dx%d" % s[:2])
def test_host_twin_builds_the_oracles_tree_at_every_root_count(orc, shape):
    """quadtree.cpp (the host twin of quadtree_kernel) keeps the oracle's candidates in the oracle's order on the wide frames' own
    candidates: the root rule has no upper limit on either side"""
    rows, cols, nl, nf, roots = shape
    raw, orb, ref = X.wide_case(orc, rows, cols, nl, nf)
    _twin_keeps_what_the_oracle_keeps(orc, ref["cands"][0], rows, cols, nf if nl == 1 else nf // 2)


def test_quota_frames_take_the_tree_where_they_say(orc):
    """the two frames of QUOTA_SHAPES are in the class they are named for, and the host twin is the oracle on them"""
    rows, cols, nl, nf, roots = X.QUOTA_SHAPES[0]
    assert X.level_quotas(nf, nl) == [1, 0]
    raw, orb, ref = X.wide_case(orc, rows, cols, nl, nf)
    assert X.shape_class(orc, rows, cols, nl)["roots"] == [1, 1]
    for (r, c), cands, quota in zip(X.level_sizes(orc, rows, cols, ref["op"]), ref["cands"], (1, 0)):
        kept = _twin_keeps_what_the_oracle_keeps(orc, cands, r, c, quota)
        assert 2 <= kept <= 4 < len(cands[0]), "one division of the root, whatever the quota"
    assert len(X.unfiltered_keypoints(orc, ref)) > 4 and set(ref["kps"]["octave"]) == {0, 1}, "both levels keep keypoints, after the mask too"

    rows, cols, nl, nf, roots = X.QUOTA_SHAPES[1]
    raw, orb, ref = X.wide_case(orc, rows, cols, nl, nf)
    xs, ys, _ = ref["cands"][0]
    assert X.n_roots(rows, cols) == roots == 1 and X.level_quotas(nf, nl) == [nf]
    passes = X.whole_list_passes(xs, ys, cols - 2 * X.BORDER, rows - 2 * X.BORDER, 8)
    p, S, Xp, refinement = X.first_verdict(passes, nf)
    print("%d candidates, (nodes, expandable) per pass %s: pass %d ends the whole-list passes" % (len(xs), passes, p))
    assert passes[:6] == [(4 ** d, 4 ** d) for d in range(1, 7)], "every cell down to the pre-sort's deepest holds two candidates or more"
    assert refinement and S < nf and Xp > X.RANK_STAGED and p == 7
    nk = len(X.unfiltered_keypoints(orc, ref))
    assert nf <= nk <= nf + 3 and len(xs) > 2 * nk, "the refinement ends at the quota, far below the candidate count"

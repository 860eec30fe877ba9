"""The dense loop closures over a cell pyramid off the device: the numpy reference of tests/register_pyr_ref.py by hand, the level rule
of libdsss.so (dsss_register_pyr_step) against that reference bit for bit on constructed tables, and the preconditions of the GPU tests
on the reference alone (tests/test_gpu_register_pyr.py): on a survey whose leg 1 lies 2.3 m and 1.7 m off, three levels find (23, -17)
cells in every segment away from every border where the flat search of the widest radius fails, two levels are too few, and a leg
beyond the top level's reach is flagged."""
import ctypes as C
import numpy as np
import pytest

from tests import mosaic_register_ref as R
from tests import register_edges_ref as E
from tests import register_pyr_ref as P

E_ARG = -2
N, M = 640, 400
CELL, SEG, RADIUS, MIN_CELLS, REFINE = P.CELL, P.SEG, P.RADIUS, P.MIN_CELLS, P.REFINE


# ---------------------------------------------------------------- the reference itself
def test_reference_pooling_by_hand():
    """a 5 x 3 layer with holes: W and H are no multiples of 2 or 4, the last column and row pool fewer cells"""
    cnt = np.array([[1, 0, 2, 0, 3],
                    [0, 0, 1, 0, 0],
                    [4, 1, 0, 0, 0]], np.int64)
    sm = np.array([[10, 0, 7, 0, 9],
                   [0, 0, 200, 0, 0],
                   [40, 255, 0, 0, 0]], np.int64)
    c0, s0 = P.pool(cnt, sm, 0)
    assert (c0 == cnt).all() and (s0 == sm).all()
    c1, s1 = P.pool(cnt, sm, 1)
    assert c1.tolist() == [[1, 3, 3], [5, 0, 0]] and s1.tolist() == [[10, 207, 9], [295, 0, 0]]
    m1, v1 = P.layer(c1, s1)
    assert v1.tolist() == [[True, True, True], [True, False, False]]
    assert m1.tolist() == [[10, (207 + 1) // 3, 3], [(295 + 2) // 5, 0, 0]] == [[10, 69, 3], [59, 0, 0]]
    c2, s2 = P.pool(cnt, sm, 2)
    assert c2.tolist() == [[9, 3]] and s2.tolist() == [[512, 9]]
    m2, v2 = P.layer(c2, s2)
    assert m2.tolist() == [[(512 + 4) // 9, 3]] == [[57, 3]] and v2.all()
    c3, s3 = P.pool(cnt, sm, 3)
    assert c3.tolist() == [[12]] and s3.tolist() == [[521]]
    # pooling twice by one level is pooling once by two: the definition is by grid coordinates
    cc, ss = P.pool(*P.pool(cnt, sm, 1), 1)
    assert (cc == c2).all() and (ss == s2).all()
    # level 0 of the pyramid is the mean layer of tests/mosaic_register_ref.py
    m0, v0 = P.pyramid(cnt, sm, 3)[0]
    assert m0.tolist() == [[10, 0, 4, 0, 3], [0, 0, 200, 0, 0], [10, 255, 0, 0, 0]] and (v0 == (cnt > 0)).all()


def _layers(seed, shift, H=36, W=41, holes=0.15):
    """two layers of one random scene, b lying `shift` cells off (b valid at (ix + sx, iy + sy) where the scene is valid at (ix, iy))"""
    rng = np.random.default_rng(seed)
    big = rng.integers(0, 256, (H + 80, W + 80)).astype(np.int64)
    ok = rng.uniform(size=big.shape) >= holes
    sx, sy = shift
    ma, va = big[40:40 + H, 40:40 + W], ok[40:40 + H, 40:40 + W]
    mb, vb = big[40 - sy:40 - sy + H, 40 - sx:40 - sx + W], ok[40 - sy:40 - sy + H, 40 - sx:40 - sx + W]
    noise = rng.integers(-3, 4, mb.shape)
    mb = np.clip(mb + noise, 0, 255)
    return np.where(va, ma, 0), va, np.where(vb, mb, 0), vb


def test_reference_centred_table_by_hand():
    """the table around a centre is the plain table of the same layers with b moved back by the centre, on a canvas wide enough that
    no cell leaves it; around (0, 0) it is R.shift_sums itself"""
    ma, va, mb, vb = _layers(1, (7, -5))
    assert (P.centred_sums(ma, va, mb, vb, 0, 0, 4) == R.shift_sums(ma, va, mb, vb, 4)).all()
    H, W = ma.shape
    pad = 16
    for cx, cy in ((7, -5), (6, -4), (-3, 9)):
        A = np.zeros((H + 2 * pad, W + 2 * pad), np.int64); VA = np.zeros(A.shape, bool); Bm = A.copy(); VB = VA.copy()
        A[pad:pad + H, pad:pad + W] = ma; VA[pad:pad + H, pad:pad + W] = va
        Bm[pad - cy:pad - cy + H, pad - cx:pad - cx + W] = mb; VB[pad - cy:pad - cy + H, pad - cx:pad - cx + W] = vb      # b'(x, y) = b(x + cx, y + cy)
        T = P.centred_sums(ma, va, mb, vb, cx, cy, 3)
        assert (T == R.shift_sums(A, VA, Bm, VB, 3)).all() and T.any()
    # the scene lies (7, -5) off: around that centre the peak is the centre itself, with every valid pair of cells equal up to the noise
    T = P.centred_sums(ma, va, mb, vb, 7, -5, 3)
    rec = R.peak(T, 3, 16, 1.0)
    assert (rec["dx"], rec["dy"]) == (0, 0) and rec["zncc"] > 0.99
    # one cell by hand: a single valid pair at total shift (2, 1)
    a = np.zeros((4, 5), np.int64); b = a.copy(); a[1, 1] = 9; b[2, 3] = 4
    T = P.centred_sums(a, a > 0, b, b > 0, 1, 1, 1)
    assert T[1 + 0, 1 + 1].tolist() == [1, 9, 4, 36, 81, 16] and T.sum() == 1 + 9 + 4 + 36 + 81 + 16


# ---------------------------------------------------------------- dsss_register_pyr_step against the reference's rule
def _same_step(sums, radius, min_cells, cell, level, cx, cy):
    """the library's step and the reference's on one table, bit for bit -> the reference's (record, usable, next)"""
    from diasss_amd import capi
    ref = P.step(sums, radius, min_cells, cell, level, cx, cy)
    dev = capi.register_pyr_step(sums.astype(np.uint64), radius, min_cells, cell, level, cx, cy)
    assert R.same_result(dev[0], ref[0]), "record %s, reference %s" % ({k: getattr(dev[0], k) for k in R.FIELDS}, ref[0])
    assert (bool(dev[1]), dev[2]) == (ref[1], ref[2])
    return ref


def test_step_centre_zero_is_the_peak(orc):
    from diasss_amd import capi
    ma, va, mb, vb = _layers(2, (2, -1))
    T = P.centred_sums(ma, va, mb, vb, 0, 0, 4)
    for level in range(4):
        rec, usable, nxt = _same_step(T, 4, 16, 0.1, level, 0, 0)
        plain = capi.mosaic_register_peak(T.astype(np.uint64), 4, max(1, 16 >> (2 * level)), 0.1 * 2 ** level)
        assert usable and R.same_result(plain, rec) and (rec["dx"], rec["dy"]) == (2, -1)
        assert nxt == ((4, -2) if level else None)


@pytest.mark.parametrize("centre", [(6, -4), (8, -6), (5, -5), "far"])
def test_step_with_a_centre_and_a_sub_cell_offset(orc, centre):
    if centre == "far":                                                  # the overlap lies 40 cells off, beyond any flat search
        ma, va, mb, vb = _layers(4, (0, 0), H=120, W=130); ma, va = ma[40:, :90], va[40:, :90]; mb, vb = mb[:80, 40:], vb[:80, 40:]
        cx, cy = -40 + 1, 40 - 2
        T = P.centred_sums(ma, va, mb, vb, cx, cy, 3)
        want = (-40, 40)
    else:
        cx, cy = centre
        ma, va, mb, vb = _layers(3, (7, -5))
        T = P.centred_sums(ma, va, mb, vb, cx, cy, 3)
        want = (7, -5)
    for level, cell in ((0, 0.1), (1, 0.1), (3, 0.37)):
        rec, usable, nxt = _same_step(T, 3, 16, cell, level, cx, cy)
        assert usable and (rec["dx"], rec["dy"]) == want and rec["on_border"] == 0
        cell_l = cell * 2 ** level
        plain = R.peak(T, 3, max(1, 16 >> (2 * level)), cell_l)
        assert plain["off_x"] != plain["dx"] * cell_l and plain["off_y"] != plain["dy"] * cell_l      # a sub-cell part on both axes
        assert rec["off_x"] == plain["off_x"] + float(cx) * cell_l and rec["off_y"] == plain["off_y"] + float(cy) * cell_l
        assert abs(rec["off_x"] - want[0] * cell_l) < 0.5 * cell_l and abs(rec["off_y"] - want[1] * cell_l) < 0.5 * cell_l
        assert (rec["zncc0"], rec["n0"]) == (plain["zncc0"], plain["n0"])                              # the table's centre shift
        assert nxt == ((2 * want[0], 2 * want[1]) if level else None)


def test_step_without_a_usable_shift(orc):
    from diasss_amd import capi
    ma, va, mb, vb = _layers(5, (1, 1))
    T = P.centred_sums(ma, va, mb, vb, 0, 0, 2)
    rec, usable, nxt = _same_step(T, 2, 100000, 0.1, 0, 9, -9)           # more cells asked for than any shift has
    assert not usable and nxt is None and (rec["dx"], rec["dy"], rec["zncc"], rec["off_x"], rec["off_y"], rec["on_border"]) == (0, 0, -2.0, 0.0, 0.0, 0)
    assert rec["n"] == rec["n0"] == int(T[2, 2, 0]) > 0
    Z = np.zeros((5, 5, 6), np.int64)
    rec, usable, nxt = _same_step(Z, 2, 1, 0.1, 2, 3, 4)
    assert not usable and rec["n0"] == 0
    # the next centre is not written without a usable shift, and not at level 0
    L = capi.lib()
    for sums, level, mc in ((Z, 2, 1), (T, 0, 16)):
        out = capi.RegResult(); u = C.c_int32(7); nx = C.c_int32(123); ny = C.c_int32(-456)
        s = np.ascontiguousarray(sums, np.uint64)
        assert L.dsss_register_pyr_step(capi._ptr(s), 2, mc, 0.1, level, 3, 4, C.byref(out), C.byref(u), C.byref(nx), C.byref(ny)) == 0
        assert u.value == (0 if sums is Z else 1) and (nx.value, ny.value) == (123, -456)


def test_step_min_cells_shifted_down_to_one(orc):
    """a table whose best shift has 3 cells: min_cells 40 is 40 >> 0 = 40, 40 >> 2 = 10, 40 >> 4 = 2, 40 >> 6 = 0 -> 1"""
    a = np.zeros((6, 7), np.int64); b = a.copy()
    a[1, 1], a[2, 4], a[4, 2] = 10, 200, 90
    b[2, 3], b[3, 6], b[5, 4] = 12, 190, 95                             # the same three cells, (2, 1) off
    T = P.centred_sums(a, a > 0, b, b > 0, 2, 0, 1)
    assert int(T[2, 1, 0]) == 3
    for level, usable in ((0, False), (1, False), (2, True), (3, True)):
        rec, u, nxt = _same_step(T, 1, 40, 0.1, level, 2, 0)
        assert u == usable
        if usable:
            assert (rec["dx"], rec["dy"], rec["n"], rec["on_border"]) == (2, 1, 3, 1) and nxt == (4, 2)
    rec, u, nxt = _same_step(T, 1, 48, 0.1, 2, 2, 0)                    # 48 >> 4 = 3: just enough
    assert u
    rec, u, nxt = _same_step(T, 1, 64, 0.1, 2, 2, 0)                    # 64 >> 4 = 4: one too many
    assert not u


def test_step_on_the_border(orc):
    ma, va, mb, vb = _layers(6, (7, -5))
    for cx, cy, border in ((4, -5, 1), (7, -2, 1), (10, -8, 1), (5, -4, 0)):
        T = P.centred_sums(ma, va, mb, vb, cx, cy, 3)
        rec, usable, nxt = _same_step(T, 3, 16, 0.1, 1, cx, cy)
        assert usable and (rec["dx"], rec["dy"]) == (7, -5) and rec["on_border"] == border and nxt == (14, -10)
        if border:                                                      # no parabola on the border: the offset is whole cells
            assert rec["off_x"] == float(7 - cx) * 0.2 + float(cx) * 0.2 and rec["off_y"] == float(-5 - cy) * 0.2 + float(cy) * 0.2


def test_step_argument_errors(orc):
    from diasss_amd import capi
    T = np.zeros((7, 7, 6), np.uint64)
    assert capi.register_pyr_step(T, 3, 16, 0.1, 3, 1 << 28, -(1 << 28))[1] == 0
    for args in ((None, 3, 16, 0.1, 0, 0, 0), (T, -1, 16, 0.1, 0, 0, 0), (T, 17, 16, 0.1, 0, 0, 0), (T, 3, 0, 0.1, 0, 0, 0), (T, 3, 16, 0.0, 0, 0, 0),
                 (T, 3, 16, -0.1, 0, 0, 0), (T, 3, 16, np.nan, 0, 0, 0), (T, 3, 16, np.inf, 0, 0, 0), (T, 3, 16, 0.1, -1, 0, 0), (T, 3, 16, 0.1, 4, 0, 0),
                 (T, 3, 16, 0.1, 1, (1 << 28) + 1, 0), (T, 3, 16, 0.1, 1, 0, -(1 << 28) - 1)):
        with pytest.raises(capi.DsssError) as ei:
            capi.register_pyr_step(*args)
        assert ei.value.code == E_ARG
    L = capi.lib()
    out = capi.RegResult(); u = C.c_int32(0); nx = C.c_int32(0); ny = C.c_int32(0)
    for o, uu, a, b in ((None, C.byref(u), C.byref(nx), C.byref(ny)), (C.byref(out), None, C.byref(nx), C.byref(ny)), (C.byref(out), C.byref(u), None, C.byref(ny)),
                        (C.byref(out), C.byref(u), C.byref(nx), None)):
        assert L.dsss_register_pyr_step(capi._ptr(T), 3, 16, 0.1, 1, 0, 0, o, uu, a, b) == E_ARG
    q = capi.reg_pyr_params_default()
    assert (q.levels, q.refine) == (1, REFINE)
    assert capi.REGSEGPYR_DTYPE.itemsize == C.sizeof(capi.RegSegPyr) == capi.REGSEG_DTYPE.itemsize + 8 + 32 + 32 and capi.REGSEGPYR_DTYPE["s"] == capi.REGSEG_DTYPE


# ---------------------------------------------------------------- preconditions of the GPU tests, on the reference alone
@pytest.fixture(scope="module")
def legs(orc):
    """the two legs of synth.Survey(2, 640, 400, seed=7) under their true poses"""
    from diasss_amd.synth import Survey
    sv = Survey(2, N, M, seed=7)
    fr = []
    for f in range(2):
        raw = sv.frame(f).numpy().copy()
        pose, alt, gr = sv.inputs(f)
        fr.append(dict(gr=gr, norm=orc.normalize(raw), mask=orc.mask(raw), true=np.ascontiguousarray(sv.poses_true[f])))
    return fr


def _survey(orc, fr, move):
    """leg 1 moved by `move` metres on the grid the GPU tests use -> (rows, grid, geo of both legs)"""
    from diasss_amd import capi
    rows = [fr[0]["true"], fr[1]["true"] + np.array([0, 0, 0, move[0], move[1], 0])]
    g = [orc.geo_img(np.ascontiguousarray(r), L["gr"], M) for r, L in zip(rows, fr)]
    gx = np.concatenate([a[0].ravel() for a in g]); gy = np.concatenate([a[1].ravel() for a in g])
    p = P.awkward_grid(lambda *v: capi.MosaicParams(*v, 0, 0), (gx.min(), gx.max(), gy.min(), gy.max()), CELL, g[1][0], g[1][1], SEG)
    return rows, p, g


def _pyr(fr, p, g, levels, radius=RADIUS, seg=SEG):
    acc = P.accumulators(g[0][0], g[0][1], fr[0]["norm"], fr[0]["mask"], p, 0)
    return P.register_segments_pyr(acc, g[1][0], g[1][1], fr[1]["norm"], fr[1]["mask"], p, seg, radius, MIN_CELLS, levels, REFINE)


def test_preconditions_inside_the_range(orc, legs):
    """Seen with this reference on the CPU, leg 1 moved by (2.3, -1.7) m, 80-ping segments, three levels, radius 8, refine 3: all 8
    segments end at exactly (23, -17) cells, no level on a border, final ZNCC 0.969 to 0.990 against at most 0.884 for the best other
    shift of the last table, 323 to 363 cells at the peak of level 2.  The flat radius-16 search of the whole frame ends on its border
    with ZNCC below 0.2; two levels (capture range 16) end with ZNCC below 0.24 in every segment."""
    rows, p, g = _survey(orc, legs, P.MOVE)
    assert p.W % 4 and p.H % 4
    win = P.segment_windows(g[1][0], g[1][1], p, SEG)
    assert any(ox % 2 for ox, _ in win) and any(oy % 2 for _, oy in win)
    out = _pyr(legs, p, g, 3)
    assert len(out) == 8
    nt, nr = (2 * RADIUS + 1) ** 2, (2 * REFINE + 1) ** 2
    for r in out:
        last = r["sums"][nt + nr:nt + 2 * nr]
        other = P.best_other(last, REFINE, MIN_CELLS, r["r"]["dx"] - 2 * r["lx"][1], r["r"]["dy"] - 2 * r["ly"][1])
        n2 = int(r["sums"][:nt].reshape(2 * RADIUS + 1, 2 * RADIUS + 1, 6)[r["ly"][2] + RADIUS, r["lx"][2] + RADIUS, 0])
        print("segment %d: level %d mask %d, t %s %s, zncc %s, best other %.3f, %d cells at the peak of level 2" % (
            r["seg"], r["level"], r["border_mask"], r["lx"], r["ly"], ["%.3f" % z for z in r["lz"]], other, n2))
        assert (r["level"], r["border_mask"], r["r"]["on_border"]) == (0, 0, 0)
        assert (r["r"]["dx"], r["r"]["dy"]) == (r["lx"][0], r["ly"][0]) == P.MOVE_CELLS
        assert r["r"]["zncc"] == r["lz"][0] >= 0.96 and r["r"]["zncc"] - other >= 0.08
        assert abs(r["r"]["off_x"] - P.MOVE[0]) < 0.5 * CELL and abs(r["r"]["off_y"] - P.MOVE[1]) < 0.5 * CELL
        assert r["sx"] > 0 and r["sy"] > 0 and n2 >= MIN_CELLS >> 4
    # every row is accepted as an edge, with an unambiguous anchor
    es, src = E.edges(orc, out, p, rows[0], 0, rows[1], N)
    assert src == list(range(8)) and all(e["lead"] > 1e-6 for e in es)
    # end to end under the oracle's solve: leg 1 lies 2.86 m off and comes back to 0.15 m (the edges' sigma is one cell, 0.1 m)
    dr = np.concatenate(rows); true = np.concatenate([legs[0]["true"], legs[1]["true"]])
    poses, stats = orc.pg_solve(dr, E.lc_edges(orc, es))
    s = E.rows_of_poses12(poses)
    d0 = float(np.hypot(dr[N:, 3] - true[N:, 3], dr[N:, 4] - true[N:, 4]).mean()); d1 = float(np.hypot(s[N:, 3] - true[N:, 3], s[N:, 4] - true[N:, 4]).mean())
    print("leg 1 off by %.3f m before, %.3f m after the oracle's solve" % (d0, d1))
    assert d0 > 2.8 and d1 < 0.1 * d0
    # the flat search of the widest radius on the same input: the whole frame as one segment
    la = P.layer(*P.accumulators(g[0][0], g[0][1], legs[0]["norm"], legs[0]["mask"], p, 0))
    flat = E.register_segments(la, g[1][0], g[1][1], legs[1]["norm"], legs[1]["mask"], p, N, 16, MIN_CELLS)
    print("flat radius 16: (%d, %d) zncc %.3f border %d" % (flat[0]["r"]["dx"], flat[0]["r"]["dy"], flat[0]["r"]["zncc"], flat[0]["r"]["on_border"]))
    assert len(flat) == 1 and flat[0]["r"]["on_border"] == 1 and flat[0]["r"]["zncc"] < 0.2
    per_seg = E.register_segments(la, g[1][0], g[1][1], legs[1]["norm"], legs[1]["mask"], p, SEG, 16, MIN_CELLS)
    assert all(r["r"]["zncc"] < 0.2 for r in per_seg) and not E.edges(orc, per_seg, p, rows[0], 0, rows[1], N)[0]
    # two levels are too few
    two = _pyr(legs, p, g, 2)
    print("two levels: zncc %s" % ["%.3f" % r["r"]["zncc"] for r in two])
    assert all(r["r"]["zncc"] < 0.3 for r in two) and not E.edges(orc, two, p, rows[0], 0, rows[1], N)[0]
    # one level is the flat reference
    one = _pyr(legs, p, g, 1)
    old = E.register_segments(la, g[1][0], g[1][1], legs[1]["norm"], legs[1]["mask"], p, SEG, RADIUS, MIN_CELLS)
    for a, b in zip(one, old):
        assert (a["sums"].reshape(b["sums"].shape) == b["sums"]).all() and a["r"] == b["r"] and (a["sx"], a["sy"]) == (b["sx"], b["sy"])
        assert a["border_mask"] == b["r"]["on_border"] and a["level"] == (0 if b["r"]["zncc"] > -2.0 else -1)


def test_preconditions_beyond_the_range(orc, legs):
    """leg 1 moved by (-3.1, 2.6) m: all 8 segments end at (-31, 26), and the top level sits on its border (-8 of 8) in all of them:
    bit 2 is set, the rows are flagged and give no edge"""
    rows, p, g = _survey(orc, legs, P.FAR)
    out = _pyr(legs, p, g, 3)
    assert len(out) == 8
    for r in out:
        assert r["level"] == 0 and r["border_mask"] & 4 and r["lx"][2] == -RADIUS and r["r"]["on_border"] == 1
        assert (r["r"]["dx"], r["r"]["dy"]) == P.FAR_CELLS
    assert E.edges(orc, out, p, rows[0], 0, rows[1], N) == ([], [])


def test_preconditions_of_the_search_that_stops(orc, legs):
    """A usable peak at level l means a valid cell of a meets a valid cell of the segment, so one level down the two windows meet within
    one cell of twice that shift: a search cannot stop on an empty region.  It stops where the overlap, counted in finer cells, falls
    under min_cells >> 2l: under the filter mask the first and last segments of leg 1 keep few cells."""
    from diasss_amd import capi
    rows, p, g = _survey(orc, legs, P.MOVE)
    p = capi.MosaicParams(p.x0, p.y0, p.cell, p.W, p.H, 1, 0)
    acc = P.accumulators(g[0][0], g[0][1], legs[0]["norm"], legs[0]["mask"], p, 1)
    out = P.register_segments_pyr(acc, g[1][0], g[1][1], legs[1]["norm"], legs[1]["mask"], p, SEG, RADIUS, MIN_CELLS, 3, REFINE)
    print("levels %s" % [r["level"] for r in out])
    stopped = [r for r in out if r["level"] > 0]
    nt, nr = (2 * RADIUS + 1) ** 2, (2 * REFINE + 1) ** 2
    assert stopped and any(r["level"] == 2 for r in stopped) and any(r["level"] == 0 for r in out) and any(r["level"] == -1 for r in out)
    for r in stopped:
        assert r["sx"] == r["sy"] == 0 and r["r"]["on_border"] == 1 and r["lz"][r["level"]] > -2.0 and r["lz"][r["level"] - 1] == -2.0
        if r["level"] == 2:
            assert not r["sums"][nt + nr:].any() and r["sums"][:nt].any()                 # level 0 was not reached: its table is zero
    assert not E.edges(orc, stopped, p, rows[0], 0, rows[1], N)[0]

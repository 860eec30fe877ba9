"""GPU parity of the dense loop closures over a cell pyramid: dsss_mosaic_register_segments_pyr (the six sums per shift of every (row,
level), every row's record, level, border bits, per-level shifts and scores and centroid sums equal to the numpy reference of
tests/register_pyr_ref.py bit for bit), its rows through the unchanged dsss_mosaic_register_edges, and both with the pose-graph solve
end to end.

Nothing expected comes from the code under test: geo coordinates are the oracle's geo_img, grey levels the oracle's normalised image,
the mask the oracle's filter mask, poses the oracle's Rodrigues construction.  Frames as in tests/test_gpu_register_segments.py: 0 and 1
are the two legs of synth.Survey(2, 640, 400, seed=7), 2 is the 500 x 700 geometry of test_gpu_mosaic_register.py, 3 is set and never
extracted.  The moved survey is the one tests/test_register_pyr_cpu.py proves the preconditions for: true rows, leg 1 moved by
(2.3, -1.7) m, or by (-3.1, 2.6) m beyond the reach of three levels, on a grid whose W and H are no multiples of 4 and on which
segment windows start on odd cells."""
import ctypes as C
import numpy as np
import pytest

from tests import mosaic_register_ref as R
from tests import register_edges_ref as E
from tests import register_pyr_ref as P
from tests.pg_report_ref import residual_bound

pytestmark = pytest.mark.gpu

E_ARG, E_STATE, E_CAPACITY = -2, -4, -5
N, M = 640, 400
N2, M2 = 500, 700
CELL, SEG, RADIUS, MIN_CELLS, REFINE = P.CELL, P.SEG, P.RADIUS, P.MIN_CELLS, P.REFINE


@pytest.fixture(scope="module")
def data(orc):
    from diasss_amd.synth import Survey
    from tests import helpers as H
    sv = Survey(2, N, M, seed=7)
    fr = []
    for f in range(2):
        raw = sv.frame(f).numpy().copy()
        pose, alt, gr = sv.inputs(f)
        fr.append(dict(N=N, M=M, raw=raw, pose=np.ascontiguousarray(pose), alt=alt, gr=gr, true=np.ascontiguousarray(sv.poses_true[f]),
                       norm=orc.normalize(raw), mask=orc.mask(raw)))
    pose, alt, gr = H.track(N2, M2, 1, seed=9)
    raw = np.random.default_rng(1).rayleigh(1.0, (N2, M2)) * 100.0
    fr.append(dict(N=N2, M=M2, raw=raw, pose=pose, alt=alt, gr=gr, true=np.ascontiguousarray(pose), norm=orc.normalize(raw), mask=orc.mask(raw)))
    return fr


@pytest.fixture(scope="module")
def ctx(data):
    from diasss_amd import capi
    c = capi.Context(max_frames=4)
    for i, L in enumerate(data):
        c.frame_set(i, L["raw"], L["N"], L["M"], L["pose"], L["alt"], L["gr"])
    c.extract_many([0, 1, 2])
    L = data[0]
    c.frame_set(3, L["raw"], L["N"], L["M"], L["pose"], L["alt"], L["gr"])          # set, never extracted
    yield c
    c.close()


def _moved(data, move):
    return [data[0]["true"], data[1]["true"] + np.array([0, 0, 0, move[0], move[1], 0])]


def _traj(rows):
    """rows of the listed frames packed with unrelated rows in front -> (rpy6, ping_off)"""
    parts, off, n = [], [], 0
    for k, r in enumerate(rows):
        parts.append(np.full((k + 2, 6), 7.0e5)); n += k + 2
        off.append(n); parts.append(r); n += len(r)
    return np.ascontiguousarray(np.concatenate(parts)), np.array(off, np.int32)


def _geo(orc, L, rows):
    return orc.geo_img(np.ascontiguousarray(rows), L["gr"], L["M"])


def _grid(orc, data, frames, rows, b, seg_pings, cell=CELL, use_mask=0):
    """the awkward grid over the listed frames: W, H no multiples of 4, windows of frame b's segments on odd cells (asserted)"""
    from diasss_amd import capi
    g = [_geo(orc, data[f], r) for f, r in zip(frames, rows)]
    gx = np.concatenate([a[0].ravel() for a in g]); gy = np.concatenate([a[1].ravel() for a in g])
    ok = np.isfinite(gx) & np.isfinite(gy)
    gb = g[frames.index(b)]
    p = P.awkward_grid(lambda *v: capi.MosaicParams(*v, 0, 0), (gx[ok].min(), gx[ok].max(), gy[ok].min(), gy[ok].max()), cell, gb[0], gb[1], seg_pings)
    win = P.segment_windows(gb[0], gb[1], p, seg_pings)
    assert p.W % 4 and p.H % 4 and any(ox % 2 for ox, _ in win) and any(oy % 2 for _, oy in win)
    p.use_mask = use_mask
    return p


def _reg(radius=RADIUS, min_cells=MIN_CELLS):
    from diasss_amd import capi
    return capi.RegParams(radius, min_cells)


def _pyr(levels, refine=REFINE):
    from diasss_amd import capi
    return capi.RegPyrParams(levels, refine)


def _ref_pair(orc, data, frames, rows, p, pair, seg_pings, levels, refine=REFINE, radius=RADIUS, min_cells=MIN_CELLS):
    """the reference's rows of one pair: frame pair[1] in segments against the whole of frame pair[0]"""
    a, b = pair
    ga = _geo(orc, data[a], rows[frames.index(a)]); gb = _geo(orc, data[b], rows[frames.index(b)])
    acc = P.accumulators(ga[0], ga[1], data[a]["norm"], data[a]["mask"], p, p.use_mask)
    return P.register_segments_pyr(acc, gb[0], gb[1], data[b]["norm"], data[b]["mask"], p, seg_pings, radius, min_cells, levels, refine)


def _run(ctx, frames, rows, p, pairs, seg_pings, levels, refine=REFINE, radius=RADIUS, min_cells=MIN_CELLS, **kw):
    rpy, off = _traj(rows)
    return ctx.mosaic_register_segments_pyr(frames, p, pairs, seg_pings, pyr=_pyr(levels, refine), reg=_reg(radius, min_cells), rpy6=rpy, ping_off=off,
                                            want_sums=True, **kw)


def _bits(x):
    return np.asarray(x, np.float64).tobytes()


def _same_rows(dev, sums, k0, pair_index, ref):
    """rows k0 .. of the device against the reference's rows of one pair; returns the next row"""
    for s, rr in enumerate(ref):
        d = dev[k0 + s]
        assert (int(d["s"]["pair"]), int(d["s"]["seg"]), int(d["s"]["p0"]), int(d["s"]["p1"])) == (pair_index, rr["seg"], rr["p0"], rr["p1"])
        bad = np.argwhere(sums[k0 + s].astype(np.int64) != rr["sums"])
        assert len(bad) == 0, "pair %d segment %d: %d sums differ, first at [shift, q] = %s: %d, reference %d" % (
            pair_index, s, len(bad), bad[0].tolist(), sums[k0 + s][tuple(bad[0])], rr["sums"][tuple(bad[0])])
        assert (int(d["level"]), int(d["border_mask"])) == (rr["level"], rr["border_mask"]), "pair %d segment %d: level %d mask %d, reference %d %d" % (
            pair_index, s, d["level"], d["border_mask"], rr["level"], rr["border_mask"])
        assert d["lx"].tolist() == rr["lx"] and d["ly"].tolist() == rr["ly"] and _bits(d["lz"]) == _bits(rr["lz"]), "pair %d segment %d: levels %s %s %s, reference %s %s %s" % (
            pair_index, s, d["lx"], d["ly"], d["lz"], rr["lx"], rr["ly"], rr["lz"])
        assert R.same_result(d["s"]["r"], rr["r"]), "pair %d segment %d: result %s, reference %s" % (pair_index, s, d["s"]["r"], rr["r"])
        assert (int(d["s"]["sx"]), int(d["s"]["sy"])) == (rr["sx"], rr["sy"]), "pair %d segment %d: centroid sums" % (pair_index, s)
    return k0 + len(ref)


def _equal(ctx, orc, data, frames, rows, p, pairs, seg_pings, levels, **kw):
    """device rows and sums of the pairs against the reference; returns (device rows, sums, the reference's rows per pair)"""
    dev, sums = _run(ctx, frames, rows, p, pairs, seg_pings, levels, **kw)
    refs = [_ref_pair(orc, data, frames, rows, p, pr, seg_pings, levels, **kw) for pr in pairs]
    assert len(dev) == sum(len(r) for r in refs) == len(sums)
    k = 0
    for i, ref in enumerate(refs):
        k = _same_rows(dev, sums, k, i, ref)
    return dev, sums, refs


# ---------------------------------------------------------------- 1. exact sums and records of every level
@pytest.mark.parametrize("levels,seg_pings,use_mask,order", [(3, 80, 0, (0, 1)), (3, 96, 0, (0, 1)), (3, 80, 1, (0, 1)), (3, 80, 0, (1, 0)), (4, 80, 0, (0, 1)),
                                                             (2, 80, 0, (0, 1))])
def test_exact_sums_and_records(ctx, orc, data, levels, seg_pings, use_mask, order):
    rows = _moved(data, P.MOVE)
    p = _grid(orc, data, [0, 1], rows, order[1], seg_pings, use_mask=use_mask)
    dev, sums, (ref,) = _equal(ctx, orc, data, [0, 1], rows, p, [order], seg_pings, levels)
    assert len(ref) == (8 if seg_pings == 80 else 7) and ref[-1]["p1"] - ref[-1]["p0"] == (80 if seg_pings == 80 else 64)
    print("levels %d seg %d mask %d pair %s: level %s, mask %s, t0 %s, zncc %s" % (levels, seg_pings, use_mask, order, [r["level"] for r in ref],
          [r["border_mask"] for r in ref], [(r["r"]["dx"], r["r"]["dy"]) for r in ref], ["%.3f" % r["r"]["zncc"] for r in ref]))
    done = [r for r in ref if r["level"] == 0]
    nt = (2 * RADIUS + 1) ** 2
    # the comparison is not of zeros: every finished row has sums at every level and a centroid
    assert all(r["sums"][:nt].any() and r["sums"][nt:].any() and r["sx"] > 0 and r["sy"] > 0 for r in done)
    want = P.MOVE_CELLS if order == (0, 1) else (-P.MOVE_CELLS[0], -P.MOVE_CELLS[1])
    if levels >= 3 and not use_mask:                                    # the recovered offset, beyond any flat search
        assert len(done) == len(ref) and all((r["r"]["dx"], r["r"]["dy"]) == want and r["border_mask"] == 0 for r in ref)
        assert (dev["s"]["r"]["dx"] == want[0]).all() and (dev["s"]["r"]["dy"] == want[1]).all() and not dev["s"]["r"]["on_border"].any()
    if use_mask:                                                        # the mask leaves the outer segments few cells: rows that stop on the way
        assert len(done) >= 3 and all((r["r"]["dx"], r["r"]["dy"]) == want for r in done) and any(r["level"] != 0 for r in ref)
    if levels == 2:                                                     # a capture range of 16 cells is too short
        assert all(r["r"]["zncc"] < 0.3 for r in ref)


# ---------------------------------------------------------------- 2. one level is the existing registration
@pytest.mark.parametrize("seg_pings", [97, N])
def test_one_level_is_the_existing_call(ctx, orc, data, seg_pings):
    rows = _moved(data, (0.23, -0.17))
    p = _grid(orc, data, [0, 1], rows, 1, SEG, use_mask=1)
    rpy, off = _traj(rows)
    pairs = [(0, 1), (1, 0)]
    old, osums = ctx.mosaic_register_segments([0, 1], p, pairs, seg_pings, reg=_reg(), rpy6=rpy, ping_off=off, want_sums=True)
    assert len(old) > 0 and osums.any() and (old["r"]["zncc"] > 0.5).any()
    for pyr in (_pyr(1), _pyr(1, 0), _pyr(1, 99), None):                # refine is ignored with one level
        new, nsums = ctx.mosaic_register_segments_pyr([0, 1], p, pairs, seg_pings, pyr=pyr, reg=_reg(), rpy6=rpy, ping_off=off, want_sums=True)
        assert len(new) == len(old)
        assert np.ascontiguousarray(new["s"]).tobytes() == old.tobytes() and nsums.tobytes() == osums.tobytes()
        assert (new["border_mask"] == old["r"]["on_border"]).all() and (new["level"] == np.where(old["r"]["zncc"] > -2.0, 0, -1)).all()
        assert _bits(new["lz"][:, 0]) == _bits(np.ascontiguousarray(old["r"]["zncc"])) and (new["lz"][:, 1:] == -2.0).all()
        ok = old["r"]["zncc"] > -2.0
        assert (new["lx"][:, 0] == np.where(ok, old["r"]["dx"], 0)).all() and (new["ly"][:, 0] == np.where(ok, old["r"]["dy"], 0)).all() and not new["lx"][:, 1:].any()


# ---------------------------------------------------------------- 3. flags
def test_a_leg_beyond_the_range_is_flagged(ctx, orc, data):
    rows = _moved(data, P.FAR)
    p = _grid(orc, data, [0, 1], rows, 1, SEG)
    dev, sums, (ref,) = _equal(ctx, orc, data, [0, 1], rows, p, [(0, 1)], SEG, 3)
    assert len(ref) == 8 and all(r["border_mask"] & 4 and r["level"] == 0 for r in ref)
    assert (dev["border_mask"] & 4 != 0).all() and (dev["s"]["r"]["on_border"] == 1).all() and (dev["s"]["r"]["zncc"] > 0.9).all()
    rpy, off = _traj(rows)
    edges, src = ctx.mosaic_register_edges([0, 1], p, [(0, 1)], np.ascontiguousarray(dev["s"]), rpy6=rpy, ping_off=off)
    assert len(edges) == 0 and len(src) == 0


# ---------------------------------------------------------------- 4. a search that stops on the way
def test_a_search_that_stops_on_the_way(ctx, orc, data):
    """the case tests/test_register_pyr_cpu.py::test_preconditions_of_the_search_that_stops proves on the reference: under the filter
    mask outer segments of leg 1 have a usable peak on a coarse level and too few cells one level down"""
    rows = _moved(data, P.MOVE)
    p = _grid(orc, data, [0, 1], rows, 1, SEG, use_mask=1)
    dev, sums, (ref,) = _equal(ctx, orc, data, [0, 1], rows, p, [(0, 1)], SEG, 3)
    stopped = [k for k, r in enumerate(ref) if r["level"] > 0]
    nt, nr = (2 * RADIUS + 1) ** 2, (2 * REFINE + 1) ** 2
    assert stopped and any(ref[k]["level"] == 2 for k in stopped)
    for k in stopped:
        d = dev[k]
        assert int(d["level"]) == ref[k]["level"] > 0 and int(d["s"]["sx"]) == 0 and int(d["s"]["sy"]) == 0 and int(d["s"]["r"]["on_border"]) == 1
        if ref[k]["level"] == 2:
            assert not sums[k][nt + nr:].any() and sums[k][:nt].any()   # level 0 was not reached: its table is zero
    rpy, off = _traj(rows)
    edges, src = ctx.mosaic_register_edges([0, 1], p, [(0, 1)], np.ascontiguousarray(dev["s"]), rpy6=rpy, ping_off=off)
    assert not set(src.tolist()) & set(stopped) and len(edges) == sum(r["level"] == 0 and r["r"]["zncc"] >= E.MIN_ZNCC for r in ref) > 0


# ---------------------------------------------------------------- 5. pairs without overlap, one frame as b of several pairs
def test_a_pair_without_overlap(ctx, orc, data):
    """frame 2 moved 300 m aside, on a grid that holds both: every window is on the grid and none within the radius of a's at any level"""
    from diasss_amd import capi
    far = [data[0]["true"], data[2]["true"] + np.array([0, 0, 0, 0, 300.0, 0])]
    g = [_geo(orc, data[f], r) for f, r in zip((0, 2), far)]
    gx = np.concatenate([a[0].ravel() for a in g]); gy = np.concatenate([a[1].ravel() for a in g])
    wide = capi.mosaic_grid((gx.min(), gx.max(), gy.min(), gy.max()), 0.5); wide.use_mask = 0
    assert wide.H > 600
    dev, sums = _run(ctx, [0, 2], far, wide, [(0, 2), (2, 0)], 128, 3)
    assert len(dev) == 4 + 5 and sums.shape == (9, 17 * 17 + 2 * 49, 6) and not sums.any()
    zero = P.step(np.zeros((2 * RADIUS + 1, 2 * RADIUS + 1, 6), np.int64), RADIUS, MIN_CELLS, wide.cell, 2, 0, 0)[0]
    for d in dev:
        assert R.same_result(d["s"]["r"], zero) and (int(d["level"]), int(d["border_mask"])) == (-1, 0)
        assert not d["lx"].any() and not d["ly"].any() and (d["lz"] == -2.0).all() and int(d["s"]["sx"]) == 0 and int(d["s"]["sy"]) == 0
    assert dev["s"]["seg"].tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 4] and dev["s"]["pair"].tolist() == [0] * 4 + [1] * 5


def test_one_frame_as_b_of_several_pairs(ctx, orc, data):
    """frame 1 is the b of three pairs, two of them the same: it is rendered once, the rows of the equal pairs are equal, and frame 0
    is an a and a b in one call.  (The kernels of this section have no slot in the profile, so the launch count does not show there.)"""
    rows = _moved(data, P.MOVE) + [data[2]["true"]]
    p = _grid(orc, data, [0, 1, 2], rows, 1, 160, use_mask=0)
    pairs = [(0, 1), (2, 1), (0, 1), (1, 0)]
    dev, sums, refs = _equal(ctx, orc, data, [0, 1, 2], rows, p, pairs, 160, 3)
    assert len(refs[0]) == 4 and all(r["level"] == 0 for r in refs[0])
    a, b = dev[0:4], dev[8:12]
    assert (b["s"]["pair"] == 2).all() and sums[0:4].tobytes() == sums[8:12].tobytes()
    for f in ("level", "border_mask", "lx", "ly", "lz"):
        assert a[f].tobytes() == b[f].tobytes()
    for f in ("seg", "p0", "p1", "r", "sx", "sy"):
        assert np.ascontiguousarray(a["s"][f]).tobytes() == np.ascontiguousarray(b["s"][f]).tobytes()


# ---------------------------------------------------------------- 6. rules
def test_rules(ctx, orc, data):
    from diasss_amd import capi
    rows = _moved(data, P.MOVE) + [data[2]["true"]]
    p = _grid(orc, data, [0, 1, 2], rows, 1, SEG, cell=0.2, use_mask=1)
    pairs = [(0, 1), (1, 0), (0, 2)]
    good = _run(ctx, [0, 1, 2], rows, p, pairs, 80, 3)
    nseg = 8 + 8 + 7
    assert len(good[0]) == nseg and good[1].any() and (good[0]["level"] == 0).any()
    rpy, off = _traj(rows)

    def call(prs=pairs, seg_pings=80, ids=(0, 1, 2), pyr=_pyr(3), reg=_reg(), **kw):
        return ctx.mosaic_register_segments_pyr(list(ids), p, prs, seg_pings, pyr=pyr, reg=reg, rpy6=rpy, ping_off=off, **kw)

    bad = [_pyr(0), _pyr(5), _pyr(-1), _pyr(2, 0), _pyr(3, 17), _pyr(4, -2)]
    for code, fn in [(E_ARG, lambda q=q: call(pyr=q)) for q in bad] + [
            (E_ARG, lambda: call(seg_pings=0)), (E_ARG, lambda: call(seg_pings=-5)), (E_CAPACITY, lambda: call(cap=nseg - 1)),
            (E_CAPACITY, lambda: call(cap=0)), (E_ARG, lambda: call(prs=[(0, 0)])), (E_ARG, lambda: call(prs=[(0, 3)])), (E_ARG, lambda: call(reg=_reg(17))),
            (E_ARG, lambda: call(reg=_reg(8, 0))),
            (E_STATE, lambda: ctx.mosaic_register_segments_pyr([0, 3], p, [(0, 3)], 80, pyr=_pyr(3), reg=_reg()))]:          # frame 3 is not extracted
        with pytest.raises(capi.DsssError) as ei:
            fn()
        assert ei.value.code == code
    # a refusal comes before anything is written or launched: the output rows stay as they were, the count comes back
    ids = np.array([0, 1, 2], np.int32); pa = np.array([0, 1, 0], np.int32); pb = np.array([1, 0, 2], np.int32)
    one = np.zeros(1, capi.REGSEGPYR_DTYPE); n = C.c_int(-1); q = _pyr(3)
    rc = ctx.L.dsss_mosaic_register_segments_pyr(ctx.h, capi._ptr(ids), 3, capi._ptr(rpy), capi._ptr(off), C.byref(p), capi._ptr(pa), capi._ptr(pb), 3, 80,
                                                 C.byref(_reg()), C.byref(q), capi._ptr(one), 1, C.byref(n), None)
    assert rc == E_CAPACITY and n.value == nseg and not one.tobytes().strip(b"\0")
    full = np.full(nseg, 0x55, np.uint8).repeat(capi.REGSEGPYR_DTYPE.itemsize).view(capi.REGSEGPYR_DTYPE); q = _pyr(5)
    before = full.tobytes()
    rc = ctx.L.dsss_mosaic_register_segments_pyr(ctx.h, capi._ptr(ids), 3, capi._ptr(rpy), capi._ptr(off), C.byref(p), capi._ptr(pa), capi._ptr(pb), 3, 80,
                                                 C.byref(_reg()), C.byref(q), capi._ptr(full), nseg, C.byref(n), None)
    assert rc == E_ARG and full.tobytes() == before
    assert len(call(prs=[])) == 0
    again = _run(ctx, [0, 1, 2], rows, p, pairs, 80, 3)                 # after the refusals, and twice: identical bytes
    assert again[0].tobytes() == good[0].tobytes() and again[1].tobytes() == good[1].tobytes()
    exact = _run(ctx, [0, 1, 2], rows, p, pairs, 80, 3, cap=nseg)
    assert exact[0].tobytes() == good[0].tobytes()
    # the frames in another order, one pair alone, without the sums: the same rows
    r = _run(ctx, [2, 1, 0], rows[::-1], p, pairs, 80, 3)
    assert r[0].tobytes() == good[0].tobytes() and r[1].tobytes() == good[1].tobytes()
    alone = _run(ctx, [0, 1, 2], rows, p, [pairs[1]], 80, 3)
    assert alone[1].tobytes() == good[1][8:16].tobytes()
    for f in ("level", "border_mask", "lx", "ly", "lz"):
        assert alone[0][f].tobytes() == good[0][f][8:16].tobytes()
    assert np.ascontiguousarray(alone[0]["s"]["r"]).tobytes() == np.ascontiguousarray(good[0]["s"]["r"][8:16]).tobytes()
    assert call().tobytes() == good[0].tobytes()
    # another call of the section in between leaves nothing behind
    ctx.mosaic_register_segments([0, 1, 2], p, pairs, 80, reg=_reg(), rpy6=rpy, ping_off=off)
    assert call().tobytes() == good[0].tobytes()


def test_more_than_one_rank_is_a_state_error():
    from diasss_amd import capi
    c = capi.Context(max_frames=2)
    try:
        c.comm_init_callback(0, 2, lambda op, arr: None)
        p = capi.MosaicParams(0.0, 0.0, 0.1, 10, 10, 0, 0)
        with pytest.raises(capi.DsssError) as ei:
            c.mosaic_register_segments_pyr([0, 1], p, [(0, 1)], 80, pyr=_pyr(3))
        assert ei.value.code == E_STATE and "rank" in str(ei.value)
    finally:
        c.close()


# ---------------------------------------------------------------- 7. end to end on the device
def test_pyramid_edges_bring_the_leg_back(ctx, orc, data):
    """The rows of three levels through the unchanged dsss_mosaic_register_edges and dsss_posegraph_solve_edges on the moved
    trajectory: leg 1, 2.86 m off, comes back towards its true place; the solve is the oracle's of the same edges at the tolerance
    tests/test_gpu_register_segments.py::test_segments_edges_solve_register_again uses.  The flat call of the same pair gives no edge."""
    rows = _moved(data, P.MOVE)
    p = _grid(orc, data, [0, 1], rows, 1, SEG)
    dr = np.ascontiguousarray(np.concatenate(rows)); off = np.array([0, N], np.int32)
    segs = ctx.mosaic_register_segments_pyr([0, 1], p, [(0, 1)], SEG, pyr=_pyr(3), reg=_reg(), rpy6=dr, ping_off=off)
    edges, src = ctx.mosaic_register_edges([0, 1], p, [(0, 1)], np.ascontiguousarray(segs["s"]), rpy6=dr, ping_off=off)
    assert len(segs) == 8 and src.tolist() == list(range(8))
    ref = _ref_pair(orc, data, [0, 1], rows, p, (0, 1), SEG, 3)
    es, ss = E.edges(orc, ref, p, rows[0], 0, rows[1], N)
    assert ss == list(range(8)) and all(e["lead"] > 1e-6 for e in es)
    for d, r in zip(edges, es):
        assert (int(d["a"]), int(d["b"])) == (r["a"], r["b"])
        for name in ("rel", "var"):
            assert (np.abs(d[name] - r[name]) <= residual_bound(r[name], 1.0)).all(), "%s: %s, reference %s" % (name, d[name], r[name])
    flat = ctx.mosaic_register_segments([0, 1], p, [(0, 1)], SEG, reg=_reg(16), rpy6=dr, ping_off=off)
    assert len(ctx.mosaic_register_edges([0, 1], p, [(0, 1)], flat, rpy6=dr, ping_off=off)[0]) == 0
    poses, stats = ctx.posegraph_solve_edges(dr, edges)
    o_poses, o_stats = orc.pg_solve(dr, edges)
    err = float(np.abs(poses - o_poses).max())
    true = np.concatenate([data[0]["true"], data[1]["true"]])
    solved = E.rows_of_poses12(poses)
    d0 = float(np.hypot(dr[N:, 3] - true[N:, 3], dr[N:, 4] - true[N:, 4]).mean()); d1 = float(np.hypot(solved[N:, 3] - true[N:, 3], solved[N:, 4] - true[N:, 4]).mean())
    print("max |pose - oracle| %.3g, LM iterations %d (oracle %d); leg 1 off by %.3f m before, %.3f m after" % (err, int(stats[0]), int(o_stats[0]), d0, d1))
    assert err < 1e-6
    assert d0 > 2.8 and d1 < 0.1 * d0 + 1e-6                           # the oracle's figure (tests/test_register_pyr_cpu.py) at the tolerance above

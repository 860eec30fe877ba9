"""GPU parity of the dense loop closures: dsss_mosaic_register_segments (every segment's six sums per shift, its result record and its
centroid sums equal to the numpy reference of tests/register_edges_ref.py bit for bit), dsss_mosaic_register_edges (the reference's
edge set) and the three of them with the pose-graph solve end to end.

Nothing expected comes from the code under test: geo coordinates are the oracle's geo_img, grey levels the oracle's normalised image,
the mask the oracle's filter mask, poses the oracle's Rodrigues construction.  Frames as in tests/test_gpu_mosaic_register.py: 0 and 1
are the two legs of synth.Survey(2, 640, 400, seed=7), 2 is the 500 x 700 geometry of test_gpu_mosaic.py, 3 is set and never extracted.
The drifted survey is the one tests/test_register_edges_cpu.py proves the preconditions for: dead-reckoning rows, leg 1 with E.drift."""
import ctypes as C
import numpy as np
import pytest

from tests import mosaic_register_ref as R
from tests import register_edges_ref as E
from tests.pg_report_ref import residual_bound

pytestmark = pytest.mark.gpu

E_ARG, E_STATE, E_CAPACITY = -2, -4, -5
N, M = 640, 400
N2, M2 = 500, 700
RADIUS, MIN_CELLS = 8, 256


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


@pytest.fixture(scope="module")
def drifted(data):
    """the rows of the drifted survey: dead reckoning, leg 1 with the drift of the feasibility check"""
    return [data[0]["pose"], E.drift(data[1]["pose"])]


def _traj(rows):
    """rows of the listed frames packed with unrelated rows in front -> (rpy6, ping_off)"""
    parts, off, n = [], [], 0
    for k, r in enumerate(rows):
        parts.append(np.full((k + 2, 6), 7.0e5)); n += k + 2
        off.append(n); parts.append(r); n += len(r)
    return np.ascontiguousarray(np.concatenate(parts)), np.array(off, np.int32)


def _geo(orc, L, rows):
    return orc.geo_img(np.ascontiguousarray(rows), L["gr"], L["M"])


def _grid(orc, data, frames, rows, cell, use_mask=0):
    from diasss_amd import capi
    g = [_geo(orc, data[f], r) for f, r in zip(frames, rows)]
    gx = np.concatenate([a[0].ravel() for a in g]); gy = np.concatenate([a[1].ravel() for a in g])
    ok = np.isfinite(gx) & np.isfinite(gy)
    p = capi.mosaic_grid((gx[ok].min(), gx[ok].max(), gy[ok].min(), gy[ok].max()), cell)
    p.use_mask = use_mask
    return p


def _reg(radius=RADIUS, min_cells=MIN_CELLS):
    from diasss_amd import capi
    return capi.RegParams(radius, min_cells)


def _ref_pair(orc, data, frames, rows, p, pair, seg_pings, radius=RADIUS, min_cells=MIN_CELLS):
    """the reference's rows of one pair: frame pair[1] in segments against the whole of frame pair[0]"""
    a, b = pair
    ra, rb = rows[frames.index(a)], rows[frames.index(b)]
    ga = _geo(orc, data[a], ra); gb = _geo(orc, data[b], rb)
    la = R.mean_layer(ga[0], ga[1], data[a]["norm"], data[a]["mask"], p, p.use_mask)
    return E.register_segments(la, gb[0], gb[1], data[b]["norm"], data[b]["mask"], p, seg_pings, radius, min_cells)


def _run(ctx, frames, rows, p, pairs, seg_pings, radius=RADIUS, min_cells=MIN_CELLS, **kw):
    rpy, off = _traj(rows)
    return ctx.mosaic_register_segments(frames, p, pairs, seg_pings, reg=_reg(radius, min_cells), rpy6=rpy, ping_off=off, want_sums=True, **kw)


def _same_rows(dev, sums, k0, pair_index, ref):
    """rows k0 .. of the device against the reference's rows of one pair; returns the next row"""
    for s, rr in enumerate(ref):
        d = dev[k0 + s]
        assert (int(d["pair"]), int(d["seg"]), int(d["p0"]), int(d["p1"])) == (pair_index, rr["seg"], rr["p0"], rr["p1"])
        bad = np.argwhere(sums[k0 + s].astype(np.int64) != rr["sums"])
        assert len(bad) == 0, "pair %d segment %d: %d sums differ, first at [dy, dx, q] = %s: %d, reference %d" % (
            pair_index, s, len(bad), bad[0].tolist(), sums[k0 + s][tuple(bad[0])], rr["sums"][tuple(bad[0])])
        assert R.same_result(d["r"], rr["r"]), "pair %d segment %d: result %s, reference %s" % (pair_index, s, d["r"], rr["r"])
        assert (int(d["sx"]), int(d["sy"])) == (rr["sx"], rr["sy"]), "pair %d segment %d: centroid sums" % (pair_index, s)
    return k0 + len(ref)


def _equal(ctx, orc, data, frames, rows, p, pairs, seg_pings, radius=RADIUS, min_cells=MIN_CELLS):
    """device rows and sums of the pairs against the reference; returns (device rows, the reference's rows per pair)"""
    dev, sums = _run(ctx, frames, rows, p, pairs, seg_pings, radius, min_cells)
    refs = [_ref_pair(orc, data, frames, rows, p, pr, seg_pings, radius, min_cells) for pr in pairs]
    assert len(dev) == sum(len(r) for r in refs) == len(sums)
    k = 0
    for i, ref in enumerate(refs):
        k = _same_rows(dev, sums, k, i, ref)
    return dev, refs


# ---------------------------------------------------------------- 1. exact sums and records
@pytest.mark.parametrize("seg_pings", [80, 97])
@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
@pytest.mark.parametrize("use_mask", [0, 1])
@pytest.mark.parametrize("cell", [0.1, 0.5])
def test_exact_sums_and_records(ctx, orc, data, drifted, cell, use_mask, order, seg_pings):
    p = _grid(orc, data, [0, 1], drifted, cell, use_mask)
    dev, (ref,) = _equal(ctx, orc, data, [0, 1], drifted, p, [order], seg_pings)
    assert len(ref) == (8 if seg_pings == 80 else 7) and ref[-1]["p1"] - ref[-1]["p0"] == (80 if seg_pings == 80 else 58)
    usable = [r for r in ref if r["r"]["zncc"] > -2.0]
    print("cell %g mask %d pair %s seg %d: %d rows, %d with a peak, n %s" % (cell, use_mask, order, seg_pings, len(ref), len(usable), [r["r"]["n"] for r in ref]))
    # the comparison is not of zeros: the mask leaves the first and the last segment without overlap, every other one has some
    assert sum(bool(r["sums"].any()) for r in ref) >= len(ref) - 2 and all(r["sx"] > 0 and r["sy"] > 0 for r in usable)
    if not use_mask:
        assert len(usable) >= len(ref) - 1


# ---------------------------------------------------------------- 2. the whole frame as one segment
@pytest.mark.parametrize("seg_pings", [N, 1000])
def test_whole_frame_as_one_segment(ctx, orc, data, drifted, seg_pings):
    p = _grid(orc, data, [0, 1], drifted, 0.1, 1)
    rpy, off = _traj(drifted)
    pairs = [(0, 1), (1, 0)]
    whole, wsums = ctx.mosaic_register([0, 1], p, pairs, reg=_reg(), rpy6=rpy, ping_off=off, want_sums=True)
    dev, sums = ctx.mosaic_register_segments([0, 1], p, pairs, seg_pings, reg=_reg(), rpy6=rpy, ping_off=off, want_sums=True)
    assert len(dev) == 2 and wsums.any()
    assert sums.tobytes() == wsums.tobytes() and np.ascontiguousarray(dev["r"]).tobytes() == whole.tobytes()
    assert dev["pair"].tolist() == [0, 1] and dev["seg"].tolist() == [0, 0] and dev["p0"].tolist() == [0, 0] and dev["p1"].tolist() == [N, N]
    assert (dev["sx"] > 0).all() and (dev["sy"] > 0).all()


# ---------------------------------------------------------------- 3. shapes where the new kernels can go wrong
def test_grid_cropped_to_the_middle_third(ctx, orc, data, drifted):
    """segments wholly outside the grid (no window, zero sums) next to segments that straddle its edge"""
    from diasss_amd import capi
    full = _grid(orc, data, [0, 1], drifted, 0.1, 0)
    q = capi.MosaicParams(full.x0 + (full.W // 3) * full.cell, full.y0 + (full.H // 3) * full.cell, full.cell, full.W // 3, full.H // 3, 0, 0)
    dev, refs = _equal(ctx, orc, data, [0, 1], drifted, q, [(0, 1), (1, 0)], 80)
    for ref in refs:
        n0 = [r["r"]["n0"] for r in ref]
        empty = [r for r in ref if not r["sums"].any()]
        print("n0 per segment %s" % n0)
        assert len(empty) >= 2 and max(n0) > 1000 and len(empty) < len(ref)
        assert all(r["r"]["n"] == 0 and r["sx"] == 0 and r["sy"] == 0 and r["r"]["zncc"] == -2.0 for r in empty)


def test_windows_narrower_than_a_tile(ctx, orc, data, drifted):
    """seg_pings 7: 92 segments of frame 0, of which only the first ten (70 pings) are on the grid, each some four cells wide"""
    rows0 = drifted[0].copy(); rows0[70:, 3] += 1.0e5
    rows = [rows0, drifted[1]]
    p = _grid(orc, data, [0, 1], drifted, 0.1, 0)
    dev, (ref,) = _equal(ctx, orc, data, [0, 1], rows, p, [(1, 0)], 7)
    assert len(ref) == 92 and ref[-1]["p1"] == N and ref[-1]["p1"] - ref[-1]["p0"] == 3
    assert all(not r["sums"].any() for r in ref[10:]) and all(r["sums"].any() for r in ref[:10])
    print("zncc of the ten segments %s" % ["%.3f" % r["r"]["zncc"] for r in ref[:10]])
    assert sum(r["r"]["zncc"] > -2.0 for r in ref[:10]) >= 5


def test_mixed_geometries_and_windows_out_of_reach(ctx, orc, data):
    rows = [data[0]["true"], data[2]["true"]]
    p = _grid(orc, data, [0, 2], rows, 0.5, 0)
    dev, (ref,) = _equal(ctx, orc, data, [0, 2], rows, p, [(0, 2)], 128)
    assert [(r["p0"], r["p1"]) for r in ref] == [(0, 128), (128, 256), (256, 384), (384, 500)] and any(r["r"]["n0"] > 100 for r in ref)
    # frame 2 moved 300 m aside, on a grid that holds both: every window is on the grid and none within the radius of a's
    far = [data[0]["true"], data[2]["true"] + np.array([0, 0, 0, 0, 300.0, 0])]
    wide = _grid(orc, data, [0, 2], far, 0.5, 0)
    assert wide.H > 600
    dev, sums = _run(ctx, [0, 2], far, wide, [(0, 2), (2, 0)], 128)
    assert len(dev) == 4 + 5 and not sums.any()
    zero = R.peak(np.zeros((2 * RADIUS + 1, 2 * RADIUS + 1, 6), np.int64), RADIUS, MIN_CELLS, wide.cell)
    for d in dev:
        assert R.same_result(d["r"], zero) and d["r"]["zncc"] == -2.0 and int(d["sx"]) == 0 and int(d["sy"]) == 0
    assert dev["seg"].tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 4] and dev["pair"].tolist() == [0] * 4 + [1] * 5


def test_one_frame_as_b_of_two_pairs(ctx, orc, data, drifted):
    """the segment layers of frame 1 are rendered once and read by both pairs"""
    rows = [drifted[0], drifted[1], data[2]["true"]]
    p = _grid(orc, data, [0, 1, 2], rows, 0.1, 1)
    dev, refs = _equal(ctx, orc, data, [0, 1, 2], rows, p, [(0, 1), (2, 1)], 160)
    assert len(refs[0]) == len(refs[1]) == 4 and any(r["r"]["n0"] > 1000 for r in refs[0])
    print("n0: pair (0, 1) %s, pair (2, 1) %s" % ([r["r"]["n0"] for r in refs[0]], [r["r"]["n0"] for r in refs[1]]))


# ---------------------------------------------------------------- 4. edges
def _same_edges(dev_edges, dev_src, ref_edges, ref_src):
    assert dev_src.tolist() == ref_src
    for d, r in zip(dev_edges, ref_edges):
        assert (int(d["a"]), int(d["b"])) == (r["a"], r["b"])
        for name in ("rel", "var"):
            assert (np.abs(d[name] - r[name]) <= residual_bound(r[name], 1.0)).all(), "%s: %s, reference %s" % (name, d[name], r[name])


@pytest.mark.parametrize("further", [0.0, 3.0])
def test_edges_are_the_references(ctx, orc, data, drifted, further):
    """further = 3: leg 1 another 3 m off, beyond the search radius of 0.8 m: whatever the reference accepts, the library accepts"""
    from diasss_amd import capi
    rows = [drifted[0], drifted[1] + np.array([0, 0, 0, further, 0, 0])]
    p = _grid(orc, data, [0, 1], drifted, 0.1, 0)
    pairs = [(0, 1), (1, 0)]
    rpy, off = _traj(rows)
    segs = ctx.mosaic_register_segments([0, 1], p, pairs, 80, reg=_reg(), rpy6=rpy, ping_off=off)
    edges, src = ctx.mosaic_register_edges([0, 1], p, pairs, segs, rpy6=rpy, ping_off=off)
    ref01 = _ref_pair(orc, data, [0, 1], rows, p, (0, 1), 80); ref10 = _ref_pair(orc, data, [0, 1], rows, p, (1, 0), 80)
    e01, s01 = E.edges(orc, ref01, p, rows[0], int(off[0]), rows[1], int(off[1]))
    e10, s10 = E.edges(orc, ref10, p, rows[1], int(off[1]), rows[0], int(off[0]))
    print("further %g: %d + %d of %d + %d rows accepted, leads %s" % (further, len(e01), len(e10), len(ref01), len(ref10), ["%.3g" % e["lead"] for e in e01 + e10]))
    assert all(e["lead"] > 1e-6 for e in e01 + e10)
    _same_edges(edges, src, e01 + e10, s01 + [len(ref01) + k for k in s10])
    if further == 0.0:
        assert s01 == list(range(8)) and all(e["a"] < e["b"] for e in e01 + e10) and all(int(off[0]) <= e["a"] < int(off[0]) + N for e in e01 + e10)
        with pytest.raises(capi.DsssError) as ei:
            ctx.mosaic_register_edges([0, 1], p, pairs, segs, rpy6=rpy, ping_off=off, cap=len(edges) - 1)
        assert ei.value.code == E_CAPACITY
        strict = capi.RegEdgeParams(2.0, 1.0, 10.0, 1.0)                                  # no ZNCC reaches 2: nothing is accepted
        assert len(ctx.mosaic_register_edges([0, 1], p, pairs, segs, edge_params=strict, rpy6=rpy, ping_off=off)[0]) == 0


def test_edges_under_the_frames_own_poses(ctx, orc, data):
    """rpy6 = NULL: the dead-reckoning pose6 of the frames; ping_off = NULL: the frames of ids one behind the other"""
    rows = [data[1]["pose"], data[0]["pose"]]
    p = _grid(orc, data, [1, 0], rows, 0.1, 0)
    segs = ctx.mosaic_register_segments([1, 0], p, [(0, 1)], 160, reg=_reg())
    edges, src = ctx.mosaic_register_edges([1, 0], p, [(0, 1)], segs)
    ref = _ref_pair(orc, data, [1, 0], rows, p, (0, 1), 160)
    es, ss = E.edges(orc, ref, p, rows[1], N, rows[0], 0)               # ids = [1, 0]: frame 1 has the pings 0 .. N - 1, frame 0 the next N
    assert len(es) >= 2 and all(e["lead"] > 1e-6 for e in es)
    _same_edges(edges, src, es, ss)
    assert all(e["a"] < N <= e["b"] for e in es)                        # b's ping (frame 1) comes first: the reversed edge


# ---------------------------------------------------------------- 5. end to end on the device
def test_segments_edges_solve_register_again(ctx, orc, data, drifted):
    """The thresholds are those tests/test_register_edges_cpu.py::test_preconditions_of_the_gpu_tests holds the reference to."""
    p = _grid(orc, data, [0, 1], drifted, 0.1, 0)
    dr = np.ascontiguousarray(np.concatenate(drifted)); off = np.array([0, N], np.int32)
    before = ctx.mosaic_register_segments([0, 1], p, [(0, 1)], 80, reg=_reg(), rpy6=dr, ping_off=off)
    edges, src = ctx.mosaic_register_edges([0, 1], p, [(0, 1)], before, rpy6=dr, ping_off=off)
    assert len(before) == 8 and src.tolist() == list(range(8))
    poses, stats = ctx.posegraph_solve_edges(dr, edges)
    o_poses, o_stats = orc.pg_solve(dr, edges)
    err = float(np.abs(poses - o_poses).max())
    print("max |pose - oracle| %.3g, LM iterations %d (oracle %d)" % (err, int(stats[0]), int(o_stats[0])))
    assert err < 1e-6
    solved = np.ascontiguousarray(E.rows_of_poses12(poses))
    after = ctx.mosaic_register_segments([0, 1], p, [(0, 1)], 80, reg=_reg(), rpy6=solved, ping_off=off)
    off0 = float(np.median(np.hypot(before["r"]["off_x"], before["r"]["off_y"]))); off1 = float(np.median(np.hypot(after["r"]["off_x"], after["r"]["off_y"])))
    z0 = float(np.median(before["r"]["zncc0"])); z1 = float(np.median(after["r"]["zncc0"]))
    print("median |offset| %.3f -> %.3f m, median zncc0 %.3f -> %.3f" % (off0, off1, z0, z1))
    assert off0 >= 0.2 and off1 <= 0.05 and z1 - z0 >= 0.5


# ---------------------------------------------------------------- 6. rules
def test_rules(ctx, orc, data, drifted):
    from diasss_amd import capi
    rows = [drifted[0], drifted[1], data[2]["true"]]
    p = _grid(orc, data, [0, 1, 2], rows, 0.5, 1)
    pairs = [(0, 1), (1, 0), (0, 2)]
    good = _run(ctx, [0, 1, 2], rows, p, pairs, 80)
    nseg = 8 + 8 + 7
    assert len(good[0]) == nseg and good[1].any()
    rpy, off = _traj(rows)

    def call(prs=pairs, seg_pings=80, ids=(0, 1, 2), **kw):
        return ctx.mosaic_register_segments(list(ids), p, prs, seg_pings, reg=_reg(), rpy6=rpy, ping_off=off, **kw)

    for code, fn in ((E_ARG, lambda: call(seg_pings=0)), (E_ARG, lambda: call(seg_pings=-5)), (E_CAPACITY, lambda: call(cap=nseg - 1)),
                     (E_CAPACITY, lambda: call(cap=0)), (E_ARG, lambda: call(prs=[(0, 0)])), (E_ARG, lambda: call(prs=[(0, 3)])),
                     (E_STATE, lambda: ctx.mosaic_register_segments([0, 3], p, [(0, 3)], 80, reg=_reg()))):          # frame 3 is not extracted
        with pytest.raises(capi.DsssError) as ei:
            fn()
        assert ei.value.code == code
    # the count comes back with the refusal
    ids = np.array([0, 1, 2], np.int32); pa = np.array([0, 1, 0], np.int32); pb = np.array([1, 0, 2], np.int32)
    one = np.zeros(1, capi.REGSEG_DTYPE); n = C.c_int(-1)
    rc = ctx.L.dsss_mosaic_register_segments(ctx.h, capi._ptr(ids), 3, capi._ptr(rpy), capi._ptr(off), C.byref(p), capi._ptr(pa), capi._ptr(pb), 3, 80,
                                             C.byref(_reg()), capi._ptr(one), 1, C.byref(n), None)
    assert rc == E_CAPACITY and n.value == nseg and not one.tobytes().strip(b"\0")
    empty = call(prs=[])
    assert len(empty) == 0
    again = _run(ctx, [0, 1, 2], rows, p, pairs, 80)                    # after the refusals, and twice: identical bytes
    assert again[0].tobytes() == good[0].tobytes() and again[1].tobytes() == good[1].tobytes()
    exact = _run(ctx, [0, 1, 2], rows, p, pairs, 80, cap=nseg)
    assert exact[0].tobytes() == good[0].tobytes()
    # permuting the pairs permutes the rows and nothing else (the pair index names the new place)
    perm = [2, 0, 1]
    q = _run(ctx, [0, 1, 2], rows, p, [pairs[k] for k in perm], 80)
    first = {k: int(np.flatnonzero(good[0]["pair"] == k)[0]) for k in range(3)}
    j = 0
    for new, k in enumerate(perm):
        cnt = int((good[0]["pair"] == k).sum())
        for s in range(cnt):
            g, d = good[0][first[k] + s], q[0][j + s]
            assert int(d["pair"]) == new and all(d[f].tobytes() == g[f].tobytes() for f in ("seg", "p0", "p1", "r", "sx", "sy"))
            assert q[1][j + s].tobytes() == good[1][first[k] + s].tobytes()
        j += cnt
    assert j == nseg
    # the frames in another order, one pair alone: the same rows
    r = _run(ctx, [2, 1, 0], rows[::-1], p, pairs, 80)
    assert r[0].tobytes() == good[0].tobytes() and r[1].tobytes() == good[1].tobytes()
    alone = _run(ctx, [0, 1, 2], rows, p, [pairs[1]], 80)
    assert alone[1].tobytes() == good[1][8:16].tobytes() and np.ascontiguousarray(alone[0]["r"]).tobytes() == np.ascontiguousarray(good[0]["r"][8:16]).tobytes()


def test_more_than_one_rank_is_a_state_error():
    from diasss_amd import capi
    c = capi.Context(max_frames=2)
    try:
        c.comm_init_callback(0, 2, lambda op, arr: None)
        p = capi.MosaicParams(0.0, 0.0, 0.1, 10, 10, 0, 0)
        with pytest.raises(capi.DsssError) as ei:
            c.mosaic_register_segments([0, 1], p, [(0, 1)], 80)
        assert ei.value.code == E_STATE and "rank" in str(ei.value)
        with pytest.raises(capi.DsssError) as ei:
            c.mosaic_register_edges([0, 1], p, [(0, 1)], np.zeros(1, capi.REGSEG_DTYPE))
        assert ei.value.code == E_STATE and "rank" in str(ei.value)
    finally:
        c.close()

"""GPU parity of the dense loop closures with a yaw fan: dsss_mosaic_register_segments_yaw (the six sums per shift of every (segment,
angle), every row's record, angle, flags, theta, theta_hat and centroid sums equal to the numpy reference of tests/register_yaw_ref.py
bit for bit), dsss_mosaic_register_edges_yaw (the reference's edge set) and both with the pose-graph solve end to end.

Nothing expected comes from the code under test: the rotation is the reference's (the oracle's orc_sincos and numpy arithmetic), geo
coordinates are the oracle's geo_img on the rotated rows, grey levels the oracle's normalised image, the mask the oracle's filter mask,
poses the oracle's Rodrigues construction.  Frames as in tests/test_gpu_register_segments.py: 0 and 1 are the two legs of
synth.Survey(2, 640, 400, seed=7), 2 is the 500 x 700 geometry of test_gpu_mosaic.py, 3 is set and never extracted.  The turned
survey is the one tests/test_register_yaw_cpu.py proves the preconditions for: true rows, the segments of leg 1 turned and moved."""
import ctypes as C
import numpy as np
import pytest

from tests import mosaic_register_ref as R
from tests import register_edges_ref as E
from tests import register_yaw_ref as Y
from tests.pg_report_ref import residual_bound
from tests.register_yaw_ref import CELL, FANS, SEG, SHIFT

pytestmark = pytest.mark.gpu

E_ARG, E_STATE, E_CAPACITY = -2, -4, -5
N, M = 640, 400
N2, M2 = 500, 700
RADIUS, MIN_CELLS = 8, 256
STEP = 0.01


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
def turned(orc, data):
    """the rows of the turned survey of fan one_step_up: true rows, every 80 pings of leg 1 turned by -0.01 rad and moved by (2, -1) cells"""
    nyaw, step, m = FANS["one_step_up"]
    assert step == STEP
    return [data[0]["true"], Y.rotated_survey(orc, data[1]["true"], SEG, m, step, SHIFT, CELL)]


def _traj(rows):
    """rows of the listed frames packed with unrelated rows in front -> (rpy6, ping_off)"""
    parts, off, n = [], [], 0
    for k, r in enumerate(rows):
        parts.append(np.full((k + 2, 6), 7.0e5)); n += k + 2
        off.append(n); parts.append(r); n += len(r)
    return np.ascontiguousarray(np.concatenate(parts)), np.array(off, np.int32)


def _grid(orc, data, frames, rows, cell, use_mask=0):
    from diasss_amd import capi
    g = [orc.geo_img(np.ascontiguousarray(r), data[f]["gr"], data[f]["M"]) for f, r in zip(frames, rows)]
    gx = np.concatenate([a[0].ravel() for a in g]); gy = np.concatenate([a[1].ravel() for a in g])
    ok = np.isfinite(gx) & np.isfinite(gy)
    p = capi.mosaic_grid((gx[ok].min(), gx[ok].max(), gy[ok].min(), gy[ok].max()), cell)
    p.use_mask = use_mask
    return p


def _reg(radius=RADIUS, min_cells=MIN_CELLS):
    from diasss_amd import capi
    return capi.RegParams(radius, min_cells)


def _fan(nyaw, step=STEP):
    from diasss_amd import capi
    return capi.RegYawParams(nyaw, 0, step)


def _ref_pair(orc, data, frames, rows, p, pair, seg_pings, nyaw, step=STEP, radius=RADIUS, min_cells=MIN_CELLS):
    """the reference's rows of one pair: frame pair[1] in segments under the fan against the whole of frame pair[0]"""
    a, b = pair
    ra, rb = rows[frames.index(a)], rows[frames.index(b)]
    ga = orc.geo_img(np.ascontiguousarray(ra), data[a]["gr"], data[a]["M"])
    la = R.mean_layer(ga[0], ga[1], data[a]["norm"], data[a]["mask"], p, p.use_mask)
    return Y.register_segments_yaw(orc, la, rb, data[b]["gr"], data[b]["M"], data[b]["norm"], data[b]["mask"], p, seg_pings, radius, min_cells, nyaw, step)


def _run(ctx, frames, rows, p, pairs, seg_pings, nyaw, step=STEP, radius=RADIUS, min_cells=MIN_CELLS, **kw):
    rpy, off = _traj(rows)
    return ctx.mosaic_register_segments_yaw(frames, p, pairs, seg_pings, yaw=_fan(nyaw, step), reg=_reg(radius, min_cells), rpy6=rpy, ping_off=off,
                                            want_sums=True, **kw)


def _bits(x):
    return np.float64(x).tobytes()


def _same_rows(dev, sums, k0, pair_index, ref):
    """rows k0 .. of the device against the reference's rows of one pair; returns the next row"""
    for s, rr in enumerate(ref):
        d = dev[k0 + s]
        assert (int(d["s"]["pair"]), int(d["s"]["seg"]), int(d["s"]["p0"]), int(d["s"]["p1"])) == (pair_index, rr["seg"], rr["p0"], rr["p1"])
        bad = np.argwhere(sums[k0 + s].astype(np.int64) != rr["sums"])
        assert len(bad) == 0, "pair %d segment %d: %d sums differ, first at [k, dy, dx, q] = %s: %d, reference %d" % (
            pair_index, s, len(bad), bad[0].tolist(), sums[k0 + s][tuple(bad[0])], rr["sums"][tuple(bad[0])])
        assert (int(d["k"]), int(d["yaw_on_border"])) == (rr["k"], rr["yaw_on_border"]), "pair %d segment %d: angle %d, reference %d" % (pair_index, s, d["k"], rr["k"])
        assert R.same_result(d["s"]["r"], rr["r"]), "pair %d segment %d: result %s, reference %s" % (pair_index, s, d["s"]["r"], rr["r"])
        for name in ("theta", "theta_hat", "zncc_k0"):
            assert _bits(d[name]) == _bits(rr[name]), "pair %d segment %d: %s %r, reference %r" % (pair_index, s, name, float(d[name]), rr[name])
        assert (int(d["s"]["sx"]), int(d["s"]["sy"])) == (rr["sx"], rr["sy"]), "pair %d segment %d: centroid sums" % (pair_index, s)
    return k0 + len(ref)


def _equal(ctx, orc, data, frames, rows, p, pairs, seg_pings, nyaw, step=STEP, radius=RADIUS, min_cells=MIN_CELLS):
    """device rows and sums of the pairs against the reference; returns (device rows, the reference's rows per pair)"""
    dev, sums = _run(ctx, frames, rows, p, pairs, seg_pings, nyaw, step, radius, min_cells)
    refs = [_ref_pair(orc, data, frames, rows, p, pr, seg_pings, nyaw, step, radius, min_cells) for pr in pairs]
    assert len(dev) == sum(len(r) for r in refs) == len(sums) and sums.shape[1] == nyaw
    k = 0
    for i, ref in enumerate(refs):
        k = _same_rows(dev, sums, k, i, ref)
    return dev, refs


# ---------------------------------------------------------------- 1. exact sums and records
@pytest.mark.parametrize("nyaw,radius,use_mask,seg_pings,order", [(3, 6, 1, 97, (0, 1)), (5, 8, 0, 97, (1, 0)), (5, 6, 0, 80, (0, 1)), (3, 8, 1, 80, (1, 0))])
def test_exact_sums_and_records(ctx, orc, data, turned, nyaw, radius, use_mask, seg_pings, order):
    p = _grid(orc, data, [0, 1], turned, CELL, use_mask)
    dev, (ref,) = _equal(ctx, orc, data, [0, 1], turned, p, [order], seg_pings, nyaw, radius=radius)
    assert len(ref) == (8 if seg_pings == 80 else 7) and ref[-1]["p1"] - ref[-1]["p0"] == (80 if seg_pings == 80 else 58)
    usable = [r for r in ref if r["r"]["zncc"] > -2.0]
    print("fan %d radius %d mask %d pair %s seg %d: %d rows, %d with a peak, k %s, theta_hat %s" % (
        nyaw, radius, use_mask, order, seg_pings, len(ref), len(usable), [r["k"] for r in ref], ["%.5f" % r["theta_hat"] for r in ref]))
    # the comparison is not of zeros, and the angles are not all the middle one
    assert all(r["sums"][k].any() for r in usable for k in range(nyaw)) and all(r["sx"] > 0 and r["sy"] > 0 for r in usable)
    assert len(usable) >= (3 if use_mask else len(ref) - 1) and any(r["k"] != (nyaw - 1) // 2 for r in usable)      # (the mask leaves few cells)
    assert all((r["sums"][0] != r["sums"][nyaw - 1]).any() for r in usable)
    if order == (0, 1) and seg_pings == 80 and nyaw == 5 and not use_mask:  # the segments as they were turned: the angle that undoes it
        assert all(r["k"] == 3 and r["yaw_on_border"] == 0 for r in usable)


# ---------------------------------------------------------------- 2. one angle is the existing registration
@pytest.mark.parametrize("seg_pings", [97, N])
def test_one_angle_is_the_existing_call(ctx, orc, data, turned, seg_pings):
    p = _grid(orc, data, [0, 1], turned, CELL, 1)
    rpy, off = _traj(turned)
    pairs = [(0, 1), (1, 0)]
    old, osums = ctx.mosaic_register_segments([0, 1], p, pairs, seg_pings, reg=_reg(), rpy6=rpy, ping_off=off, want_sums=True)
    for yaw in (_fan(1), _fan(1, 0.3), None):
        new, nsums = ctx.mosaic_register_segments_yaw([0, 1], p, pairs, seg_pings, yaw=yaw, reg=_reg(), rpy6=rpy, ping_off=off, want_sums=True)
        assert len(new) == len(old) > 0 and osums.any()
        assert np.ascontiguousarray(new["s"]).tobytes() == old.tobytes() and nsums.shape[1] == 1 and nsums[:, 0].tobytes() == osums.tobytes()
        assert not new["k"].any() and not new["yaw_on_border"].any() and not new["theta"].any() and not new["theta_hat"].any()
        assert new["zncc_k0"].tobytes() == np.ascontiguousarray(old["r"]["zncc"]).tobytes()
    # and the unrotated angle of a wider fan is that table too
    fan, fsums = ctx.mosaic_register_segments_yaw([0, 1], p, pairs, seg_pings, yaw=_fan(3), reg=_reg(), rpy6=rpy, ping_off=off, want_sums=True)
    assert fsums[:, 1].tobytes() == osums.tobytes() and fan["zncc_k0"].tobytes() == np.ascontiguousarray(old["r"]["zncc"]).tobytes()


def test_rotate_rows_is_the_references(orc, data, turned):
    from diasss_amd import capi
    rows = turned[1]
    for theta in (0.0, 0.01, -0.02, 0.3):
        for p0, p1 in ((0, N), (97, 194), (582, N), (5, 6)):
            assert capi.register_rotate_rows(rows, p0, p1, theta).tobytes() == Y.rotate_rows(orc, rows, p0, p1, theta).tobytes()
    assert capi.register_rotate_rows(rows, 97, 194, 0.0).tobytes() == rows[97:194].tobytes()


# ---------------------------------------------------------------- 3. shapes where the new kernel can go wrong
def test_grid_cropped_to_the_middle_third(ctx, orc, data, turned):
    """segments turned wholly off the grid (no window, zero sums under every angle) next to segments that straddle its edge"""
    from diasss_amd import capi
    full = _grid(orc, data, [0, 1], turned, CELL, 0)
    q = capi.MosaicParams(full.x0 + (full.W // 3) * full.cell, full.y0 + (full.H // 3) * full.cell, full.cell, full.W // 3, full.H // 3, 0, 0)
    dev, refs = _equal(ctx, orc, data, [0, 1], turned, q, [(0, 1), (1, 0)], 80, 3)
    for ref in refs:
        n0 = [r["r"]["n0"] for r in ref]
        empty = [r for r in ref if not r["sums"].any()]
        print("n0 per segment %s" % n0)
        assert len(empty) >= 2 and max(n0) > 1000 and len(empty) < len(ref)
        assert all(r["r"]["n"] == 0 and r["sx"] == 0 and r["sy"] == 0 and r["r"]["zncc"] == -2.0 and (r["k"], r["yaw_on_border"], r["theta_hat"]) == (1, 0, 0.0) for r in empty)


def test_a_wide_fan_of_short_segments(ctx, orc, data, turned):
    """seg_pings 7 and a step of 0.2 rad: windows a few cells wide that turn far; only the first ten segments (70 pings) of frame 0
    are on the grid"""
    rows0 = turned[0].copy(); rows0[70:, 3] += 1.0e5
    rows = [rows0, turned[1]]
    p = _grid(orc, data, [0, 1], turned, CELL, 0)
    dev, (ref,) = _equal(ctx, orc, data, [0, 1], rows, p, [(1, 0)], 7, 3, step=0.2, min_cells=64)
    assert len(ref) == 92 and ref[-1]["p1"] == N and ref[-1]["p1"] - ref[-1]["p0"] == 3
    assert all(not r["sums"].any() for r in ref[10:]) and all(r["sums"][1].any() for r in ref[:10])
    print("k of the ten segments %s, zncc %s" % ([r["k"] for r in ref[:10]], ["%.3f" % r["r"]["zncc"] for r in ref[:10]]))
    assert sum(r["r"]["zncc"] > -2.0 for r in ref[:10]) >= 5


def test_one_frame_as_b_of_two_pairs(ctx, orc, data, turned):
    """the fan layers of frame 1 are rendered once and read by both pairs"""
    rows = [turned[0], turned[1], data[2]["true"]]
    p = _grid(orc, data, [0, 1, 2], rows, 0.5, 1)
    dev, refs = _equal(ctx, orc, data, [0, 1, 2], rows, p, [(0, 1), (2, 1)], 160, 5, min_cells=64)
    assert len(refs[0]) == len(refs[1]) == 4 and any(r["r"]["n0"] > 100 for r in refs[0])
    print("n0: pair (0, 1) %s, pair (2, 1) %s" % ([r["r"]["n0"] for r in refs[0]], [r["r"]["n0"] for r in refs[1]]))


def test_a_pair_without_a_usable_angle(ctx, orc, data):
    """frame 2 moved 300 m aside, on a grid that holds both: every (segment, angle) has a window on the grid and none comes within the
    radius of a's: the row is the unrotated angle's record with k = mid"""
    far = [data[0]["true"], data[2]["true"] + np.array([0, 0, 0, 0, 300.0, 0])]
    wide = _grid(orc, data, [0, 2], far, 0.5, 0)
    assert wide.H > 600
    dev, sums = _run(ctx, [0, 2], far, wide, [(0, 2), (2, 0)], 128, 3)
    assert len(dev) == 4 + 5 and sums.shape[:2] == (9, 3) and not sums.any()
    zero = R.peak(np.zeros((2 * RADIUS + 1, 2 * RADIUS + 1, 6), np.int64), RADIUS, MIN_CELLS, wide.cell)
    for d in dev:
        assert R.same_result(d["s"]["r"], zero) and (int(d["k"]), int(d["yaw_on_border"]), float(d["theta"]), float(d["theta_hat"]), float(d["zncc_k0"])) == (1, 0, 0.0, 0.0, -2.0)
        assert int(d["s"]["sx"]) == 0 and int(d["s"]["sy"]) == 0
    assert dev["s"]["seg"].tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 4] and dev["s"]["pair"].tolist() == [0] * 4 + [1] * 5


# ---------------------------------------------------------------- 4. edges
def _same_edges(dev_edges, dev_src, ref_edges, ref_src):
    assert dev_src.tolist() == ref_src
    for d, r in zip(dev_edges, ref_edges):
        assert (int(d["a"]), int(d["b"])) == (r["a"], r["b"])
        assert (np.abs(d["rel"] - r["rel"]) <= residual_bound(r["rel"], 1.0)).all(), "rel: %s, reference %s" % (d["rel"], r["rel"])
        assert np.asarray(d["var"]).tobytes() == r["var"].tobytes(), "var: %s, reference %s" % (d["var"], r["var"])


@pytest.mark.parametrize("nyaw", [5, 3, 1])
def test_edges_are_the_references(ctx, orc, data, turned, nyaw):
    """nyaw 3: the angle that undoes the turn of leg 1 is the last of the fan, so pair (0, 1) gives no edge; nyaw 1: the existing edges"""
    from diasss_amd import capi
    p = _grid(orc, data, [0, 1], turned, CELL, 0)
    pairs = [(0, 1), (1, 0)]
    rpy, off = _traj(turned)
    ep = capi.RegEdgeYawParams(capi.reg_edge_params_default(), _fan(nyaw), 1.0)
    segs = ctx.mosaic_register_segments_yaw([0, 1], p, pairs, 80, yaw=_fan(nyaw), reg=_reg(), rpy6=rpy, ping_off=off)
    edges, src = ctx.mosaic_register_edges_yaw([0, 1], p, pairs, segs, edge_params=ep, rpy6=rpy, ping_off=off)
    ref01 = _ref_pair(orc, data, [0, 1], turned, p, (0, 1), 80, nyaw); ref10 = _ref_pair(orc, data, [0, 1], turned, p, (1, 0), 80, nyaw)
    e01, s01 = Y.edges_yaw(orc, ref01, p, turned[0], int(off[0]), turned[1], int(off[1]), nyaw, STEP)
    e10, s10 = Y.edges_yaw(orc, ref10, p, turned[1], int(off[1]), turned[0], int(off[0]), nyaw, STEP)
    print("fan %d: %d + %d of %d + %d rows accepted, leads %s" % (nyaw, len(e01), len(e10), len(ref01), len(ref10), ["%.3g" % e["lead"] for e in e01 + e10]))
    assert all(e["lead"] > 1e-6 for e in e01 + e10)
    _same_edges(edges, src, e01 + e10, s01 + [len(ref01) + k for k in s10])
    if nyaw == 5:
        assert s01 == list(range(8)) and all(e["var"][2] == STEP ** 2 for e in e01)
        with pytest.raises(capi.DsssError) as ei:
            ctx.mosaic_register_edges_yaw([0, 1], p, pairs, segs, edge_params=ep, rpy6=rpy, ping_off=off, cap=len(edges) - 1)
        assert ei.value.code == E_CAPACITY
        with pytest.raises(capi.DsssError) as ei:
            ctx.mosaic_register_edges_yaw([0, 1], p, pairs, segs, edge_params=capi.RegEdgeYawParams(capi.reg_edge_params_default(), _fan(4), 1.0), rpy6=rpy, ping_off=off)
        assert ei.value.code == E_ARG
    if nyaw == 3:
        assert s01 == [] and all(r["yaw_on_border"] == 1 for r in ref01)
    if nyaw == 1:
        old = ctx.mosaic_register_edges([0, 1], p, pairs, np.ascontiguousarray(segs["s"]), rpy6=rpy, ping_off=off)
        assert len(edges) > 0 and old[0].tobytes() == edges.tobytes() and old[1].tobytes() == src.tobytes()


# ---------------------------------------------------------------- 5. end to end on the device
def _wrap(a):
    return (a + np.pi) % (2 * np.pi) - np.pi


@pytest.mark.parametrize("name", sorted(FANS))
def test_fan_edges_turn_the_leg_back(ctx, orc, data, name):
    """The surveys are those tests/test_register_yaw_cpu.py::test_preconditions_of_the_gpu_tests holds the reference to.  Both solves
    start from the same rows; the translation-only edges are dsss_mosaic_register_edges on the rows of the same fan call."""
    from diasss_amd import capi
    nyaw, step, m = FANS[name]
    rows = [data[0]["true"], Y.rotated_survey(orc, data[1]["true"], SEG, m, step, SHIFT, CELL)]
    p = _grid(orc, data, [0, 1], rows, CELL, 0)
    dr = np.ascontiguousarray(np.concatenate(rows)); off = np.array([0, N], np.int32)
    segs = ctx.mosaic_register_segments_yaw([0, 1], p, [(0, 1)], SEG, yaw=_fan(nyaw, step), reg=_reg(), rpy6=dr, ping_off=off)
    assert len(segs) == 8 and (segs["k"] - (nyaw - 1) // 2 == m).all() and (segs["s"]["r"]["dx"] == SHIFT[0]).all() and (segs["s"]["r"]["dy"] == SHIFT[1]).all()
    assert (segs["s"]["r"]["zncc"] > segs["zncc_k0"]).all()
    ep = capi.RegEdgeYawParams(capi.reg_edge_params_default(), _fan(nyaw, step), 1.0)
    fan_edges, src = ctx.mosaic_register_edges_yaw([0, 1], p, [(0, 1)], segs, edge_params=ep, rpy6=dr, ping_off=off)
    plain_edges, psrc = ctx.mosaic_register_edges([0, 1], p, [(0, 1)], np.ascontiguousarray(segs["s"]), rpy6=dr, ping_off=off)
    assert src.tolist() == psrc.tolist() == list(range(8))
    true = np.concatenate([data[0]["true"], data[1]["true"]])
    err = {}
    for what, edges in (("translation", plain_edges), ("fan", fan_edges)):
        poses, stats = ctx.posegraph_solve_edges(dr, edges)
        err[what] = float(np.abs(_wrap(E.rows_of_poses12(poses)[N:, 2] - true[N:, 2])).mean())
    print("mean |yaw - true| of leg 1: before %.5f, translation-only edges %.5f, fan edges %.5f" % (abs(m) * step, err["translation"], err["fan"]))
    assert err["fan"] < err["translation"]


# ---------------------------------------------------------------- 6. rules
def test_rules(ctx, orc, data, turned):
    from diasss_amd import capi
    rows = [turned[0], turned[1], data[2]["true"]]
    p = _grid(orc, data, [0, 1, 2], rows, 0.5, 1)
    pairs = [(0, 1), (1, 0), (0, 2)]
    good = _run(ctx, [0, 1, 2], rows, p, pairs, 80, 3)
    nseg = 8 + 8 + 7
    assert len(good[0]) == nseg and good[1].any() and good[1].shape == (nseg, 3, 17, 17, 6)
    rpy, off = _traj(rows)

    def call(prs=pairs, seg_pings=80, ids=(0, 1, 2), yaw=_fan(3), **kw):
        return ctx.mosaic_register_segments_yaw(list(ids), p, prs, seg_pings, yaw=yaw, reg=_reg(), rpy6=rpy, ping_off=off, **kw)

    bad_fans = [_fan(0), _fan(2), _fan(4), _fan(19), _fan(-1), _fan(3, 0.0), _fan(3, -0.01), _fan(3, np.nan), _fan(3, np.inf)]
    for code, fn in [(E_ARG, lambda y=y: call(yaw=y)) for y in bad_fans] + [
            (E_ARG, lambda: call(seg_pings=0)), (E_ARG, lambda: call(seg_pings=-5)), (E_CAPACITY, lambda: call(cap=nseg - 1)),
            (E_CAPACITY, lambda: call(cap=0)), (E_ARG, lambda: call(prs=[(0, 0)])), (E_ARG, lambda: call(prs=[(0, 3)])),
            (E_ARG, lambda: ctx.mosaic_register_segments_yaw([0, 1, 2], p, pairs, 80, yaw=_fan(3), reg=_reg(17), rpy6=rpy, ping_off=off)),
            (E_STATE, lambda: ctx.mosaic_register_segments_yaw([0, 3], p, [(0, 3)], 80, yaw=_fan(3), reg=_reg()))]:          # frame 3 is not extracted
        with pytest.raises(capi.DsssError) as ei:
            fn()
        assert ei.value.code == code
    # a refusal comes before anything is written or launched: the output rows stay as they were, the count comes back
    ids = np.array([0, 1, 2], np.int32); pa = np.array([0, 1, 0], np.int32); pb = np.array([1, 0, 2], np.int32)
    one = np.zeros(1, capi.REGSEGYAW_DTYPE); n = C.c_int(-1); y = _fan(3)
    rc = ctx.L.dsss_mosaic_register_segments_yaw(ctx.h, capi._ptr(ids), 3, capi._ptr(rpy), capi._ptr(off), C.byref(p), capi._ptr(pa), capi._ptr(pb), 3, 80,
                                                 C.byref(_reg()), C.byref(y), capi._ptr(one), 1, C.byref(n), None)
    assert rc == E_CAPACITY and n.value == nseg and not one.tobytes().strip(b"\0")
    full = np.full(nseg, 0x55, np.uint8).repeat(capi.REGSEGYAW_DTYPE.itemsize).view(capi.REGSEGYAW_DTYPE); y = _fan(4)
    before = full.tobytes()
    rc = ctx.L.dsss_mosaic_register_segments_yaw(ctx.h, capi._ptr(ids), 3, capi._ptr(rpy), capi._ptr(off), C.byref(p), capi._ptr(pa), capi._ptr(pb), 3, 80,
                                                 C.byref(_reg()), C.byref(y), capi._ptr(full), nseg, C.byref(n), None)
    assert rc == E_ARG and full.tobytes() == before
    assert len(call(prs=[])) == 0
    again = _run(ctx, [0, 1, 2], rows, p, pairs, 80, 3)                 # after the refusals, and twice: identical bytes
    assert again[0].tobytes() == good[0].tobytes() and again[1].tobytes() == good[1].tobytes()
    exact = _run(ctx, [0, 1, 2], rows, p, pairs, 80, 3, cap=nseg)
    assert exact[0].tobytes() == good[0].tobytes()
    # the frames in another order, one pair alone: the same rows
    r = _run(ctx, [2, 1, 0], rows[::-1], p, pairs, 80, 3)
    assert r[0].tobytes() == good[0].tobytes() and r[1].tobytes() == good[1].tobytes()
    alone = _run(ctx, [0, 1, 2], rows, p, [pairs[1]], 80, 3)
    assert alone[1].tobytes() == good[1][8:16].tobytes()
    for f in ("k", "yaw_on_border", "theta", "theta_hat", "zncc_k0"):
        assert alone[0][f].tobytes() == good[0][f][8:16].tobytes()
    assert np.ascontiguousarray(alone[0]["s"]["r"]).tobytes() == np.ascontiguousarray(good[0]["s"]["r"][8:16]).tobytes()
    # without the sums the rows are the same
    quiet = ctx.mosaic_register_segments_yaw([0, 1, 2], p, pairs, 80, yaw=_fan(3), reg=_reg(), rpy6=rpy, ping_off=off)
    assert quiet.tobytes() == good[0].tobytes()


def test_more_than_one_rank_is_a_state_error():
    from diasss_amd import capi
    c = capi.Context(max_frames=2)
    try:
        c.comm_init_callback(0, 2, lambda op, arr: None)
        p = capi.MosaicParams(0.0, 0.0, 0.1, 10, 10, 0, 0)
        with pytest.raises(capi.DsssError) as ei:
            c.mosaic_register_segments_yaw([0, 1], p, [(0, 1)], 80, yaw=_fan(3))
        assert ei.value.code == E_STATE and "rank" in str(ei.value)
        with pytest.raises(capi.DsssError) as ei:
            c.mosaic_register_edges_yaw([0, 1], p, [(0, 1)], np.zeros(1, capi.REGSEGYAW_DTYPE))
        assert ei.value.code == E_STATE and "rank" in str(ei.value)
    finally:
        c.close()

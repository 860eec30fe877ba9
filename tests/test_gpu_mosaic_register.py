"""GPU parity of the dense overlap registration (dsss_mosaic_register): all six sums of every shift equal to the numpy reference of
tests/mosaic_register_ref.py, and the result record equal to the reference's bit for bit.

Nothing expected comes from the code under test: geo coordinates are the oracle's geo_img, grey levels the oracle's normalised image,
the mask the oracle's filter mask.  Frames 0 and 1 are the two legs of synth.Survey(2, 640, 400, seed=7), rendered from the true poses;
frame 2 is the 500 x 700 geometry of test_gpu_mosaic.py; frame 3 is set and never extracted.  Trajectories go in as rpy6 / ping_off."""
import ctypes as C
import numpy as np
import pytest

from tests import mosaic_register_ref as R

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -2, -4
N, M = 640, 400
N2, M2 = 500, 700


@pytest.fixture(scope="module")
def data(orc):
    from diasss_amd.synth import Survey
    from tests import helpers as H
    sv = Survey(2, N, M, seed=7)
    fr = []
    for f in range(2):
        raw = sv.frame(f).numpy().copy()
        pose, alt, gr = sv.inputs(f)
        fr.append(dict(N=N, M=M, raw=raw, pose=pose, alt=alt, gr=gr, true=np.ascontiguousarray(sv.poses_true[f]), norm=orc.normalize(raw), mask=orc.mask(raw)))
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


def _layers(orc, data, frames, rows, p):
    out = {}
    for f, r in zip(frames, rows):
        gx, gy = _geo(orc, data[f], r)
        out[f] = R.mean_layer(gx, gy, data[f]["norm"], data[f]["mask"], p, p.use_mask)
    return out


def _ref(lay, a, b, radius):
    return R.shift_sums(lay[a][0], lay[a][1], lay[b][0], lay[b][1], radius)


def _reg(radius, min_cells=256):
    from diasss_amd import capi
    return capi.RegParams(radius, min_cells)


def _run(ctx, frames, rows, p, pairs, radius, min_cells=256):
    rpy, off = _traj(rows)
    return ctx.mosaic_register(frames, p, pairs, reg=_reg(radius, min_cells), rpy6=rpy, ping_off=off, want_sums=True)


def _equal(ctx, orc, data, frames, rows, p, pairs, radius, min_cells=256):
    """device sums and results of the pairs against the reference; returns the reference's (sums, result) per pair"""
    lay = _layers(orc, data, frames, rows, p)
    res, sums = _run(ctx, frames, rows, p, pairs, radius, min_cells)
    out = []
    for k, (a, b) in enumerate(pairs):
        ref = _ref(lay, a, b, radius)
        assert sums[k].shape == ref.shape
        bad = np.argwhere(sums[k].astype(np.int64) != ref)
        assert len(bad) == 0, "pair (%d, %d): %d sums differ, first at [dy, dx, q] = %s: %d, reference %d" % (
            a, b, len(bad), bad[0].tolist(), sums[k][tuple(bad[0])], ref[tuple(bad[0])])
        rr = R.peak(ref, radius, min_cells, p.cell)
        assert R.same_result(res[k], rr), "pair (%d, %d): result %s, reference %s" % (a, b, res[k], rr)
        out.append((ref, rr))
    return out


# ---------------------------------------------------------------- 1. exact sums
@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
@pytest.mark.parametrize("use_mask", [0, 1])
@pytest.mark.parametrize("cell", [0.1, 0.5, 1.0])
def test_exact_sums(ctx, orc, data, cell, use_mask, order):
    rows = [data[0]["true"], data[1]["true"]]
    p = _grid(orc, data, [0, 1], rows, cell, use_mask)
    (ref, rr), = _equal(ctx, orc, data, [0, 1], rows, p, [order], 6)
    print("cell %g mask %d pair %s: grid %d x %d, n0 %d, peak (%d, %d) zncc %.4f" % (cell, use_mask, order, p.W, p.H, rr["n0"], rr["dx"], rr["dy"], rr["zncc"]))
    assert rr["n0"] > 0 and ref[:, :, 3].any()                      # the legs overlap on this grid: the comparison is not of zeros


# ---------------------------------------------------------------- 2. recovery
@pytest.mark.parametrize("shift", [(0, 0), (3, -2), (-4, 5)])
def test_recovers_a_known_offset(ctx, orc, data, shift):
    """Leg 1 moved by a whole number of 0.1 m cells: the peak is that shift exactly.  The preconditions hold on the reference alone.
    Measured with the reference on the CPU (oracle normalisation, no mask, radius 6): peak ZNCC 0.982 against 0.795 for the best other shift
    (a lead of 0.187) and 38 651 to 39 142 cells at the peak, for each of the three offsets; asserted are a lead of 0.1 and 10 000 cells."""
    moved = data[1]["true"] + np.array([0, 0, 0, 0.1 * shift[0], 0.1 * shift[1], 0])
    base = [data[0]["true"], data[1]["true"]]
    p = _grid(orc, data, [0, 1], base, 0.1, 0)
    (ref, rr), = _equal(ctx, orc, data, [0, 1], [data[0]["true"], moved], p, [(0, 1)], 6)
    z = R.scores(ref, 6, 256)
    others = max(z[j][i][0] for j in range(13) for i in range(13) if (i - 6, j - 6) != shift)
    print("shift %s: reference peak (%d, %d) zncc %.4f, best other %.4f, n %d" % (shift, rr["dx"], rr["dy"], rr["zncc"], others, rr["n"]))
    assert (rr["dx"], rr["dy"]) == shift
    assert rr["zncc"] - others > LEAD and rr["n"] >= 10000
    res = _run(ctx, [0, 1], [data[0]["true"], moved], p, [(0, 1)], 6)[0]
    assert (int(res[0]["dx"]), int(res[0]["dy"])) == shift and abs(res[0]["off_x"] - 0.1 * shift[0]) <= 0.05 and abs(res[0]["off_y"] - 0.1 * shift[1]) <= 0.05


LEAD = 0.1


# ---------------------------------------------------------------- 3. cross-check with the consistency map
def test_radius_zero_counts_the_cells_seen_twice(ctx, orc, data):
    rows = [data[0]["true"], data[1]["true"]]
    for cell, use_mask in ((0.1, 0), (0.5, 1)):
        p = _grid(orc, data, [0, 1], rows, cell, use_mask)
        rpy, off = _traj(rows)
        nfr = ctx.mosaic_consistency([0, 1], p, rpy6=rpy, ping_off=off)[0]
        res = ctx.mosaic_register([0, 1], p, [(0, 1), (1, 0)], reg=_reg(0, 1), rpy6=rpy, ping_off=off)
        twice = int((nfr == 2).sum())
        assert twice > 100 and int(res[0]["n0"]) == twice == int(res[1]["n0"]) == int(res[0]["n"])
        assert int(res[0]["on_border"]) == 1 and res[0]["zncc"] == res[1]["zncc"] == res[0]["zncc0"]


# ---------------------------------------------------------------- 4. windows and borders
def test_clipped_grid(ctx, orc, data):
    """a sub-rectangle that cuts through the overlap: b's halo leaves the grid on every side"""
    rows = [data[0]["true"], data[1]["true"]]
    full = _grid(orc, data, [0, 1], rows, 0.1, 0)
    lay = _layers(orc, data, [0, 1], rows, full)
    both = lay[0][1] & lay[1][1]
    ys, xs = np.nonzero(both)
    from diasss_amd import capi
    x_lo, x_hi = int(np.percentile(xs, 25)), int(np.percentile(xs, 75)); y_lo, y_hi = int(np.percentile(ys, 25)), int(np.percentile(ys, 75))
    q = capi.MosaicParams(full.x0 + x_lo * full.cell, full.y0 + y_lo * full.cell, full.cell, x_hi - x_lo + 1, y_hi - y_lo + 1, 0, 0)
    out = _equal(ctx, orc, data, [0, 1], rows, q, [(0, 1), (1, 0)], 6)
    assert out[0][1]["n0"] > 1000 and out[0][1]["n0"] < int(both.sum())


def test_windows_that_do_not_touch(ctx, orc, data):
    far = data[1]["true"] + np.array([0, 0, 0, 1000.0, 0, 0])
    rows = [data[0]["true"], far]
    near = _grid(orc, data, [0, 1], [data[0]["true"], data[1]["true"]], 0.1, 0)      # leg 1 is off this grid
    wide = _grid(orc, data, [0, 1], rows, 0.1, 0)                                     # both on the grid, a kilometre apart
    assert wide.W > 10000
    for p in (near, wide):
        res, sums = _run(ctx, [0, 1], rows, p, [(0, 1), (1, 0)], 6)
        assert not sums.any()
        for r in res:
            assert R.same_result(r, R.peak(np.zeros((13, 13, 6), np.int64), 6, 256, p.cell))
            assert r["zncc"] == -2.0 and r["dx"] == 0 and r["dy"] == 0 and r["n"] == 0


def test_search_square_larger_than_the_overlap(ctx, orc, data):
    rows = [data[0]["true"], data[1]["true"]]
    p = _grid(orc, data, [0, 1], rows, 1.0, 0)
    out = _equal(ctx, orc, data, [0, 1], rows, p, [(0, 1), (1, 0)], 16, min_cells=16)
    lay = _layers(orc, data, [0, 1], rows, p)
    ys, xs = np.nonzero(lay[0][1] & lay[1][1])
    assert 0 < ys.max() - ys.min() + 1 < 33, "the overlap should be narrower than the search square"
    assert out[0][0][:, :, 0].min() == 0 or out[0][0][0, 0, 0] < out[0][0][16, 16, 0]


def test_mixed_geometries(ctx, orc, data):
    rows = [data[0]["true"], data[2]["true"]]
    p = _grid(orc, data, [0, 2], rows, 0.1, 0)
    out = _equal(ctx, orc, data, [0, 2], rows, p, [(0, 2), (2, 0)], 6)
    assert out[0][1]["n0"] > 1000


def test_nan_row(ctx, orc, data):
    bad = data[0]["true"].copy(); bad[17, 3] = np.nan
    rows = [bad, data[1]["true"]]
    p = _grid(orc, data, [0, 1], [data[0]["true"], data[1]["true"]], 0.1, 0)
    (ref, rr), = _equal(ctx, orc, data, [0, 1], rows, p, [(0, 1)], 6)
    clean = _ref(_layers(orc, data, [0, 1], [data[0]["true"], data[1]["true"]], p), 0, 1, 6)
    assert rr["n0"] > 10000 and (ref != clean).any()


# ---------------------------------------------------------------- 5. invariance
def test_order_and_repeat(ctx, orc, data):
    rows = [data[0]["true"] + np.array([0, 0, 0, 0.17, -0.08, 0]), data[1]["true"], data[2]["true"]]
    p = _grid(orc, data, [0, 1, 2], rows, 0.1, 1)
    pairs = [(0, 1), (1, 0), (0, 2)]
    a = _run(ctx, [0, 1, 2], rows, p, pairs, 6)
    b = _run(ctx, [0, 1, 2], rows, p, pairs, 6)
    r = _run(ctx, [2, 1, 0], rows[::-1], p, pairs, 6)
    assert a[0].tobytes() == b[0].tobytes() == r[0].tobytes() and a[1].tobytes() == b[1].tobytes() == r[1].tobytes()
    assert a[1][0].any() and a[1][2].any()
    perm = [2, 0, 1]
    q = _run(ctx, [0, 1, 2], rows, p, [pairs[k] for k in perm], 6)
    for j, k in enumerate(perm):
        assert q[0][j].tobytes() == a[0][k].tobytes() and q[1][j].tobytes() == a[1][k].tobytes()
    for k, pr in enumerate(pairs):
        one = _run(ctx, [0, 1, 2], rows, p, [pr], 6)
        assert one[0][0].tobytes() == a[0][k].tobytes() and one[1][0].tobytes() == a[1][k].tobytes()


# ---------------------------------------------------------------- 6. errors
def test_errors_leave_the_context_usable(ctx, orc, data):
    from diasss_amd import capi
    rows = [data[0]["true"], data[1]["true"]]
    p = _grid(orc, data, [0, 1], rows, 0.5, 0)
    rpy, off = _traj(rows)
    good = ctx.mosaic_register([0, 1], p, [(0, 1)], reg=_reg(6), rpy6=rpy, ping_off=off, want_sums=True)
    assert good[1].any()

    def raw_call(npairs, out):
        ids = np.array([0, 1], np.int32); pa = np.array([0], np.int32); pb = np.array([1], np.int32)
        return ctx.L.dsss_mosaic_register(ctx.h, capi._ptr(ids), 2, capi._ptr(rpy), capi._ptr(off), C.byref(p), capi._ptr(pa), capi._ptr(pb), npairs,
                                          C.byref(_reg(6)), capi._ptr(out), None)

    calls = [
        (E_ARG, lambda: ctx.mosaic_register([0, 1], p, [(0, 2)], reg=_reg(6), rpy6=rpy, ping_off=off)),              # a pair member not in ids
        (E_ARG, lambda: ctx.mosaic_register([0, 1], p, [(0, 1), (1, 7)], reg=_reg(6), rpy6=rpy, ping_off=off)),
        (E_ARG, lambda: ctx.mosaic_register([0, 1], p, [(0, 1), (-1, 0)], reg=_reg(6), rpy6=rpy, ping_off=off)),
        (E_ARG, lambda: ctx.mosaic_register([0, 1], p, [(1, 1)], reg=_reg(6), rpy6=rpy, ping_off=off)),              # a == b
        (E_ARG, lambda: ctx.mosaic_register([0, 1], p, [(0, 1)], reg=_reg(-1), rpy6=rpy, ping_off=off)),
        (E_ARG, lambda: ctx.mosaic_register([0, 1], p, [(0, 1)], reg=_reg(17), rpy6=rpy, ping_off=off)),
        (E_ARG, lambda: ctx.mosaic_register([0, 1], p, [(0, 1)], reg=_reg(6, 0), rpy6=rpy, ping_off=off)),
        (E_STATE, lambda: ctx.mosaic_register([0, 3], p, [(0, 3)], reg=_reg(6))),                                    # frame 3 is not extracted
    ]
    for code, call in calls:
        with pytest.raises(capi.DsssError) as ei:
            call()
        assert ei.value.code == code
    assert raw_call(-1, np.zeros(1, capi.REG_DTYPE)) == E_ARG
    assert raw_call(1, None) == E_ARG
    assert raw_call(0, None) == 0                                                                                     # no pairs: valid
    empty = ctx.mosaic_register([0, 1], p, [], reg=_reg(6), rpy6=rpy, ping_off=off)
    assert len(empty) == 0
    again = ctx.mosaic_register([0, 1], p, [(0, 1)], reg=_reg(6), rpy6=rpy, ping_off=off, want_sums=True)
    assert again[0].tobytes() == good[0].tobytes() and again[1].tobytes() == good[1].tobytes()
    dflt = ctx.mosaic_register([0, 1], p, [(0, 1)], rpy6=rpy, ping_off=off, want_sums=True)                           # reg=None: radius 8, 256 cells
    assert dflt[1].shape == (1, 17, 17, 6) and (dflt[1][0, 2:15, 2:15] == good[1][0]).all()


def test_more_than_one_rank_is_a_state_error():
    from diasss_amd import capi
    c = capi.Context(max_frames=2)
    try:
        c.comm_init_callback(0, 2, lambda op, arr: None)
        with pytest.raises(capi.DsssError) as ei:
            c.mosaic_register([0, 1], capi.MosaicParams(0.0, 0.0, 0.1, 10, 10, 0, 0), [(0, 1)])
        assert ei.value.code == E_STATE and "rank" in str(ei.value)
    finally:
        c.close()

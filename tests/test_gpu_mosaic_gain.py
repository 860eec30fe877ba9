"""GPU parity of the range-gain normalisation: dsss_mosaic_gain_stats exact against the reference at the shapes where
mosaic_gainstat_kernel (here at one band) takes another path, and every entry that bins samples (render, consistency, register,
segments, yaw fan, pyramid) under a table against its existing numpy reference fed the corrected grey levels, bit for bit.

Nothing expected comes from the code under test: grey levels and masks are the oracle's, the statistics, the table and the corrected
samples come from tests/mosaic_gain_ref.py, geo coordinates from the oracle's geo_img.  Frames 0 and 1 are the two legs of
synth.Survey(2, 640, 400, seed=7) with the sensor profile of tests/mosaic_gain_cases.py (tests/test_mosaic_gain_cpu.py proves the
precondition of the effect test on them), 2 is a 500 x 700 frame (another M), 3 is set and never extracted, 4 has 333 pings of 400."""
import numpy as np
import pytest

from tests import extract_shapes_ref as X
from tests import mosaic_gain_cases as K
from tests import mosaic_gain_ref as G
from tests import mosaic_register_ref as R
from tests import register_edges_ref as E
from tests import register_pyr_ref as P
from tests import register_yaw_ref as Y

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -2, -4
N, M = K.N, K.M
N2, M2 = 500, 700
N4 = 333


# ---------------------------------------------------------------- frames and context
@pytest.fixture(scope="module")
def data(orc):
    from tests import helpers as H
    case = K.effect_case(orc)
    sv = case["sv"]
    fr = []
    for f in range(2):
        pose, alt, gr = sv.inputs(f)
        L = case["legs"][f]
        fr.append(dict(N=N, M=M, raw=case["raws"][f], pose=np.ascontiguousarray(pose), alt=alt, gr=gr, true=np.ascontiguousarray(sv.poses_true[f]),
                       norm=L["norm"], mask=L["mask"]))
    pose, alt, gr = H.track(N2, M2, 1, seed=9)
    raw = np.random.default_rng(1).rayleigh(1.0, (N2, M2)) * 100.0
    fr.append(dict(N=N2, M=M2, raw=raw, pose=pose, alt=alt, gr=gr, true=np.ascontiguousarray(pose), norm=orc.normalize(raw), mask=orc.mask(raw)))
    fr.append(fr[0])
    pose, alt, gr = H.track(N4, M, 0, seed=5)
    raw = np.random.default_rng(4).rayleigh(1.0, (N4, M)) * 100.0
    fr.append(dict(N=N4, M=M, raw=raw, pose=pose, alt=alt, gr=gr, true=np.ascontiguousarray(pose), norm=orc.normalize(raw), mask=orc.mask(raw)))
    return fr


def _snapshot(c, data):
    """every entry that bins samples, on frames 0 and 1 under the dead-reckoning rows: layers, sums and rows as bytes"""
    from diasss_amd import capi
    p = capi.mosaic_grid(c.mosaic_bounds([0, 1]), 0.1)
    pairs = [(0, 1), (1, 0)]
    reg = capi.RegParams(4, 64)
    out = {}
    out["render"] = b"".join(a.tobytes() for a in c.mosaic_render([0, 1], p))
    nfr, s1, s2, score = c.mosaic_consistency([0, 1], p)
    out["consistency"] = nfr.tobytes() + s1.tobytes() + s2.tobytes() + np.float64(score).tobytes()
    out["register"] = b"".join(a.tobytes() for a in c.mosaic_register([0, 1], p, pairs, reg=reg, want_sums=True))
    out["segments"] = b"".join(a.tobytes() for a in c.mosaic_register_segments([0, 1], p, pairs, 97, reg=reg, want_sums=True))
    out["yaw"] = b"".join(a.tobytes() for a in c.mosaic_register_segments_yaw([0, 1], p, pairs, 97, yaw=capi.RegYawParams(3, 0, 0.01), reg=reg, want_sums=True))
    out["pyr"] = b"".join(a.tobytes() for a in c.mosaic_register_segments_pyr([0, 1], p, pairs, 97, pyr=capi.RegPyrParams(2, P.REFINE), reg=reg, want_sums=True))
    return out


@pytest.fixture(scope="module")
def ctx(data):
    from diasss_amd import capi
    c = capi.Context(max_frames=5)
    for i, L in enumerate(data):
        c.frame_set(i, L["raw"], L["N"], L["M"], L["pose"], L["alt"], L["gr"])
    c.extract_many([0, 1, 2, 4])
    assert c.mosaic_gain_get() is None
    c.before = _snapshot(c, data)                    # taken before any table was set in this context
    yield c
    c.close()


@pytest.fixture
def clean(ctx):
    """the context without a table, before and after the test"""
    ctx.mosaic_gain_set(None)
    yield ctx
    ctx.mosaic_gain_set(None)


def _traj(rows):
    """rows of the listed frames packed with unrelated rows in front -> (rpy6, ping_off)"""
    parts, off, n = [], [], 0
    for k, r in enumerate(rows):
        parts.append(np.full((k + 2, 6), 7.0e5)); n += k + 2
        off.append(n); parts.append(r); n += len(r)
    return np.ascontiguousarray(np.concatenate(parts)), np.array(off, np.int32)


def _geo(orc, L, rows):
    return orc.geo_img(np.ascontiguousarray(rows), L["gr"], L["M"])


def _grid(orc, data, frames, rows, cell, use_mask):
    from diasss_amd import capi
    g = [_geo(orc, data[f], r) for f, r in zip(frames, rows)]
    gx = np.concatenate([a[0].ravel() for a in g]); gy = np.concatenate([a[1].ravel() for a in g])
    p = capi.mosaic_grid((gx.min(), gx.max(), gy.min(), gy.max()), cell)
    p.use_mask = use_mask
    return p


def _same(dev, ref):
    return dev.shape == ref.shape and (dev.astype(np.int64) == ref).all()


def _real_table(orc):
    return np.array(K.effect_case(orc)["gain"], np.uint16)


def _built_table(orc):
    """the real table with columns of gain 0, columns that clamp (65535: everything but 0 -> 255; 1024: everything from 64 on) and
    columns of 256 put into it"""
    t = _real_table(orc).copy()
    t[::7] = 0; t[3::11] = 65535; t[5::13] = 1024; t[1::17] = 256; t[190:210] = 0
    return t


# ---------------------------------------------------------------- 1. the statistics, exact
@pytest.mark.parametrize("use_mask", [0, 1])
@pytest.mark.parametrize("ids", [(0, 1), (0, 4, 1), (4,), (1,)], ids=lambda v: "frames" + "".join(map(str, v)))
def test_stats_exact(clean, data, ids, use_mask):
    """M = 400: dword rows, two column chunks of 64 lanes (the second with 36 at work), four rows at a time, row blocks of 512 with a
    partial last one (640: a block and 128 rows, all in batches; 333: 80 rows a lane in batches and three or four one by one); frames of
    different N in one call; n = 1"""
    S, C = clean.mosaic_gain_stats(list(ids), use_mask)
    rS, rC = G.col_stats([(data[f]["norm"], data[f]["mask"]) for f in ids], use_mask)
    assert S.dtype == np.uint64 and C.dtype == np.uint64
    assert C.tolist() == rC, "counts differ"
    assert S.tolist() == rS, "sums differ"
    total = sum(data[f]["N"] for f in ids) * M
    if use_mask:
        assert 0.01 * total < sum(rC) < 0.99 * total                # the mask keeps some samples and rejects others (1.8 % of the speckle frame)
    else:
        assert rC == [total // M] * M


@pytest.mark.parametrize("shape", [(501, 402), (69, 86), (69, 1234), (69, 1236)], ids=lambda s: "%dx%d" % s)
def test_stats_shapes(orc, shape):
    """M % 4 == 2 (rows not dword-aligned, the byte path; N odd and no multiple of any row block), M < 256 (32 lanes a row, eight rows
    at a time), M > 1024 (five column chunks, the last one partly idle) on both paths; 69 pings are 17 rows a lane: two batches and one"""
    from diasss_amd import capi
    rows, cols = shape
    c = capi.Context(max_frames=2)
    try:
        if rows == 69:
            nf = [s[3] for s in X.WIDE_SHAPES if s[:2] == shape][0]
            raw, orb, ref = X.wide_case(orc, rows, cols, 1, nf)
            mp, op = X.device_params(c, X.SMALL_MASK, orb)
            c.set_params(mask=mp, orb=op)
            norm, mask = ref["norm"], ref["mask"]
        else:
            raw = np.random.default_rng(rows).rayleigh(1.0, shape) * 100.0
            norm, mask = orc.normalize(raw), orc.mask(raw)
        pose, alt, gr = X.dr_inputs(rows, cols)
        c.frame_set(0, raw, rows, cols, pose, alt, gr)
        c.extract(0)
        dn, dm = c.frame_norm(0, rows, cols)
        assert (dn == norm).all() and (dm == mask).all()
        for use_mask in (0, 1):
            S, C = c.mosaic_gain_stats([0], use_mask)
            rS, rC = G.col_stats([(norm, mask)], use_mask)
            assert len(S) == cols and C.tolist() == rC and S.tolist() == rS, "%d x %d mask %d" % (rows, cols, use_mask)
            if use_mask:
                assert 0 < sum(rC) < rows * cols
        # the table of these statistics through the library and back from the device
        g, T = capi.mosaic_gain_table(S, C, capi.GainParams(8, 2, 0, 0))
        assert (g.tolist(), T) == G.table(rS, rC, cols, 8, 2, 0)
        c.mosaic_gain_set(g)
        assert c.mosaic_gain_get().tolist() == g.tolist()
    finally:
        c.close()


# ---------------------------------------------------------------- 2. the layers under a table
@pytest.mark.parametrize("cell", [0.1, 1.7])
def test_layers_under_a_table(clean, orc, data, cell):
    """render, consistency and register under a constructed table against the references fed apply(norm, table); cell 1.7 puts
    thousands of samples of both frames into a cell (contended cells)"""
    from diasss_amd import capi
    tab = _built_table(orc)
    cor = [G.apply(data[f]["norm"], tab) for f in (0, 1)]
    kept = data[0]["mask"] != 0
    assert (cor[0][kept] == 255).mean() > 0.05 and (cor[0][kept] == 0).mean() > 0.1 and (cor[0] != data[0]["norm"]).mean() > 0.5
    rows = [data[0]["pose"], data[1]["pose"]]
    geo = [_geo(orc, data[f], rows[f]) for f in (0, 1)]
    clean.mosaic_gain_set(tab)
    assert clean.mosaic_gain_get().tolist() == tab.tolist()
    for use_mask in (1, 0):
        p = _grid(orc, data, [0, 1], rows, cell, use_mask)
        acc = [P.accumulators(geo[f][0], geo[f][1], cor[f], data[f]["mask"], p, use_mask) for f in (0, 1)]
        Cn, S = acc[0][0] + acc[1][0], acc[0][1] + acc[1][1]
        s, c, img = clean.mosaic_render([0, 1], p)
        assert _same(c, Cn), "cnt differs"
        assert _same(s, S), "sum differs"
        assert _same(img, P.layer(Cn, S)[0]), "img differs"
        assert Cn.max() > (1000 if cell == 1.7 else 2)
        frames = [(geo[f][0], geo[f][1], cor[f], data[f]["mask"]) for f in (0, 1)]
        ref = K.consistency(frames, p, use_mask)
        nfr, s1, s2, score = clean.mosaic_consistency([0, 1], p)
        assert _same(nfr, ref[0]) and _same(s1, ref[1]) and _same(s2, ref[2])
        assert ref[3] > 0 and abs(score - ref[3]) <= 1e-12 * ref[3]
        radius, min_cells = 4, (64 if cell == 0.1 else 16)
        lay = [P.layer(*a) for a in acc]
        res, sums = clean.mosaic_register([0, 1], p, [(0, 1), (1, 0)], reg=capi.RegParams(radius, min_cells), want_sums=True)
        for k, (a, b) in enumerate([(0, 1), (1, 0)]):
            rs = R.shift_sums(lay[a][0], lay[a][1], lay[b][0], lay[b][1], radius)
            assert (sums[k].astype(np.int64) == rs).all(), "pair %d: sums differ" % k
            assert R.same_result(res[k], R.peak(rs, radius, min_cells, p.cell)), "pair %d: result" % k
            assert rs[radius, radius, 0] > min_cells
    # and the layers without the table are another thing
    under = clean.mosaic_render([0, 1], p)[0]
    clean.mosaic_gain_set(None)
    assert (under != clean.mosaic_render([0, 1], p)[0]).any()


# ---------------------------------------------------------------- 3. switch-back
def test_switch_back(clean, orc, data):
    """a table of 256s, and no table after a real one, give what the context gave before any table was set, byte for byte"""
    assert _snapshot(clean, data) == clean.before                    # (the calls repeat themselves)
    clean.mosaic_gain_set(np.full(M, 256, np.uint16))
    unity = _snapshot(clean, data)
    for k in unity:
        assert unity[k] == clean.before[k], "%s differs under a table of 256s" % k
    clean.mosaic_gain_set(_real_table(orc))
    real = _snapshot(clean, data)
    for k in real:
        assert real[k] != clean.before[k], "%s does not see the table" % k
    clean.mosaic_gain_set(None)
    assert clean.mosaic_gain_get() is None
    after = _snapshot(clean, data)
    for k in after:
        assert after[k] == clean.before[k], "%s differs after the table was cleared" % k


# ---------------------------------------------------------------- 4. segments, yaw fan and pyramid under the real table
def _corrected(orc, data):
    tab = _real_table(orc)
    return tab, [G.apply(data[f]["norm"], tab) for f in (0, 1)]


def _same_seg(d, rr, pair_index, what):
    assert (int(d["pair"]), int(d["seg"]), int(d["p0"]), int(d["p1"])) == (pair_index, rr["seg"], rr["p0"], rr["p1"]), what
    assert R.same_result(d["r"], rr["r"]), "%s: result %s, reference %s" % (what, d["r"], rr["r"])
    assert (int(d["sx"]), int(d["sy"])) == (rr["sx"], rr["sy"]), "%s: centroid sums" % what


def test_segments_under_the_table(clean, orc, data):
    from diasss_amd import capi
    tab, cor = _corrected(orc, data)
    rows = [data[0]["pose"], E.drift(data[1]["pose"])]                   # the drifted survey of tests/test_gpu_register_segments.py
    p = _grid(orc, data, [0, 1], rows, 0.1, 1)
    ga, gb = _geo(orc, data[0], rows[0]), _geo(orc, data[1], rows[1])
    la = R.mean_layer(ga[0], ga[1], cor[0], data[0]["mask"], p, 1)
    ref = E.register_segments(la, gb[0], gb[1], cor[1], data[1]["mask"], p, 80, 8, 256)
    plain = E.register_segments(R.mean_layer(ga[0], ga[1], data[0]["norm"], data[0]["mask"], p, 1), gb[0], gb[1], data[1]["norm"], data[1]["mask"], p, 80, 8, 256)
    rpy, off = _traj(rows)
    clean.mosaic_gain_set(tab)
    dev, sums = clean.mosaic_register_segments([0, 1], p, [(0, 1)], 80, reg=capi.RegParams(8, 256), rpy6=rpy, ping_off=off, want_sums=True)
    assert len(dev) == len(ref) == 8
    for s, rr in enumerate(ref):
        assert (sums[s].astype(np.int64) == rr["sums"]).all(), "segment %d: sums differ" % s
        _same_seg(dev[s], rr, 0, "segment %d" % s)
    usable = [r for r in ref if r["r"]["zncc"] > -2.0]
    print("zncc under the table %s, without %s" % (["%.3f" % r["r"]["zncc"] for r in ref], ["%.3f" % r["r"]["zncc"] for r in plain]))
    assert len(usable) >= 4 and any((a["sums"] != b["sums"]).any() for a, b in zip(ref, plain))


def test_yaw_fan_under_the_table(clean, orc, data):
    from diasss_amd import capi
    tab, cor = _corrected(orc, data)
    nyaw, step, m = Y.FANS["one_step_up"]
    rows = [data[0]["true"], Y.rotated_survey(orc, data[1]["true"], Y.SEG, m, step, Y.SHIFT, Y.CELL)]          # the turned survey of tests/test_gpu_register_yaw.py
    p = _grid(orc, data, [0, 1], rows, Y.CELL, 1)
    ga = _geo(orc, data[0], rows[0])
    la = R.mean_layer(ga[0], ga[1], cor[0], data[0]["mask"], p, 1)
    ref = Y.register_segments_yaw(orc, la, rows[1], data[1]["gr"], M, cor[1], data[1]["mask"], p, 97, 6, 256, 3, step)
    rpy, off = _traj(rows)
    clean.mosaic_gain_set(tab)
    dev, sums = clean.mosaic_register_segments_yaw([0, 1], p, [(0, 1)], 97, yaw=capi.RegYawParams(3, 0, step), reg=capi.RegParams(6, 256), rpy6=rpy, ping_off=off,
                                                   want_sums=True)
    assert len(dev) == len(ref) == 7 and sums.shape[1] == 3
    for s, rr in enumerate(ref):
        d = dev[s]
        assert (sums[s].astype(np.int64) == rr["sums"]).all(), "segment %d: sums differ" % s
        assert (int(d["k"]), int(d["yaw_on_border"])) == (rr["k"], rr["yaw_on_border"])
        _same_seg(d["s"], rr, 0, "segment %d" % s)
        for name in ("theta", "theta_hat", "zncc_k0"):
            assert np.float64(d[name]).tobytes() == np.float64(rr[name]).tobytes(), "segment %d: %s" % (s, name)
    assert sum(r["r"]["zncc"] > -2.0 for r in ref) >= 3


def test_pyramid_under_the_table(clean, orc, data):
    from diasss_amd import capi
    tab, cor = _corrected(orc, data)
    rows = [data[0]["true"], data[1]["true"] + np.array([0, 0, 0, P.MOVE[0], P.MOVE[1], 0])]                   # the moved survey of tests/test_gpu_register_pyr.py
    g = [_geo(orc, data[f], rows[f]) for f in (0, 1)]
    gx = np.concatenate([a[0].ravel() for a in g]); gy = np.concatenate([a[1].ravel() for a in g])
    p = P.awkward_grid(lambda *v: capi.MosaicParams(*v, 0, 0), (gx.min(), gx.max(), gy.min(), gy.max()), P.CELL, g[1][0], g[1][1], P.SEG)
    p.use_mask = 1                                   # (the table was estimated over the samples the mask keeps)
    acc = P.accumulators(g[0][0], g[0][1], cor[0], data[0]["mask"], p, 1)
    ref = P.register_segments_pyr(acc, g[1][0], g[1][1], cor[1], data[1]["mask"], p, P.SEG, P.RADIUS, P.MIN_CELLS, 3, P.REFINE)
    rpy, off = _traj(rows)
    clean.mosaic_gain_set(tab)
    dev, sums = clean.mosaic_register_segments_pyr([0, 1], p, [(0, 1)], P.SEG, pyr=capi.RegPyrParams(3, P.REFINE), reg=capi.RegParams(P.RADIUS, P.MIN_CELLS),
                                                   rpy6=rpy, ping_off=off, want_sums=True)
    assert len(dev) == len(ref) == 8
    for s, rr in enumerate(ref):
        d = dev[s]
        assert (sums[s].astype(np.int64) == rr["sums"]).all(), "segment %d: sums differ" % s
        assert (int(d["level"]), int(d["border_mask"])) == (rr["level"], rr["border_mask"])
        assert d["lx"].tolist() == rr["lx"] and d["ly"].tolist() == rr["ly"] and np.asarray(d["lz"], np.float64).tobytes() == np.asarray(rr["lz"], np.float64).tobytes()
        _same_seg(d["s"], rr, 0, "segment %d" % s)
    # the comparison is not of empty rows: four segments walk all three levels down to the offset the leg was moved by (three without
    # the table), the outer ones, which the mask leaves few cells, stop on the way
    done = [r for r in ref if r["level"] == 0 and (r["r"]["dx"], r["r"]["dy"]) == P.MOVE_CELLS]
    assert len(done) >= 4 and any(r["level"] != 0 for r in ref)


# ---------------------------------------------------------------- 5. the effect
def test_effect_is_the_references(clean, orc, data):
    """Under the true poses, cell 0.1, mask on: the device's statistics, table, consistency score and ZNCC with and without the table are
    the reference's, so the inequalities tests/test_mosaic_gain_cpu.py::test_effect_precondition proves hold on the device: score
    21.914 -> 10.843, ZNCC at zero shift 0.7667 -> 0.9377."""
    from diasss_amd import capi
    case = K.effect_case(orc)
    q = case["p"]
    p = capi.MosaicParams(q.x0, q.y0, q.cell, q.W, q.H, 1, 0)
    g = capi.mosaic_grid(clean.mosaic_bounds([0, 1], *_traj([data[0]["true"], data[1]["true"]])), K.CELL)
    assert (g.x0, g.y0, g.W, g.H) == (p.x0, p.y0, p.W, p.H)
    S, C = clean.mosaic_gain_stats([0, 1], 1)
    assert S.tolist() == case["S"] and C.tolist() == case["C"]
    tab, T = capi.mosaic_gain_table(S, C, capi.GainParams(K.MIN_COUNT, K.SMOOTH, K.TARGET, 0))
    assert tab.tolist() == case["gain"] and T == case["T"] == 117
    rpy, off = _traj([data[0]["true"], data[1]["true"]])
    reg = capi.reg_params_default()
    for name, table, norms in (("without", None, None), ("with", tab, case["corrected"])):
        clean.mosaic_gain_set(table)
        frames = K.frames_of(case["legs"], norms)
        ref = K.consistency(frames, q, 1)
        nfr, s1, s2, score = clean.mosaic_consistency([0, 1], p, rpy6=rpy, ping_off=off)
        (ma, va), (mb, vb) = (R.mean_layer(f[0], f[1], f[2], f[3], q, 1) for f in frames)
        rs = R.shift_sums(ma, va, mb, vb, 1)
        res, sums = clean.mosaic_register([0, 1], p, [(0, 1)], reg=capi.RegParams(1, reg.min_cells), rpy6=rpy, ping_off=off, want_sums=True)
        print("%s the table: score %.3f (reference %.3f), zncc0 %.4f" % (name, score, ref[3], res[0]["zncc0"]))
        assert _same(nfr, ref[0]) and _same(s1, ref[1]) and _same(s2, ref[2]) and abs(score - ref[3]) <= 1e-12 * ref[3]
        assert (sums[0].astype(np.int64) == rs).all() and R.same_result(res[0], R.peak(rs, 1, reg.min_cells, p.cell))
        assert np.float64(res[0]["zncc0"]).tobytes() == np.float64(K.zncc0(frames, q, 1, reg.min_cells)).tobytes()


# ---------------------------------------------------------------- 6. errors
def _code(fn, *a, **kw):
    from diasss_amd import capi
    with pytest.raises(capi.DsssError) as e:
        fn(*a, **kw)
    return e.value.code


def test_errors_leave_context_and_table(clean, orc, data):
    from diasss_amd import capi
    tab = _real_table(orc)
    clean.mosaic_gain_set(tab)
    p = capi.mosaic_grid(clean.mosaic_bounds([0, 1]), 0.1)
    good = clean.mosaic_render([0, 1], p)[0].tobytes()
    S0, C0 = clean.mosaic_gain_stats([0, 1], 1)
    # statistics
    assert _code(clean.mosaic_gain_stats, [0, 2]) == E_ARG               # mixed M
    assert _code(clean.mosaic_gain_stats, [0, 0]) == E_ARG               # listed twice
    assert _code(clean.mosaic_gain_stats, [0, 7]) == E_ARG               # out of range
    assert _code(clean.mosaic_gain_stats, []) == E_ARG
    assert _code(clean.mosaic_gain_stats, [0, 3]) == E_STATE             # not extracted
    L = clean.L
    ids = np.array([0, 1], np.int32); buf = np.zeros(M, np.uint64)
    assert L.dsss_mosaic_gain_stats(clean.h, capi._ptr(ids), 2, 1, None, capi._ptr(buf)) == E_ARG
    assert L.dsss_mosaic_gain_stats(clean.h, capi._ptr(ids), 2, 1, capi._ptr(buf), None) == E_ARG
    # set / get
    assert _code(clean.mosaic_gain_set, tab[:1]) == E_ARG                # M < 2
    assert _code(clean.mosaic_gain_get, cap=M - 1) == E_ARG              # cap < M
    Mout = capi.C.c_int(-1)
    assert L.dsss_mosaic_gain_get(clean.h, None, 0, capi.C.byref(Mout)) == E_ARG and Mout.value == M      # the size is told all the same
    assert L.dsss_mosaic_gain_get(clean.h, capi._ptr(np.zeros(M, np.uint16)), M, None) == E_ARG
    assert clean.mosaic_gain_get(cap=M + 3).tolist() == tab.tolist()
    # a table of another M under every entry: refused before anything happens
    pairs = [(0, 2)]
    p2 = capi.mosaic_grid(clean.mosaic_bounds([0, 2]), 0.1)
    assert _code(clean.mosaic_render, [0, 2], p2) == E_ARG
    assert _code(clean.mosaic_consistency, [0, 2], p2) == E_ARG
    assert _code(clean.mosaic_register, [0, 2], p2, pairs) == E_ARG
    assert _code(clean.mosaic_register_segments, [0, 2], p2, pairs, 80) == E_ARG
    assert _code(clean.mosaic_register_segments_yaw, [0, 2], p2, pairs, 80, yaw=capi.RegYawParams(3, 0, 0.01)) == E_ARG
    assert _code(clean.mosaic_register_segments_pyr, [0, 2], p2, pairs, 80, pyr=capi.RegPyrParams(2, P.REFINE)) == E_ARG
    assert _code(clean.mosaic_render, [0, 3], p) == E_STATE              # the state rule comes first, as without a table
    # the context is usable, the table is the one that was set, and a valid call gives what it gave
    assert clean.mosaic_gain_get().tolist() == tab.tolist()
    assert clean.mosaic_render([0, 1], p)[0].tobytes() == good
    S1, C1 = clean.mosaic_gain_stats([0, 1], 1)
    assert S1.tolist() == S0.tolist() and C1.tolist() == C0.tolist()
    # the statistics are those of the uncorrected samples, table or not
    assert S0.tolist() == K.effect_case(orc)["S"]
    # frames of another M are fine again once the table is gone, and a table of their M serves them
    clean.mosaic_gain_set(None)
    clean.mosaic_render([0, 2], p2)
    clean.mosaic_gain_set(np.full(M2, 300, np.uint16))
    clean.mosaic_render([2], p2)
    assert _code(clean.mosaic_render, [0, 2], p2) == E_ARG
    assert _code(clean.mosaic_gain_set, tab[:1]) == E_ARG and clean.mosaic_gain_get().tolist() == [300] * M2

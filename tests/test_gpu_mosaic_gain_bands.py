"""GPU parity of the altitude-banded range gain, everything exact: dsss_mosaic_gain_stats_banded against the reference at the shapes
where mosaic_gainstat_kernel takes another path and under the altitude series that drive its band logic (and, on the same frames, the
one-band launch behind dsss_mosaic_gain_stats against mosaic_gain_ref.col_stats), dsss_frame_get_corrected on the same frames, and
every entry that bins samples (render, consistency, register, segments, yaw fan, pyramid, composite) under a banded table against
its existing numpy reference fed the grey levels of mosaic_gain_bands_ref.apply_banded.

Nothing expected comes from the code under test: grey levels and masks are the oracle's, the statistics, the table and the corrected
samples come from tests/mosaic_gain_bands_ref.py, geo coordinates from the oracle's geo_img.  Frames 0 and 1 are the two legs of the
effect survey of tests/mosaic_gain_bands_cases.py (tests/test_mosaic_gain_bands_cpu.py proves the precondition of the effect test on
them), 2 is a 500 x 700 frame (another M), 3 is set and never extracted.

dsss_frame_set copies the altitudes unread, so NaN, infinite and far out-of-range altitudes reach the device: the "wild" series runs
here as every other one."""
import numpy as np
import pytest

from tests import extract_shapes_ref as X
from tests import mosaic_composite_ref as CR
from tests import mosaic_gain_bands_cases as K
from tests import mosaic_gain_bands_ref as B
from tests import mosaic_gain_cases as KC
from tests import mosaic_gain_ref as G
from tests import mosaic_register_ref as R
from tests import register_edges_ref as E
from tests import register_pyr_ref as P
from tests import register_yaw_ref as Y

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -2, -4
N, M = K.N, K.M
N2, M2 = 500, 700
NB = K.BANDS[2]


# ---------------------------------------------------------------- 1. statistics and corrected waterfall at every shape and series
def _shape_frame(orc, c, shape):
    """raw, norm, mask of the shape's frame, and the context's parameters set for it"""
    rows, cols = shape
    if rows == 69:
        nf = [s[3] for s in X.WIDE_SHAPES if s[:2] == shape][0]
        raw, orb, ref = X.wide_case(orc, rows, cols, 1, nf)
        mp, op = X.device_params(c, X.SMALL_MASK, orb)
        c.set_params(mask=mp, orb=op)
        return raw, ref["norm"], ref["mask"]
    raw = np.random.default_rng(rows).rayleigh(1.0, shape) * 100.0
    return raw, orc.normalize(raw), orc.mask(raw)


def _check_stats(c, ids, frames, alts, what):
    for bands in (K.SHAPE_BANDS, K.SHAPE_BANDS[:2] + (1,)):
        for use_mask in (0, 1):
            S, C = c.mosaic_gain_stats(ids, use_mask, bands=bands)
            rS, rC = B.band_stats(frames, alts, bands, use_mask)
            assert S.dtype == np.uint64 and S.shape == C.shape == (bands[2], frames[0][0].shape[1])
            assert C.tolist() == rC, "%s bands %d mask %d: counts differ" % (what, bands[2], use_mask)
            assert S.tolist() == rS, "%s bands %d mask %d: sums differ" % (what, bands[2], use_mask)
            cS, cC = c.mosaic_gain_stats(ids, use_mask)
            assert S.sum(axis=0).tolist() == cS.tolist() and C.sum(axis=0).tolist() == cC.tolist()      # summed over the bands: the column entry
            gS, gC = G.col_stats(frames, use_mask)                                                     # ... which is the one kernel at one band: held to the reference itself
            assert cS.tolist() == gS and cC.tolist() == gC, "%s mask %d: the column entry differs from the reference" % (what, use_mask)


def _check_corrected(c, fid, norm, alt, what):
    cols = norm.shape[1]
    c.mosaic_gain_set(None)
    assert (c.frame_corrected(fid) == norm).all(), "%s: no table" % what
    tab = K.built_table(16, cols)
    c.mosaic_gain_set(tab, bands=K.SHAPE_BANDS)
    ref = B.apply_banded(norm, alt, tab, K.SHAPE_BANDS)
    dev = c.frame_corrected(fid)
    assert dev.dtype == np.uint8 and dev.shape == ref.shape and (dev == ref).all(), "%s: banded table" % what
    c.mosaic_gain_set(tab[3])
    assert (c.frame_corrected(fid) == G.apply(norm, tab[3])).all(), "%s: one band" % what
    c.mosaic_gain_set(None)
    return ref


@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: "%dx%d" % s)
def test_stats_and_corrected_shapes(orc, shape):
    """every shape x every altitude series x mask on and off x 16 bands and 1: the statistics exact, and the corrected waterfall under a
    table whose gains differ in every (band, column), under one of its rows as a column table, and under none"""
    from diasss_amd import capi
    rows, cols = shape
    c = capi.Context(max_frames=1)
    try:
        raw, norm, mask = _shape_frame(orc, c, shape)
        pose, _, gr = X.dr_inputs(rows, cols)
        for kind in K.SERIES:
            alt = K.series(kind, rows, K.SHAPE_BANDS)
            c.frame_set(0, raw, rows, cols, pose, alt, gr)
            c.extract(0)
            if kind == K.SERIES[0]:
                dn, dm = c.frame_norm(0, rows, cols)
                assert (dn == norm).all() and (dm == mask).all()
            what = "%d x %d %s" % (rows, cols, kind)
            _check_stats(c, [0], [(norm, mask)], [alt], what)
            ref = _check_corrected(c, 0, norm, alt, what)
            if kind in ("cycle", "edges"):
                bs = B.bands_of(K.SHAPE_BANDS, alt)
                assert set(bs.tolist()) == set(range(16)) and (ref != norm).any()
        assert 0 < int((mask != 0).sum()) < rows * cols
    finally:
        c.close()


def test_stats_mixed_frames_in_one_call(orc):
    """frames of 333 and 640 pings of 400 columns under different series in ONE call, in both orders, and each alone"""
    from diasss_amd import capi
    c = capi.Context(max_frames=2)
    try:
        fr, alts = [], []
        for i, (rows, kind) in enumerate(((333, "runs"), (640, "cycle"))):
            raw = np.random.default_rng(rows).rayleigh(1.0, (rows, 400)) * 100.0
            pose, _, gr = X.dr_inputs(rows, 400)
            alt = K.series(kind, rows, K.SHAPE_BANDS)
            c.frame_set(i, raw, rows, 400, pose, alt, gr)
            fr.append((orc.normalize(raw), orc.mask(raw))); alts.append(alt)
        c.extract_many([0, 1])
        _check_stats(c, [0, 1], fr, alts, "333 + 640")
        _check_stats(c, [1, 0], fr[::-1], alts[::-1], "640 + 333")
        _check_stats(c, [1], fr[1:], alts[1:], "640 alone")
    finally:
        c.close()


# ---------------------------------------------------------------- frames and context of the effect case
@pytest.fixture(scope="module")
def data(orc):
    from tests import helpers as H
    case = K.effect_case(orc)
    sv = case["sv"]
    fr = []
    for f in range(2):
        pose, _, gr = sv.inputs(f)
        L = case["legs"][f]
        fr.append(dict(N=N, M=M, raw=case["raws"][f], pose=np.ascontiguousarray(pose), alt=case["alts"][f], gr=gr, true=np.ascontiguousarray(sv.poses_true[f]),
                       norm=L["norm"], mask=L["mask"]))
    pose, alt, gr = H.track(N2, M2, 1, seed=9)
    raw = np.random.default_rng(1).rayleigh(1.0, (N2, M2)) * 100.0
    fr.append(dict(N=N2, M=M2, raw=raw, pose=pose, alt=alt, gr=gr, true=np.ascontiguousarray(pose), norm=orc.normalize(raw), mask=orc.mask(raw)))
    fr.append(fr[0])
    return fr


def _snapshot(c):
    """all seven entries that bin samples, on frames 0 and 1 under the dead-reckoning rows: layers, sums and rows as bytes"""
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
    lay, info = c.mosaic_composite([0, 1], p, fill_radius=2)
    out["composite"] = b"".join(lay[n].tobytes() for n in CR.LAYERS) + bytes(info)
    return out


@pytest.fixture(scope="module")
def ctx(data):
    from diasss_amd import capi
    c = capi.Context(max_frames=4)
    for i, L in enumerate(data):
        c.frame_set(i, L["raw"], L["N"], L["M"], L["pose"], L["alt"], L["gr"])
    c.extract_many([0, 1, 2])
    assert c.mosaic_gain_get() is None and c.mosaic_gain_get_banded() is None
    c.before = _snapshot(c)                          # taken before any table was set in this context
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


def _corrected(orc, data, tab=None):
    tab = _real_table(orc) if tab is None else tab
    return tab, [B.apply_banded(data[f]["norm"], data[f]["alt"], tab, K.BANDS) for f in (0, 1)]


# ---------------------------------------------------------------- 2. the layers under a banded table
@pytest.mark.parametrize("cell", [0.1, 1.7])
def test_layers_under_the_banded_table(clean, orc, data, cell):
    """render, consistency and register under the reference's banded table against the references fed apply_banded's grey levels; cell 1.7
    puts thousands of samples of both frames into a cell (contended cells)"""
    from diasss_amd import capi
    tab, cor = _corrected(orc, data)
    col_cor = K.effect_case(orc)["corrected_col"]
    assert all((cor[f] != col_cor[f]).mean() > 0.2 for f in (0, 1))          # (the banded table is not the column table in disguise)
    rows = [data[0]["pose"], data[1]["pose"]]
    geo = [_geo(orc, data[f], rows[f]) for f in (0, 1)]
    clean.mosaic_gain_set(tab, bands=K.BANDS)
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
        ref = KC.consistency(frames, p, use_mask)
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


@pytest.mark.parametrize("mode,R_", [(CR.NEAR, 0), (CR.FIRST, 2)])
def test_composite_under_the_banded_table(clean, orc, data, mode, R_):
    """img and the source layers: the winner's value is corrected with the band of the WINNING ping"""
    from diasss_amd import capi
    tab, cor = _corrected(orc, data, K.built_table(NB, M, seed=8))
    rows = [data[0]["true"], data[1]["true"]]
    rpy, off = _traj(rows)
    p = _grid(orc, data, [0, 1], rows, 0.13, 1)
    fr = []
    for f in (0, 1):
        gx, gy = _geo(orc, data[f], rows[f])
        fr.append(dict(id=f, gx=gx, gy=gy, norm=cor[f], mask=data[f]["mask"]))
    lay, counts, stats = CR.composite(fr, p, 1, mode, R_)
    clean.mosaic_gain_set(tab, bands=K.BANDS)
    dev, info = clean.mosaic_composite([1, 0], p, mode=mode, fill_radius=R_, rpy6=rpy[:, :], ping_off=off[::-1].copy())
    for name in CR.LAYERS:
        assert _same(dev[name], lay[name]), "%s differs" % name
    assert (info.direct, info.filled, info.empty) == counts and stats["contended"] > 100
    plain = CR.composite([dict(f, norm=data[f["id"]]["norm"]) for f in fr], p, 1, mode, R_)[0]
    held = lay["src_frame"] >= 0
    assert (plain["img"] != lay["img"])[held].mean() > 0.5 and (plain["src_ping"] == lay["src_ping"]).all()


# ---------------------------------------------------------------- 3. segments, yaw fan and pyramid under the banded table
def _same_seg(d, rr, pair_index, what):
    assert (int(d["pair"]), int(d["seg"]), int(d["p0"]), int(d["p1"])) == (pair_index, rr["seg"], rr["p0"], rr["p1"]), what
    assert R.same_result(d["r"], rr["r"]), "%s: result %s, reference %s" % (what, d["r"], rr["r"])
    assert (int(d["sx"]), int(d["sy"])) == (rr["sx"], rr["sy"]), "%s: centroid sums" % what


def test_segments_under_the_banded_table(clean, orc, data):
    from diasss_amd import capi
    tab, cor = _corrected(orc, data)
    rows = [data[0]["pose"], E.drift(data[1]["pose"])]                   # the drifted survey of tests/test_gpu_register_segments.py
    p = _grid(orc, data, [0, 1], rows, 0.1, 1)
    ga, gb = _geo(orc, data[0], rows[0]), _geo(orc, data[1], rows[1])
    la = R.mean_layer(ga[0], ga[1], cor[0], data[0]["mask"], p, 1)
    ref = E.register_segments(la, gb[0], gb[1], cor[1], data[1]["mask"], p, 80, 8, 256)
    rpy, off = _traj(rows)
    clean.mosaic_gain_set(tab, bands=K.BANDS)
    dev, sums = clean.mosaic_register_segments([0, 1], p, [(0, 1)], 80, reg=capi.RegParams(8, 256), rpy6=rpy, ping_off=off, want_sums=True)
    assert len(dev) == len(ref) == 8
    for s, rr in enumerate(ref):
        assert (sums[s].astype(np.int64) == rr["sums"]).all(), "segment %d: sums differ" % s
        _same_seg(dev[s], rr, 0, "segment %d" % s)
    assert sum(r["r"]["zncc"] > -2.0 for r in ref) >= 4


def test_yaw_fan_under_the_banded_table(clean, orc, data):
    from diasss_amd import capi
    tab, cor = _corrected(orc, data)
    nyaw, step, m = Y.FANS["one_step_up"]
    rows = [data[0]["true"], Y.rotated_survey(orc, data[1]["true"], Y.SEG, m, step, Y.SHIFT, Y.CELL)]          # the turned survey of tests/test_gpu_register_yaw.py
    p = _grid(orc, data, [0, 1], rows, Y.CELL, 1)
    ga = _geo(orc, data[0], rows[0])
    la = R.mean_layer(ga[0], ga[1], cor[0], data[0]["mask"], p, 1)
    ref = Y.register_segments_yaw(orc, la, rows[1], data[1]["gr"], M, cor[1], data[1]["mask"], p, 97, 6, 256, 3, step)
    rpy, off = _traj(rows)
    clean.mosaic_gain_set(tab, bands=K.BANDS)
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


def test_pyramid_under_the_banded_table(clean, orc, data):
    from diasss_amd import capi
    tab, cor = _corrected(orc, data)
    rows = [data[0]["true"], data[1]["true"] + np.array([0, 0, 0, P.MOVE[0], P.MOVE[1], 0])]                   # the moved survey of tests/test_gpu_register_pyr.py
    g = [_geo(orc, data[f], rows[f]) for f in (0, 1)]
    gx = np.concatenate([a[0].ravel() for a in g]); gy = np.concatenate([a[1].ravel() for a in g])
    p = P.awkward_grid(lambda *v: capi.MosaicParams(*v, 0, 0), (gx.min(), gx.max(), gy.min(), gy.max()), P.CELL, g[1][0], g[1][1], P.SEG)
    p.use_mask = 1
    acc = P.accumulators(g[0][0], g[0][1], cor[0], data[0]["mask"], p, 1)
    ref = P.register_segments_pyr(acc, g[1][0], g[1][1], cor[1], data[1]["mask"], p, P.SEG, P.RADIUS, P.MIN_CELLS, 3, P.REFINE)
    rpy, off = _traj(rows)
    clean.mosaic_gain_set(tab, bands=K.BANDS)
    dev, sums = clean.mosaic_register_segments_pyr([0, 1], p, [(0, 1)], P.SEG, pyr=capi.RegPyrParams(3, P.REFINE), reg=capi.RegParams(P.RADIUS, P.MIN_CELLS),
                                                   rpy6=rpy, ping_off=off, want_sums=True)
    assert len(dev) == len(ref) == 8
    for s, rr in enumerate(ref):
        d = dev[s]
        assert (sums[s].astype(np.int64) == rr["sums"]).all(), "segment %d: sums differ" % s
        assert (int(d["level"]), int(d["border_mask"])) == (rr["level"], rr["border_mask"])
        assert d["lx"].tolist() == rr["lx"] and d["ly"].tolist() == rr["ly"] and np.asarray(d["lz"], np.float64).tobytes() == np.asarray(rr["lz"], np.float64).tobytes()
        _same_seg(d["s"], rr, 0, "segment %d" % s)
    assert any(r["level"] == 0 for r in ref)


# ---------------------------------------------------------------- 4. byte identity, set / get
def test_byte_identity(clean, orc, data):
    """all seven entries: a one-band table through dsss_mosaic_gain_set_banded gives the bytes of the same table through
    dsss_mosaic_gain_set; a banded table whose rows are all equal gives the bytes of the column table; a cleared table gives the bytes
    taken before anything was set; and the real banded table gives other bytes than the column table"""
    col = np.array(K.effect_case(orc)["col"][2], np.uint16)
    clean.mosaic_gain_set(col)
    by_set = _snapshot(clean)
    clean.mosaic_gain_set(col[None, :], bands=(123.0, 0.001, 1))
    one = _snapshot(clean)
    clean.mosaic_gain_set(np.tile(col, (NB, 1)), bands=K.BANDS)
    equal = _snapshot(clean)
    clean.mosaic_gain_set(_real_table(orc), bands=K.BANDS)
    real = _snapshot(clean)
    clean.mosaic_gain_set(None, bands=None)
    after = _snapshot(clean)
    assert set(by_set) == {"render", "consistency", "register", "segments", "yaw", "pyr", "composite"}
    for k in by_set:
        assert one[k] == by_set[k], "%s: one band through set_banded" % k
        assert equal[k] == by_set[k], "%s: equal rows" % k
        assert after[k] == clean.before[k], "%s: after the table was cleared" % k
        assert by_set[k] != clean.before[k] and real[k] != by_set[k], "%s does not see the table" % k
    clean.mosaic_gain_set(_real_table(orc), bands=K.BANDS)
    clean.L.dsss_mosaic_gain_set_banded(clean.h, None, 0, None)                       # a NULL table clears, whatever else is passed
    assert clean.mosaic_gain_get_banded() is None and _snapshot(clean)["render"] == clean.before["render"]


def test_set_get_round_trip(clean, orc):
    from diasss_amd import capi
    tab = _real_table(orc)
    clean.mosaic_gain_set(tab, bands=K.BANDS)
    got, b = clean.mosaic_gain_get_banded()
    assert got.tolist() == tab.tolist() and (b.alt0, b.dalt, b.nbands) == K.BANDS
    out = np.full(M, 7, np.uint16); Mout = capi.C.c_int(-1)
    assert clean.L.dsss_mosaic_gain_get(clean.h, capi._ptr(out), M, capi.C.byref(Mout)) == E_STATE       # a 6-band table: not this entry's
    assert Mout.value == -1 and (out == 7).all()                                                         # ... and it writes nothing
    with pytest.raises(capi.DsssError) as e:
        clean.mosaic_gain_get()
    assert e.value.code == E_STATE
    clean.mosaic_gain_set(tab[2])                                                                        # a one-band set: it works again
    assert clean.mosaic_gain_get().tolist() == tab[2].tolist()
    got, b = clean.mosaic_gain_get_banded()
    assert got.tolist() == [tab[2].tolist()] and (b.alt0, b.dalt, b.nbands) == (0.0, 1.0, 1)
    clean.mosaic_gain_set(tab[:1], bands=(K.BANDS[0], K.BANDS[1], 1))                                    # one band through the banded entry
    assert clean.mosaic_gain_get().tolist() == tab[0].tolist()
    clean.mosaic_gain_set(None)
    assert clean.mosaic_gain_get() is None and clean.mosaic_gain_get_banded() is None


# ---------------------------------------------------------------- 5. the effect
def test_effect_is_the_references(clean, orc, data):
    """Under the true poses, cell 0.1, mask on: the device's banded statistics, table and consistency scores with no table, the column
    table and the banded table are the reference's, so the ordering tests/test_mosaic_gain_bands_cpu.py::test_effect_precondition proves
    holds on the device: 32.01 (none) -> 19.83 (column) -> 9.29 (banded)."""
    from diasss_amd import capi
    case = K.effect_case(orc)
    sc = K.scores(orc)
    q = case["p"]
    p = capi.MosaicParams(q.x0, q.y0, q.cell, q.W, q.H, 1, 0)
    S, C = clean.mosaic_gain_stats([0, 1], 1, bands=K.BANDS)
    assert S.tolist() == case["S"] and C.tolist() == case["C"]
    gp = capi.GainParams(K.MIN_COUNT, K.SMOOTH, K.TARGET, 0)
    tab, T = capi.mosaic_gain_table(S, C, gp, nbands=NB)
    assert tab.tolist() == case["gain"] and T == case["T"]
    cS, cC = clean.mosaic_gain_stats([0, 1], 1)
    ctab, cT = capi.mosaic_gain_table(cS, cC, gp)
    assert ctab.tolist() == case["col"][2] and cT == case["col"][3] == T
    rpy, off = _traj([data[0]["true"], data[1]["true"]])
    got = {}
    for name, table, bands, norms in (("none", None, None, None), ("column", ctab, None, case["corrected_col"]), ("banded", tab, K.BANDS, case["corrected"])):
        clean.mosaic_gain_set(table, bands=bands)
        ref = KC.consistency(KC.frames_of(case["legs"], norms), q, 1)
        nfr, s1, s2, score = clean.mosaic_consistency([0, 1], p, rpy6=rpy, ping_off=off)
        print("%s: score %.3f (reference %.3f)" % (name, score, ref[3]))
        assert _same(nfr, ref[0]) and _same(s1, ref[1]) and _same(s2, ref[2]) and abs(score - ref[3]) <= 1e-12 * ref[3]
        assert abs(ref[3] - sc[name]) <= 1e-12 * ref[3]
        got[name] = score
        for f in (0, 1):
            assert (clean.frame_corrected(f) == (data[f]["norm"] if norms is None else norms[f])).all(), "%s: corrected waterfall of frame %d" % (name, f)
    assert got["banded"] < got["column"] < got["none"]


# ---------------------------------------------------------------- 6. errors
def _code(fn, *a, **kw):
    from diasss_amd import capi
    with pytest.raises(capi.DsssError) as e:
        fn(*a, **kw)
    return e.value.code


def test_errors_leave_context_and_table(clean, orc, data):
    from diasss_amd import capi
    tab = _real_table(orc)
    clean.mosaic_gain_set(tab, bands=K.BANDS)
    p = capi.mosaic_grid(clean.mosaic_bounds([0, 1]), 0.1)
    good = clean.mosaic_render([0, 1], p)[0].tobytes()
    S0, C0 = clean.mosaic_gain_stats([0, 1], 1, bands=K.BANDS)
    L = clean.L
    Pt = capi._ptr
    nan, inf = float("nan"), float("inf")
    bad_bands = [(7.0, 1.0, 0), (7.0, 1.0, 17), (7.0, 1.0, -1), (nan, 1.0, 6), (inf, 1.0, 6), (-inf, 1.0, 6), (7.0, nan, 6), (7.0, inf, 6), (7.0, 0.0, 6),
                 (7.0, -1.0, 6)]
    # statistics: the bands, then whatever the column entry refuses
    for b in bad_bands:
        assert _code(clean.mosaic_gain_stats, [0, 1], 1, bands=b) == E_ARG, b
    assert _code(clean.mosaic_gain_stats, [0, 2], bands=K.BANDS) == E_ARG          # mixed M
    assert _code(clean.mosaic_gain_stats, [0, 0], bands=K.BANDS) == E_ARG          # listed twice
    assert _code(clean.mosaic_gain_stats, [0, 7], bands=K.BANDS) == E_ARG          # out of range
    assert _code(clean.mosaic_gain_stats, [], bands=K.BANDS) == E_ARG
    assert _code(clean.mosaic_gain_stats, [0, 3], bands=K.BANDS) == E_STATE        # not extracted
    ids = np.array([0, 1], np.int32); buf = np.zeros((NB, M), np.uint64); gb = capi.GainBands(*K.BANDS, 0)
    assert L.dsss_mosaic_gain_stats_banded(clean.h, Pt(ids), 2, 1, capi.C.byref(gb), None, Pt(buf)) == E_ARG
    assert L.dsss_mosaic_gain_stats_banded(clean.h, Pt(ids), 2, 1, capi.C.byref(gb), Pt(buf), None) == E_ARG
    assert L.dsss_mosaic_gain_stats_banded(clean.h, Pt(ids), 2, 1, None, Pt(buf), Pt(buf)) == E_ARG
    # set / get
    for b in bad_bands:
        nb = min(max(b[2], 1), 16)
        assert L.dsss_mosaic_gain_set_banded(clean.h, Pt(np.zeros((nb, M), np.uint16)), M, capi.C.byref(capi.GainBands(*b, 0))) == E_ARG, b
    assert L.dsss_mosaic_gain_set_banded(clean.h, Pt(tab), M, None) == E_ARG
    assert L.dsss_mosaic_gain_set_banded(clean.h, Pt(tab), 1, capi.C.byref(gb)) == E_ARG                  # M < 2
    out = np.zeros((NB, M), np.uint16); Mout = capi.C.c_int(-1); bout = capi.GainBands()
    assert L.dsss_mosaic_gain_get_banded(clean.h, Pt(out), NB * M - 1, capi.C.byref(Mout), capi.C.byref(bout)) == E_ARG      # cap below nbands x M
    assert Mout.value == M and bout.nbands == NB                                                          # the size is told all the same
    assert L.dsss_mosaic_gain_get_banded(clean.h, None, 0, capi.C.byref(Mout), capi.C.byref(bout)) == E_ARG
    assert L.dsss_mosaic_gain_get_banded(clean.h, Pt(out), NB * M, None, capi.C.byref(bout)) == E_ARG
    assert L.dsss_mosaic_gain_get_banded(clean.h, Pt(out), NB * M, capi.C.byref(Mout), None) == E_ARG
    # the corrected waterfall
    assert _code(clean.frame_corrected, 3) == E_STATE                              # not extracted
    assert _code(clean.frame_corrected, 2) == E_ARG                                # a table of another M
    assert L.dsss_frame_get_corrected(clean.h, 0, None) == E_ARG
    assert L.dsss_frame_get_corrected(clean.h, 9, Pt(np.zeros((N, M), np.uint8))) == E_ARG
    assert L.dsss_frame_get_corrected(clean.h, -1, Pt(np.zeros((N, M), np.uint8))) == E_ARG
    # a banded table of another M under every entry: refused before anything happens
    pairs = [(0, 2)]
    p2 = capi.mosaic_grid(clean.mosaic_bounds([0, 2]), 0.1)
    assert _code(clean.mosaic_render, [0, 2], p2) == E_ARG
    assert _code(clean.mosaic_consistency, [0, 2], p2) == E_ARG
    assert _code(clean.mosaic_register, [0, 2], p2, pairs) == E_ARG
    assert _code(clean.mosaic_register_segments, [0, 2], p2, pairs, 80) == E_ARG
    assert _code(clean.mosaic_register_segments_yaw, [0, 2], p2, pairs, 80, yaw=capi.RegYawParams(3, 0, 0.01)) == E_ARG
    assert _code(clean.mosaic_register_segments_pyr, [0, 2], p2, pairs, 80, pyr=capi.RegPyrParams(2, P.REFINE)) == E_ARG
    assert _code(clean.mosaic_composite, [0, 2], p2) == E_ARG
    assert _code(clean.mosaic_render, [0, 3], p) == E_STATE                        # the state rule comes first, as without a table
    # the context is usable, the table is the one that was set, and valid calls give what they gave
    got, b = clean.mosaic_gain_get_banded()
    assert got.tolist() == tab.tolist() and (b.alt0, b.dalt, b.nbands) == K.BANDS
    assert clean.mosaic_render([0, 1], p)[0].tobytes() == good
    S1, C1 = clean.mosaic_gain_stats([0, 1], 1, bands=K.BANDS)
    assert S1.tolist() == S0.tolist() and C1.tolist() == C0.tolist()
    # the statistics are those of the uncorrected samples, table or not
    assert S0.tolist() == K.effect_case(orc)["S"]
    # frames of another M are fine again once the table is gone
    clean.mosaic_gain_set(None)
    clean.mosaic_render([0, 2], p2)
    assert (clean.frame_corrected(2) == data[2]["norm"]).all()

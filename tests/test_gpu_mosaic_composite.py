"""GPU parity of the composite mosaic (dsss_mosaic_composite), exact on every layer and on the cell counts.

Nothing expected comes from the code under test: geo coordinates are the oracle's geo_img, grey levels the oracle's normalised image,
the mask the oracle's filter mask; ranks, winners, gain correction and fill come from tests/mosaic_composite_ref.py.  Frames 0 and 1
are the two legs of tests/test_gpu_mosaic.py (tests/mosaic_composite_cases.py; tests/test_mosaic_composite_cpu.py proves the
preconditions of these cases on the reference alone), 2 is leg 0 once more, 3 is leg 0 set and never extracted."""
import itertools

import numpy as np
import pytest

from tests import extract_shapes_ref as X
from tests import mosaic_composite_cases as K
from tests import mosaic_composite_ref as CR

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -2, -4


# ---------------------------------------------------------------- context and comparisons
@pytest.fixture(scope="module")
def ctx(orc):
    from diasss_amd import capi
    L = K.legs(orc)
    c = capi.Context(max_frames=4)
    for i, l in enumerate((L[0], L[1], L[0], L[0])):
        c.frame_set(i, l["raw"], l["N"], l["M"], l["pose"], l["alt"], l["gr"])
    c.extract_many([0, 1, 2])
    assert c.mosaic_gain_get() is None
    yield c
    c.close()


@pytest.fixture
def clean(ctx):
    """the context without a gain table, before and after the test"""
    ctx.mosaic_gain_set(None)
    yield ctx
    ctx.mosaic_gain_set(None)


def _dev_params(p, **kw):
    from diasss_amd import capi
    q = capi.MosaicParams(p.x0, p.y0, p.cell, p.W, p.H, p.use_mask, 0)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def _check(dev, info, ref, what=""):
    lay, counts, _ = ref
    for name in CR.LAYERS:
        d = dev[name]
        assert d.shape == lay[name].shape, "%s %s: shape" % (what, name)
        bad = d.astype(np.int64) != lay[name]
        assert not bad.any(), "%s %s differs in %d cells, first at %s: device %s, reference %s" % (
            what, name, int(bad.sum()), np.argwhere(bad)[0].tolist(), d[bad][:4].tolist(), lay[name][bad][:4].tolist())
    assert (info.direct, info.filled, info.empty) == counts, "%s: counts %s, reference %s" % (what, (info.direct, info.filled, info.empty), counts)


def _bytes(dev, info):
    return b"".join(dev[n].tobytes() for n in CR.LAYERS) + bytes(info)


def _packed(rows_list, gaps, seed=5):
    """the frames' rows packed into one rpy6 array with unrelated rows in front of each -> (rpy6, ping_off)"""
    rng = np.random.default_rng(seed)
    parts, off, n = [], [], 0
    for rows, gap in zip(rows_list, gaps):
        parts.append(rng.standard_normal((gap, 6)) * 50.0); n += gap
        off.append(n); parts.append(rows); n += len(rows)
    return np.ascontiguousarray(np.concatenate(parts)), np.array(off, np.int32)


def _code(fn, *a, **kw):
    from diasss_amd import capi
    with pytest.raises(capi.DsssError) as e:
        fn(*a, **kw)
    return e.value.code


# ---------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("use_mask", [0, 1])
@pytest.mark.parametrize("cell", [0.05, 0.13, 1.7])
def test_parity(clean, orc, cell, use_mask):
    """cell 0.05 leaves holes, 0.13 puts several consecutive bins of a ping into one cell (runs within a wavefront), 1.7 thousands of
    samples of both frames (contended cells); all four modes, no fill"""
    L = K.legs(orc)
    p = K.full_grid(L, cell, use_mask)
    bb = clean.mosaic_bounds([0, 1])
    from diasss_amd import capi
    g = capi.mosaic_grid(bb, cell)
    assert (g.x0, g.y0, g.W, g.H) == (p.x0, p.y0, p.W, p.H)
    for mode in CR.MODES:
        ref = K.reference(orc, cell, use_mask, mode)
        dev, info = clean.mosaic_composite([0, 1], _dev_params(p), mode=mode)
        _check(dev, info, ref, "cell %g mask %d mode %d" % (cell, use_mask, mode))
        assert dev["img"].dtype == np.uint8 and dev["fill"].dtype == np.uint8 and dev["src_ping"].dtype == np.int32
        assert ref[1][0] > 100 and ref[1][1] == 0
        if cell == 1.7:
            assert ref[2]["fullest"] > 1000
    assert (K.reference(orc, cell, use_mask, CR.NEAR)[0]["src_col"] != K.reference(orc, cell, use_mask, CR.FAR)[0]["src_col"]).any()


# ---------------------------------------------------------------- 2. frame shapes
@pytest.mark.parametrize("shape", [(69, 86), (69, 1234)], ids=lambda s: "%dx%d" % s)
def test_frame_shapes(orc, shape):
    """69 x 86: one column chunk shorter than a wavefront's worth (86 = 64 + 22), and the port columns 0 and 1 fall in one cell with
    equal q and g, so col decides; 69 x 1234: five column chunks, the last with 210 columns"""
    from diasss_amd import capi
    rows, cols = shape
    c = capi.Context(max_frames=1)
    try:
        nf = [s[3] for s in X.WIDE_SHAPES if s[:2] == shape][0]
        raw, orb, oref = X.wide_case(orc, rows, cols, 1, nf)
        mp, op = X.device_params(c, X.SMALL_MASK, orb)
        c.set_params(mask=mp, orb=op)
        pose, alt, gr = X.dr_inputs(rows, cols)
        c.frame_set(0, raw, rows, cols, pose, alt, gr)
        c.extract(0)
        gx, gy = orc.geo_img(pose, gr, cols)
        assert gx[5, 0] == gx[5, 1] and gy[5, 0] == gy[5, 1]                        # columns 0 and 1 are one point
        fr = [dict(id=0, gx=gx, gy=gy, norm=oref["norm"], mask=oref["mask"])]
        for cell, use_mask, R in ((0.05, 0, 0), (0.13, 0, 2), (0.13, 1, 4)):
            p = K.grid(gx.min(), gx.max(), gy.min(), gy.max(), cell, use_mask)
            for mode in CR.MODES:
                ref = CR.composite(fr, p, use_mask, mode, R)
                dev, info = c.mosaic_composite([0], _dev_params(p), mode=mode, fill_radius=R)
                _check(dev, info, ref, "%d x %d cell %g mask %d mode %d R %d" % (rows, cols, cell, use_mask, mode, R))
                if not use_mask and cell == 0.05:                                # columns 0 and 1 of every ping tie in q and g: column 0 wins, never 1
                    assert ref[2]["ties_qg"] >= rows and (ref[0]["src_col"] == 0).sum() > 10 and not (ref[0]["src_col"] == 1).any()
    finally:
        c.close()


def test_more_frames_than_the_resolve_stages(orc):
    """1030 frames of 69 x 86, one raw image under poses 0.07 m apart across the track: above 1024 jobs mosaic_resolve_kernel searches the
    job table where it lies, and g runs to 71 070; winners come from hundreds of frames, whatever the order of ids"""
    from diasss_amd import capi
    F, rows, cols = 1030, 69, 86
    c = capi.Context(max_frames=F)
    try:
        raw, orb, oref = X.wide_case(orc, rows, cols, 1, 50)
        mp, op = X.device_params(c, X.SMALL_MASK, orb)
        c.set_params(mask=mp, orb=op)
        pose, alt, gr = X.dr_inputs(rows, cols)
        fr = []
        for f in range(F):
            pf = pose.copy(); pf[:, 4] += 0.07 * f; pf[:, 3] += 0.013 * (f % 7)
            c.frame_set(f, raw, rows, cols, pf, alt, gr)
            gx, gy = orc.geo_img(pf, gr, cols)
            fr.append(dict(id=f, gx=gx, gy=gy, norm=oref["norm"], mask=oref["mask"]))
        c.extract_many(list(range(F)))
        gx = np.concatenate([f["gx"].ravel() for f in fr[::F - 1]]); gy = np.concatenate([f["gy"].ravel() for f in fr[::F - 1]])
        p = K.grid(gx.min(), gx.max(), gy.min(), gy.max(), 0.1, 1)
        ids = np.random.default_rng(F).permutation(F)
        for mode, R in ((CR.FAR, 0), (CR.FIRST, 1)):
            ref = CR.composite(fr, p, 1, mode, R)
            dev, info = c.mosaic_composite(ids, _dev_params(p), mode=mode, fill_radius=R)
            _check(dev, info, ref, "%d frames, mode %d" % (F, mode))
        assert len(np.unique(ref[0]["src_frame"])) > 300 and ref[0]["src_frame"].max() > 1024
    finally:
        c.close()


# ---------------------------------------------------------------- 3. ties between frames
def test_ties_by_frame(clean, orc):
    """the same raw frame as ids 0 and 2 under identical poses: every sample exists twice with equal q and col, and the smaller g,
    frame 0's, wins everywhere -- whatever the order of ids"""
    L = K.legs(orc)
    fr = K.frames([L[0], L[0]], ids=(0, 2))
    gx, gy = L[0]["gx"], L[0]["gy"]
    p = K.grid(gx.min(), gx.max(), gy.min(), gy.max(), 0.13, 0)
    for mode in (CR.NEAR, CR.FIRST):
        ref = CR.composite(fr, p, 0, mode, 1)
        assert set(np.unique(ref[0]["src_frame"]).tolist()) == {-1, 0}
        a = clean.mosaic_composite([0, 2], _dev_params(p), mode=mode, fill_radius=1)
        b = clean.mosaic_composite([2, 0], _dev_params(p), mode=mode, fill_radius=1)
        _check(a[0], a[1], ref, "ids 0, 2 mode %d" % mode)
        assert _bytes(*a) == _bytes(*b)
        if mode == CR.FIRST:                                                      # the lowest g of the cell: the smallest ping of frame 0 that reaches it
            S = CR.samples(fr[:1], p, 0, mode)
            first = np.full(p.W * p.H, 1 << 40, np.int64)
            np.minimum.at(first, S["cell"], S["ping"])
            v = ref[0]["fill"].ravel() == 0
            assert (a[0]["src_ping"].ravel()[v] == first[v]).all()


# ---------------------------------------------------------------- 4. order and repetition
def test_order_and_repeat(clean, orc):
    L = K.legs(orc)
    p = _dev_params(K.full_grid(L, 0.13, 1))
    rows = [L[0]["pose"], L[1]["pose"] + np.array([0, 0, 0.01, 0.3, 0.2, 0]), L[0]["pose"] + np.array([0, 0, -0.02, 1.1, -0.7, 0])]
    rpy, off = _packed(rows, (4, 9, 2))
    for traj in (False, True):
        got = []
        for perm in ((0, 1, 2), (2, 0, 1), (1, 2, 0), (0, 1, 2)):
            kw = dict(rpy6=rpy, ping_off=off[list(perm)].copy()) if traj else {}
            got.append(_bytes(*clean.mosaic_composite(list(perm), p, mode=CR.MID, fill_radius=2, **kw)))
        assert got[0] == got[1] == got[2] == got[3]
    geo = [orc.geo_img(np.ascontiguousarray(r), l["gr"], l["M"]) for r, l in zip(rows, (L[0], L[1], L[0]))]
    fr = [dict(id=i, gx=g[0], gy=g[1], norm=l["norm"], mask=l["mask"]) for i, (g, l) in enumerate(zip(geo, (L[0], L[1], L[0])))]
    ref = CR.composite(fr, p, 1, CR.MID, 2)
    dev, info = clean.mosaic_composite([1, 2, 0], p, mode="mid", fill_radius=2, rpy6=rpy, ping_off=off[[1, 2, 0]].copy())
    _check(dev, info, ref, "three frames under a trajectory")
    assert all(int((ref[0]["src_frame"] == f).sum()) > 100 for f in (0, 1, 2))


# ---------------------------------------------------------------- 5. trajectory override, dropped pings and the fill
@pytest.mark.parametrize("R", [0, 1, 2, 4])
def test_trajectory_override_and_fill(clean, orc, R):
    """the dead-reckoning rows as a packed trajectory with gaps, the pings of K.BAD_PINGS made NaN: 641 x 823 cells, 21 x 103 fill tiles"""
    L = K.legs(orc)
    rows = [l["pose"].copy() for l in L]
    rows[0][K.BAD_PINGS, 3] = np.nan
    rpy, off = _packed(rows, (5, 7))
    p = K.full_grid(L, 0.05, 0)
    assert (p.W, p.H) == (641, 823)
    ref = K.reference(orc, 0.05, 0, CR.NEAR, R=R, bad=True)
    dev, info = clean.mosaic_composite([0, 1], _dev_params(p), fill_radius=R, rpy6=rpy, ping_off=off)
    _check(dev, info, ref, "R %d" % R)
    print("R %d: direct %d, filled %d, empty %d" % (R, info.direct, info.filled, info.empty))
    assert (info.filled > 0) == (R > 0)


def test_fill_on_a_clipped_grid(clean, orc):
    """a window of 153 x 311 cells inside the survey, no multiple of the fill tile: its lower edge cuts the gap of the pings 200-202
    where leg 0 alone covers the ground (holes on the border that are enclosed along x), its right edge lies in the gap of the pings
    300-305 (holes whose samples on the far side fall outside the grid, which are not in V0: they stay empty); the halo of the border
    tiles is clipped"""
    L = K.legs(orc)
    full = K.full_grid(L, 0.05, 0)
    q = _dev_params(full, x0=full.x0 + 150 * full.cell, y0=full.y0 + 20 * full.cell, W=153, H=311)
    assert q.W % 32 and q.H % 8
    fr = K.frames(L, keep=K.bad_keep(L))
    rows = [l["pose"].copy() for l in L]
    rows[0][K.BAD_PINGS, 4] = np.inf
    rpy, off = _packed(rows, (0, 3))
    edge = np.zeros((q.H, q.W), bool); edge[0] = edge[-1] = True; edge[:, 0] = edge[:, -1] = True
    filled = []
    for R in (1, 4):
        ref = CR.composite(fr, q, 0, CR.MID, R)
        fl = ref[0]["fill"]
        assert ((fl == 255) & edge).sum() > 50 and ((fl == 0) & edge).sum() > 100 and (fl[:, -1] == 255).sum() > 50
        dev, info = clean.mosaic_composite([1, 0], q, mode=CR.MID, fill_radius=R, rpy6=rpy, ping_off=off[::-1].copy())
        _check(dev, info, ref, "clipped, R %d" % R)
        filled.append((ref[1][1], int(((fl > 0) & (fl < 255) & edge).sum())))
    assert filled[1][0] > filled[0][0] + 100 and filled[1][1] > 0                # R = 4 closes the three-ping gap, on the border too


# ---------------------------------------------------------------- 6. under a gain table
def test_under_a_gain_table(clean, orc):
    """frames 0 and 2 (leg 0 twice, the second moved by a trajectory) under a constructed table with gains of 0 and clamping gains: the
    values are the reference's fed the corrected levels, the sources those without a table; a table of 256s and a cleared table give
    the bytes taken before any table was set"""
    L = K.legs(orc)
    M = L[0]["M"]
    moved = L[0]["pose"].copy()
    moved[:, 2] += np.linspace(0.0, 0.05, L[0]["N"]); moved[:, 3] += 0.7; moved[:, 4] -= 0.4
    rpy, off = _packed([L[0]["pose"], moved], (3, 11))
    geo = [(L[0]["gx"], L[0]["gy"]), orc.geo_img(moved, L[0]["gr"], M)]
    fr = [dict(id=i, gx=g[0], gy=g[1], norm=L[0]["norm"], mask=L[0]["mask"]) for i, g in zip((0, 2), geo)]
    gx = np.concatenate([g[0].ravel() for g in geo]); gy = np.concatenate([g[1].ravel() for g in geo])
    tab = np.random.default_rng(3).integers(150, 400, M).astype(np.uint16)
    tab[::7] = 0; tab[3::11] = 65535; tab[5::13] = 1024; tab[1::17] = 256; tab[190:210] = 0
    for use_mask, mode, R in ((1, CR.NEAR, 0), (0, CR.FAR, 2)):
        p = K.grid(gx.min(), gx.max(), gy.min(), gy.max(), 0.1, use_mask)
        q = _dev_params(p)
        kw = dict(mode=mode, fill_radius=R, rpy6=rpy, ping_off=off)
        before = clean.mosaic_composite([0, 2], q, **kw)
        plain = CR.composite(fr, p, use_mask, mode, R)
        _check(before[0], before[1], plain, "no table")
        clean.mosaic_gain_set(tab)
        ref = CR.composite(fr, p, use_mask, mode, R, gain=tab)
        under = clean.mosaic_composite([0, 2], q, **kw)
        _check(under[0], under[1], ref, "under the table")
        v = ref[0]["fill"] < 255
        assert (ref[0]["img"][v] == 255).mean() > 0.02 and (ref[0]["img"][v] == 0).mean() > 0.1 and (ref[0]["img"] != plain[0]["img"])[v].mean() > 0.5
        for name in ("src_frame", "src_ping", "src_col", "fill"):
            assert under[0][name].tobytes() == before[0][name].tobytes(), "%s moved under the table" % name
        clean.mosaic_gain_set(np.full(M, 256, np.uint16))
        assert _bytes(*clean.mosaic_composite([0, 2], q, **kw)) == _bytes(*before)
        clean.mosaic_gain_set(tab)
        clean.mosaic_gain_set(None)
        assert _bytes(*clean.mosaic_composite([0, 2], q, **kw)) == _bytes(*before)


# ---------------------------------------------------------------- 7. the mean mosaic is untouched
def test_mean_mosaic_untouched(clean, orc):
    L = K.legs(orc)
    p = _dev_params(K.full_grid(L, 0.13, 1))
    before = clean.mosaic_render([0, 1], p)
    clean.mosaic_composite([0, 1], p, mode=CR.FAR, fill_radius=4)
    clean.mosaic_composite([0, 1], p, want=())
    after = clean.mosaic_render([0, 1], p)
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- 8. errors and NULL outputs
def test_errors_leave_the_context_usable(clean, orc):
    from diasss_amd import capi
    L = K.legs(orc)
    p = _dev_params(K.full_grid(L, 1.7, 1))
    ref = K.reference(orc, 1.7, 1, CR.NEAR)

    def still_right():
        dev, info = clean.mosaic_composite([0, 1], p)
        _check(dev, info, ref, "after an error")

    f = clean.mosaic_composite
    rpy, off = _packed([l["pose"] for l in L], (0, 0))
    calls = [
        (E_ARG, lambda: f([0, 1], p, mode=4)),
        (E_ARG, lambda: f([0, 1], p, mode=-1)),
        (E_ARG, lambda: f([0, 1], p, fill_radius=5)),
        (E_ARG, lambda: f([0, 1], p, fill_radius=-1)),
        (E_STATE, lambda: f([0, 3], p)),                                           # set, never extracted
        (E_ARG, lambda: f([0, 1], p, rpy6=rpy)),
        (E_ARG, lambda: f([0, 1, 0], p)),
        (E_ARG, lambda: f([0, 4], p)),
        (E_ARG, lambda: f([], p)),
        (E_ARG, lambda: f([0, 1], _dev_params(p, cell=0.0))),
        (E_ARG, lambda: f([0, 1], _dev_params(p, W=0))),
        (E_ARG, lambda: f([0, 1], _dev_params(p, W=1 << 15, H=(1 << 13) + 1))),
    ]
    for code, call in calls:
        assert _code(call) == code
        still_right()
    # a gain table of another M than a listed frame's: refused, and the table stays
    tab = np.full(L[0]["M"], 300, np.uint16)
    clean.mosaic_gain_set(tab)
    assert _code(f, [0, 1], p) == E_ARG
    assert _code(f, [0, 1], p, mode=7) == E_ARG
    assert clean.mosaic_gain_get().tolist() == tab.tolist()
    f([0, 2], p)                                                                   # frames of the table's M are served
    clean.mosaic_gain_set(None)
    still_right()


def test_null_outputs(clean, orc):
    """every combination of NULL outputs: the call succeeds, what was asked for is what the full call gives, nothing else is needed"""
    from diasss_amd import capi
    L = K.legs(orc)
    p = _dev_params(K.full_grid(L, 1.7, 0))
    ids = np.array([0, 1], np.int32)
    cp = capi.CompParams(CR.MID, 2)
    full, info = clean.mosaic_composite([0, 1], p, mode=CR.MID, fill_radius=2)
    _check(full, info, K.reference(orc, 1.7, 0, CR.MID, R=2), "all outputs")
    names = [n for n, _ in capi.COMP_LAYERS]
    for mask in itertools.product((0, 1), repeat=6):
        out = {n: np.full((p.H, p.W), 99, t) for (n, t), m in zip(capi.COMP_LAYERS, mask) if m}
        inf = capi.CompInfo(-1, -1, -1) if mask[5] else None
        rc = clean.L.dsss_mosaic_composite(clean.h, capi._ptr(ids), 2, None, None, capi.C.byref(p), capi.C.byref(cp),
                                           *[capi._ptr(out.get(n)) for n in names], capi.C.byref(inf) if inf is not None else None)
        assert rc == 0, mask
        for n in out:
            assert out[n].tobytes() == full[n].tobytes(), (mask, n)
        if inf is not None:
            assert bytes(inf) == bytes(info)
    # NULL parameters are the defaults: near, no fill
    out = np.empty((p.H, p.W), np.uint8)
    assert clean.L.dsss_mosaic_composite(clean.h, capi._ptr(ids), 2, None, None, capi.C.byref(p), None, capi._ptr(out), None, None, None, None, None) == 0
    assert (out == K.reference(orc, 1.7, 0, CR.NEAR)[0]["img"]).all()
    dev, inf = clean.mosaic_composite([0, 1], p, want=("info",))
    assert dev == {} and (inf.direct, inf.filled, inf.empty) == K.reference(orc, 1.7, 0, CR.NEAR)[1]
    assert clean.mosaic_composite([0, 1], p, want=()) == ({}, None)

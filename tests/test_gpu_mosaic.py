"""GPU parity of the georeferenced mosaic and the overlap-consistency map (dsss_mosaic_*), exact on every integer layer.

Nothing expected comes from the code under test: geo coordinates are the oracle's geo_img, grey levels the oracle's normalised image,
the mask the oracle's filter mask, and the binning is np.floor((g - origin) / cell) with np.add.at, here in the test."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -2, -4
from tests.helpers import MOSAIC_SIZES as SIZES


# ---------------------------------------------------------------- numpy reference
def _bin(gx, gy, norm, mask, p, use_mask, keep_rows=None):
    """(sum, cnt) of one frame over the grid p, int64 H x W"""
    W, H = p.W, p.H
    with np.errstate(invalid="ignore", over="ignore"):
        fx = np.floor((gx - p.x0) / p.cell); fy = np.floor((gy - p.y0) / p.cell)
        ok = (fx >= 0) & (fx < W) & (fy >= 0) & (fy < H)
    if use_mask:
        ok &= mask != 0
    if keep_rows is not None:
        ok &= keep_rows[:, None]
    idx = fy[ok].astype(np.int64) * W + fx[ok].astype(np.int64)
    s = np.zeros(W * H, np.int64); c = np.zeros(W * H, np.int64)
    np.add.at(s, idx, norm[ok].astype(np.int64)); np.add.at(c, idx, 1)
    return s.reshape(H, W), c.reshape(H, W), int(ok.sum())


def _mean(s, c):
    return np.where(c > 0, (s + c // 2) // np.maximum(c, 1), 0)


def ref_render(frames, p, use_mask):
    """frames: list of (gx, gy, norm, mask[, keep_rows]) -> sum, cnt, img, samples kept"""
    S = np.zeros((p.H, p.W), np.int64); Cn = np.zeros((p.H, p.W), np.int64); kept = 0
    for fr in frames:
        s, c, k = _bin(fr[0], fr[1], fr[2], fr[3], p, use_mask, fr[4] if len(fr) > 4 else None)
        S += s; Cn += c; kept += k
    return S, Cn, _mean(S, Cn), kept


def ref_consistency(frames, p, use_mask):
    nfr = np.zeros((p.H, p.W), np.int64); s1 = np.zeros_like(nfr); s2 = np.zeros_like(nfr)
    for fr in frames:
        s, c, _ = _bin(fr[0], fr[1], fr[2], fr[3], p, use_mask)
        m = _mean(s, c)
        nfr += c > 0; s1 += np.where(c > 0, m, 0); s2 += np.where(c > 0, m * m, 0)
    sel = nfr >= 2
    num = (s2[sel].astype(np.float64) - s1[sel].astype(np.float64) ** 2 / nfr[sel].astype(np.float64)).sum()
    den = float((nfr[sel] - 1).sum())
    return nfr, s1, s2, (float(np.sqrt(num / den)) if den > 0 else 0.0)


def _same(dev, ref):
    return dev.shape == ref.shape and (dev.astype(np.int64) == ref).all()


def _params(capi, p, **kw):
    q = capi.MosaicParams(p.x0, p.y0, p.cell, p.W, p.H, p.use_mask, 0)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


# ---------------------------------------------------------------- the two overlapping legs
@pytest.fixture(scope="module")
def ctx():
    from diasss_amd import capi
    c = capi.Context(max_frames=4)
    c.loaded = None                         # which set of frames the context holds
    yield c
    c.close()


@pytest.fixture(scope="module")
def legs(orc):
    """leg 0 at 640 x 400 heading +x, leg 1 at 500 x 700 heading back over it; seeded Rayleigh images; the oracle's products"""
    from tests import helpers as H
    out = []
    for leg, (N, M) in enumerate(SIZES):
        pose, alt, gr = H.track(N, M, leg, seed=9)
        raw = np.random.default_rng(leg).rayleigh(1.0, (N, M)) * 100.0
        gx, gy = orc.geo_img(pose, gr, M)
        out.append(dict(N=N, M=M, pose=pose, alt=alt, gr=gr, raw=raw, gx=gx, gy=gy, norm=orc.normalize(raw), mask=orc.mask(raw)))
    return out


@pytest.fixture
def pair(ctx, legs):
    """the context with the two legs in frames 0 and 1, extracted (set again when another test has replaced them)"""
    if ctx.loaded != "legs":
        for i, L in enumerate(legs):
            ctx.frame_set(i, L["raw"], L["N"], L["M"], L["pose"], L["alt"], L["gr"])
        ctx.extract_many([0, 1])
        ctx.loaded = "legs"
    return ctx


def _dr_frames(legs):
    return [(L["gx"], L["gy"], L["norm"], L["mask"]) for L in legs]


def _full_grid(capi, legs, cell):
    gx = np.concatenate([L["gx"].ravel() for L in legs]); gy = np.concatenate([L["gy"].ravel() for L in legs])
    return capi.mosaic_grid((gx.min(), gx.max(), gy.min(), gy.max()), cell)


# ---------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("cell", [0.05, 0.13, 1.7])
def test_render_parity(pair, legs, cell):
    """cell 0.13 puts several consecutive bins of a ping into one cell (runs within a wavefront), cell 1.7 thousands of samples of both frames
    (contended cells)"""
    from diasss_amd import capi
    bb = pair.mosaic_bounds([0, 1])
    gx = np.concatenate([L["gx"].ravel() for L in legs]); gy = np.concatenate([L["gy"].ravel() for L in legs])
    assert (bb == np.array([gx.min(), gx.max(), gy.min(), gy.max()])).all(), "bounds differ from the oracle's geo extremes"
    p = capi.mosaic_grid(bb, cell)
    assert p.use_mask == 1
    for use_mask in (0, 1):
        q = _params(capi, p, use_mask=use_mask)
        S, Cn, I, kept = ref_render(_dr_frames(legs), q, use_mask)
        s, c, img = pair.mosaic_render([0, 1], q)
        print("cell %g mask %d: grid %d x %d, %d samples kept, fullest cell %d" % (cell, use_mask, p.W, p.H, kept, Cn.max()))
        assert _same(c, Cn), "cnt differs"
        assert _same(s, S), "sum differs"
        assert _same(img, I), "img differs"
        assert kept > 10000 and Cn.max() >= (2 if cell < 0.1 else 4)
    if cell == 1.7:
        assert Cn.max() > 1000


def test_mask_polarity_is_not_vacuous(legs):
    """the masked case above only means something if the oracle's mask keeps some pixels and rejects others"""
    for L in legs:
        kept = (L["mask"] != 0).mean()
        assert 0.05 < kept < 0.95


# ---------------------------------------------------------------- 2. clipping
def test_render_clipped_grid(pair, legs):
    """origin inside the survey: samples left of and below it must drop out, not land in column or row 0 (floor, not truncation)"""
    from diasss_amd import capi
    full = _full_grid(capi, legs, 0.13)
    q = _params(capi, full, x0=full.x0 + (full.W // 4) * full.cell, y0=full.y0 + (full.H // 4) * full.cell, W=(full.W * 5) // 8, H=(full.H * 5) // 8,
                use_mask=0)
    S, Cn, I, kept = ref_render(_dr_frames(legs), q, 0)
    total = sum(L["N"] * L["M"] for L in legs)
    print("clipped grid %d x %d of %d x %d: reference drops %.1f %%" % (q.W, q.H, full.W, full.H, 100.0 * (total - kept) / total))
    assert 0.2 < (total - kept) / total < 0.8
    s, c, img = pair.mosaic_render([0, 1], q)
    assert _same(c, Cn) and _same(s, S) and _same(img, I)


# ---------------------------------------------------------------- 3. trajectory override
def _packed(rows_list, gaps, seed=5):
    """the frames' rows packed into one rpy6 array with unrelated rows in front of each -> (rpy6, ping_off)"""
    rng = np.random.default_rng(seed)
    parts, off, n = [], [], 0
    for rows, gap in zip(rows_list, gaps):
        parts.append(rng.standard_normal((gap, 6)) * 50.0); n += gap
        off.append(n); parts.append(rows); n += len(rows)
    return np.ascontiguousarray(np.concatenate(parts)), np.array(off, np.int32)


def test_trajectory_override(pair, legs, orc):
    from diasss_amd import capi
    p = _full_grid(capi, legs, 0.13)
    base = pair.mosaic_render([0, 1], p)
    rpy, off = _packed([L["pose"] for L in legs], (5, 7))
    assert off[1] != legs[0]["N"] and off[1] > 0
    same = pair.mosaic_render([0, 1], p, rpy6=rpy, ping_off=off)
    for a, b in zip(base, same):
        assert a.tobytes() == b.tobytes(), "the dead-reckoning rows given as a trajectory change the mosaic"
    moved, frames = [], []
    for L in legs:
        m = L["pose"].copy()
        m[:, 2] += np.linspace(0.0, 0.05, L["N"]); m[:, 3] += 0.7; m[:, 4] -= 0.4
        moved.append(m)
        gx, gy = orc.geo_img(m, L["gr"], L["M"])
        frames.append((gx, gy, L["norm"], L["mask"]))
    rpy, off = _packed(moved, (3, 11))
    bb = pair.mosaic_bounds([0, 1], rpy6=rpy, ping_off=off)
    gx = np.concatenate([f[0].ravel() for f in frames]); gy = np.concatenate([f[1].ravel() for f in frames])
    assert (bb == np.array([gx.min(), gx.max(), gy.min(), gy.max()])).all()
    q = capi.mosaic_grid(bb, 0.13)
    S, Cn, I, kept = ref_render(frames, q, 1)
    s, c, img = pair.mosaic_render([0, 1], q, rpy6=rpy, ping_off=off)
    assert _same(c, Cn) and _same(s, S) and _same(img, I)
    assert not _same(c, ref_render(_dr_frames(legs), q, 1)[1]), "the moved trajectory should give another mosaic"


# ---------------------------------------------------------------- 4. non-finite and huge poses
def test_bad_pings_are_dropped(pair, legs):
    from diasss_amd import capi
    p = _full_grid(capi, legs, 0.13)
    rows = [L["pose"].copy() for L in legs]
    rows[0][17, 3] = np.nan; rows[0][300, 4] = np.inf; rows[1][123, 3] = 1e300
    keep = [np.ones(L["N"], bool) for L in legs]
    keep[0][[17, 300]] = False; keep[1][123] = False
    rpy, off = _packed(rows, (0, 2))
    s, c, img = pair.mosaic_render([0, 1], p, rpy6=rpy, ping_off=off)          # returns DSSS_OK: no exception
    S, Cn, I, kept = ref_render([(L["gx"], L["gy"], L["norm"], L["mask"], k) for L, k in zip(legs, keep)], p, 1)
    assert _same(c, Cn) and _same(s, S) and _same(img, I)
    nfr, s1, s2, score = pair.mosaic_consistency([0, 1], p, rpy6=rpy, ping_off=off)
    assert np.isfinite(score) and int(nfr.max()) == 2


# ---------------------------------------------------------------- 5. consistency layers
@pytest.mark.parametrize("cell", [0.13, 0.5])
def test_consistency_layers(pair, legs, cell):
    from diasss_amd import capi
    p = _full_grid(capi, legs, cell)
    for use_mask in (1, 0):
        q = _params(capi, p, use_mask=use_mask)
        R = ref_consistency(_dr_frames(legs), q, use_mask)
        assert int((R[0] == 2).sum()) >= 100, "the legs do not overlap"
        nfr, s1, s2, score = pair.mosaic_consistency([0, 1], q)
        print("cell %g mask %d: %d cells seen twice, score %.15g (reference %.15g)" % (cell, use_mask, int((R[0] == 2).sum()), score, R[3]))
        assert _same(nfr, R[0]) and _same(s1, R[1]) and _same(s2, R[2])
        assert R[3] > 0 and abs(score - R[3]) <= 1e-12 * R[3]


def test_consistency_without_overlap(pair, legs):
    from diasss_amd import capi
    p = _full_grid(capi, legs, 0.5)
    nfr, s1, s2, score = pair.mosaic_consistency([1], p)
    R = ref_consistency(_dr_frames(legs)[1:], p, 1)
    assert _same(nfr, R[0]) and _same(s1, R[1]) and _same(s2, R[2]) and score == 0.0 and int(nfr.max()) == 1


# ---------------------------------------------------------------- 6. order and repeatability
def test_order_and_repeat(pair, legs):
    from diasss_amd import capi
    p = _full_grid(capi, legs, 0.13)
    rpy, off = _packed([L["pose"] + np.array([0, 0, 0.01, 0.3, 0.2, 0]) for L in legs], (4, 9))
    for kw01, kw10 in ((dict(), dict()), (dict(rpy6=rpy, ping_off=off), dict(rpy6=rpy, ping_off=off[::-1].copy()))):
        a = pair.mosaic_render([0, 1], p, **kw01); b = pair.mosaic_render([0, 1], p, **kw01); r = pair.mosaic_render([1, 0], p, **kw10)
        for x, y, z in zip(a, b, r):
            assert x.tobytes() == y.tobytes() == z.tobytes()
        a = pair.mosaic_consistency([0, 1], p, **kw01); b = pair.mosaic_consistency([0, 1], p, **kw01); r = pair.mosaic_consistency([1, 0], p, **kw10)
        for x, y, z in zip(a[:3], b[:3], r[:3]):
            assert x.tobytes() == y.tobytes() == z.tobytes()
        assert a[3] == b[3] == r[3]


# ---------------------------------------------------------------- 9. small and wide frames, a table of three jobs
def _shape_ctx(orc, rows, cols, poses):
    """a context of its own that holds the speckle frame of the extraction's wide shapes once per pose in `poses`, extracted under the
    small-frame mask -> (context, the oracle's (gx, gy, norm, mask) of every frame)"""
    from diasss_amd import capi
    from tests import extract_shapes_ref as X
    nf = [s[3] for s in X.WIDE_SHAPES if s[:2] == (rows, cols)][0]
    raw, orb, oref = X.wide_case(orc, rows, cols, 1, nf)
    _, alt, gr = X.dr_inputs(rows, cols)
    frames = [orc.geo_img(pose, gr, cols) + (oref["norm"], oref["mask"]) for pose in poses]
    c = capi.Context(max_frames=len(poses))
    try:
        mp, op = X.device_params(c, X.SMALL_MASK, orb)
        c.set_params(mask=mp, orb=op)
        for f, pose in enumerate(poses):
            c.frame_set(f, raw, rows, cols, pose, alt, gr)
        c.extract_many(list(range(len(poses))))
    except Exception:
        c.close()
        raise
    return c, frames


def _extremes_grid(capi, frames, cell):
    gx = np.concatenate([f[0].ravel() for f in frames]); gy = np.concatenate([f[1].ravel() for f in frames])
    return capi.mosaic_grid((gx.min(), gx.max(), gy.min(), gy.max()), cell)


@pytest.mark.parametrize("shape", [(69, 86), (69, 1234)], ids=lambda s: "%dx%d" % s)
def test_render_frame_shapes(orc, shape):
    """the mean scatter at the composite's frame shapes.  69 x 86: one column chunk whose second wavefront is part full (64 + 22), and
    columns 0 and 1 of a ping are one point, so a run starts in lane 0; 69 x 1234: five column chunks, the last with 210 columns.  On the
    grid of the frame's own extremes the unmasked reference keeps every sample, at cell 0.13 its fullest cell holds a run, and the
    mask keeps some samples and drops others"""
    from diasss_amd import capi
    from tests import extract_shapes_ref as X
    rows, cols = shape
    c, frames = _shape_ctx(orc, rows, cols, [X.dr_inputs(rows, cols)[0]])
    try:
        gx, gy = frames[0][:2]
        assert gx[5, 0] == gx[5, 1] and gy[5, 0] == gy[5, 1]                        # columns 0 and 1 are one point
        for cell in (0.05, 0.13):
            p = _extremes_grid(capi, frames, cell)
            kept = {}
            for use_mask in (0, 1):
                q = _params(capi, p, use_mask=use_mask)
                S, Cn, I, kept[use_mask] = ref_render(frames, q, use_mask)
                s, cn, img = c.mosaic_render([0], q)
                print("%d x %d cell %g mask %d: grid %d x %d, %d samples kept, fullest cell %d" % (rows, cols, cell, use_mask, p.W, p.H, kept[use_mask], Cn.max()))
                assert _same(cn, Cn), "cnt differs"
                assert _same(s, S), "sum differs"
                assert _same(img, I), "img differs"
                if cell == 0.13:
                    assert Cn.max() >= 2
            assert kept[0] == rows * cols
            assert 0 < kept[1] < kept[0]
    finally:
        c.close()


def test_three_job_table(orc):
    """the 69 x 86 frame as frames 0, 1 and 2 under poses 0.07 m apart across the track, so that they overlap: the job lookup of the
    scatter with more than two jobs (the render) and with a table per frame (the consistency map), listed as (2, 0, 1) and as (0, 1, 2)"""
    from diasss_amd import capi
    from tests import extract_shapes_ref as X
    rows, cols = 69, 86
    pose = X.dr_inputs(rows, cols)[0]
    poses = []
    for f in range(3):
        pf = pose.copy(); pf[:, 4] += 0.07 * f; pf[:, 3] += 0.013 * (f % 7)
        poses.append(pf)
    c, frames = _shape_ctx(orc, rows, cols, poses)
    try:
        p = _extremes_grid(capi, frames, 0.13)
        for use_mask in (0, 1):
            q = _params(capi, p, use_mask=use_mask)
            S, Cn, I, kept = ref_render(frames, q, use_mask)
            R = ref_consistency(frames, q, use_mask)
            print("mask %d: grid %d x %d, %d samples kept, %d cells seen by three frames, reference score %.15g" % (
                use_mask, p.W, p.H, kept, int((R[0] == 3).sum()), R[3]))
            assert int(R[0].max()) == 3 and R[3] > 0
            a = c.mosaic_render([2, 0, 1], q)
            assert _same(a[1], Cn) and _same(a[0], S) and _same(a[2], I)
            m = c.mosaic_consistency([2, 0, 1], q)
            assert _same(m[0], R[0]) and _same(m[1], R[1]) and _same(m[2], R[2])
            assert abs(m[3] - R[3]) <= 1e-12 * R[3]
            b = c.mosaic_render([0, 1, 2], q); n = c.mosaic_consistency([0, 1, 2], q)
            for x, y in zip(list(a) + list(m[:3]), list(b) + list(n[:3])):
                assert x.tobytes() == y.tobytes()
            assert m[3] == n[3]
    finally:
        c.close()


# ---------------------------------------------------------------- 8. errors
def test_errors_leave_the_context_usable(pair, legs):
    from diasss_amd import capi
    p = _full_grid(capi, legs, 1.7)
    S, Cn, I, _ = ref_render(_dr_frames(legs), p, 1)
    R = ref_consistency(_dr_frames(legs), p, 1)

    def still_right():
        s, c, img = pair.mosaic_render([0, 1], p)
        assert _same(c, Cn) and _same(s, S) and _same(img, I)
        nfr, s1, s2, score = pair.mosaic_consistency([0, 1], p)
        assert _same(nfr, R[0]) and _same(s1, R[1]) and _same(s2, R[2])

    L = legs[0]
    pair.frame_set(2, L["raw"], L["N"], L["M"], L["pose"], L["alt"], L["gr"])       # set, never extracted
    rpy, off = _packed([L["pose"] for L in legs], (0, 0))
    calls = [
        (E_STATE, lambda f: f([0, 2], p)),
        (E_ARG, lambda f: f([0, 1], p, rpy6=rpy)),
        (E_ARG, lambda f: f([0, 1, 0], p)),
        (E_ARG, lambda f: f([0, 4], p)),
        (E_ARG, lambda f: f([0, 1], _params(capi, p, cell=0.0))),
        (E_ARG, lambda f: f([0, 1], _params(capi, p, cell=float("nan")))),
        (E_ARG, lambda f: f([0, 1], _params(capi, p, W=0))),
        (E_ARG, lambda f: f([0, 1], _params(capi, p, W=1 << 15, H=(1 << 13) + 1))),
    ]
    for code, call in calls:
        for f in (pair.mosaic_render, pair.mosaic_consistency):
            with pytest.raises(capi.DsssError) as ei:
                call(f)
            assert ei.value.code == code
        still_right()
    assert (pair.mosaic_bounds([0, 2]) == pair.mosaic_bounds([0])).all()         # bounds need the geometry alone
    with pytest.raises(capi.DsssError) as ei:
        pair.mosaic_bounds([0, 1], rpy6=rpy)
    assert ei.value.code == E_ARG


# ---------------------------------------------------------------- 7. the score measures registration
def test_score_measures_registration(ctx, orc):
    from diasss_amd import capi
    from diasss_amd.synth import Survey
    F, N, M = 4, 640, 400
    sv = Survey(F, N, M, seed=31)
    raws = [sv.frame(f).numpy().copy() for f in range(F)]
    ctx.loaded = "survey"
    for f in range(F):
        pose, alt, gr = sv.inputs(f)
        ctx.frame_set(f, raws[f], N, M, pose, alt, gr)
    ctx.extract_many(list(range(F)))
    norms = [orc.normalize(r) for r in raws]; masks = [orc.mask(r) for r in raws]
    true = [np.ascontiguousarray(t) for t in sv.poses_true]
    shifted = [t + (np.array([0, 0, 0, 1.0, 1.0, 0]) if f % 2 else 0.0) for f, t in enumerate(true)]
    ids = list(range(F)); off = np.arange(F, dtype=np.int32) * N
    p = capi.mosaic_grid(ctx.mosaic_bounds(ids, rpy6=np.concatenate(true), ping_off=off), 0.25)
    refs = []
    for rows in (true, shifted):
        frames = [orc.geo_img(rows[f], sv.gr, M) + (norms[f], masks[f]) for f in range(F)]
        refs.append(ref_consistency(frames, p, 1))
    print("reference score under the true poses %.4f, with the odd legs shifted by (1, 1) m %.4f" % (refs[0][3], refs[1][3]))
    assert refs[1][3] > refs[0][3] > 0
    for rows, R in zip((true, shifted), refs):
        nfr, s1, s2, score = ctx.mosaic_consistency(ids, p, rpy6=np.concatenate(rows), ping_off=off)
        assert _same(nfr, R[0]) and _same(s1, R[1]) and _same(s2, R[2])
        assert abs(score - R[3]) <= 1e-12 * R[3]


# ---------------------------------------------------------------- the sample limit of a cell
def test_sample_limit_per_cell(ctx, orc):
    """2^24 samples is the most a cell may take (255 x 2^24 < 2^32: below it the uint32 sum cannot wrap).  One frame of 4200 x 4000 =
    16.8 M pixels into ONE cell is over the limit and must be reported, not wrapped; split over two cells it is under it, and the layers
    then hold every sample and every grey level (the packed accumulators at counts of millions, every wavefront on the same two cells)"""
    from diasss_amd import capi
    from tests import helpers as H
    E_CAPACITY = -5
    N, M = 4200, 4000
    assert N * M > 1 << 24 and N * M // 2 < 1 << 24
    pose, alt, gr = H.track(N, M, 0, seed=3)
    raw = np.random.default_rng(11).random((N, M)) * 200.0 + 1.0
    ctx.loaded = "big"
    ctx.frame_set(3, raw, N, M, pose, alt, gr)
    ctx.extract(3)
    one = capi.MosaicParams(-5000.0, -5000.0, 10000.0, 1, 1, 0, 0)
    for f in (ctx.mosaic_render, ctx.mosaic_consistency):
        with pytest.raises(capi.DsssError) as ei:
            f([3], one)
        assert ei.value.code == E_CAPACITY
    two = capi.MosaicParams(pose[N // 2, 3] - 10000.0, -5000.0, 10000.0, 2, 1, 0, 0)      # the track's middle ping sits on the edge between the cells
    s, c, img = ctx.mosaic_render([3], two)
    norm = orc.normalize(raw)
    print("two cells: counts %s, sums %s" % (c.ravel().tolist(), s.ravel().tolist()))
    assert int(c.sum(dtype=np.int64)) == N * M and int(c.max()) <= 1 << 24 and int(c.min()) > 1 << 22
    assert int(s.sum(dtype=np.int64)) == int(norm.sum(dtype=np.int64))
    assert (img.astype(np.int64) == (s.astype(np.int64) + c // 2) // c).all()

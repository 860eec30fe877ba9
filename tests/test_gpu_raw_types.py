"""GPU: raw waterfalls of u8, u16 and f32 samples next to f64.  A typed frame gives bit for bit what the f64 path gives for the same
samples widened to double -- every stage against the oracle on the widened frame AND against the device's own f64 path -- from every
residence (borrowed device pointer at every element alignment, pageable host, page-locked host streamed in by the extraction), in
batches that mix types and geometries, through the eager start of dsss_frames_set and its fall-backs, and when a frame is set again
with another type.  Frames and cases: tests/raw_types_ref.py (tests/test_raw_types_cpu.py holds them to their preconditions).
No tolerance anywhere: every widening is exact."""
import os

import numpy as np
import pytest

from tests import extract_shapes_ref as X
from tests import raw_types_ref as R

pytestmark = pytest.mark.gpu

FIELDS = ("x", "y", "size", "angle", "response", "octave")
E_ARG, E_STATE = -2, -4
NONE, BORROWED, OWNED, PENDING = 0, 1, 2, 3


@pytest.fixture(scope="module")
def ctx():
    from diasss_amd import capi
    c = capi.Context(max_frames=12)
    yield c
    c.close()


class _params:
    """the context under the parameter dicts `mask` and `orb`, the defaults again on the way out"""

    def __init__(self, ctx, mask, orb):
        self.ctx, self.mask, self.orb = ctx, mask, orb

    def __enter__(self):
        mp, op = X.device_params(self.ctx, self.mask, self.orb)
        self.ctx.set_params(mask=mp, orb=op)

    def __exit__(self, *exc):
        mp, op, _, _ = self.ctx.default_params()
        self.ctx.set_params(mask=mp, orb=op)


class _env:
    def __init__(self, k, v): self.k, self.v = k, v
    def __enter__(self): self.old = os.environ.get(self.k); os.environ[self.k] = self.v
    def __exit__(self, *exc):
        if self.old is None: os.environ.pop(self.k, None)
        else: os.environ[self.k] = self.old


def _images(ctx, fid, N, M, nlevels):
    """norm, mask and every pyramid level as bytes"""
    norm, mask = ctx.frame_norm(fid, N, M)
    return [norm.tobytes(), mask.tobytes()] + [ctx.frame_level(fid, l, N, M).tobytes() for l in range(nlevels)]


def _features(ctx, fid):
    return [np.asarray(a).tobytes() for a in ctx.features_get(fid)]


def _taps(ctx, fid, nlevels):
    return [a.tobytes() for l in range(nlevels) for a in ctx.frame_candidates(fid, l)]


def _check_oracle(ctx, orc, fid, ref, pose, gr, what, taps=True):
    N, M = ref["norm"].shape
    norm, mask = ctx.frame_norm(fid, N, M)
    assert (norm == ref["norm"]).all(), "%s: normalised image differs at %d pixels" % (what, int((norm != ref["norm"]).sum()))
    assert (mask == ref["mask"]).all(), "%s: filter mask differs at %d pixels" % (what, int((mask != ref["mask"]).sum()))
    for l, lv in enumerate(ref["levels"]):
        g = ctx.frame_level(fid, l, lv.shape[0], lv.shape[1])
        assert g.shape == lv.shape and (g == lv).all(), "%s: pyramid level %d differs" % (what, l)
    if taps:
        for l, (xs, ys, rs) in enumerate(ref["cands"]):
            gx, gy, gr_ = ctx.frame_candidates(fid, l)
            assert len(gx) == len(xs) and (gx == xs).all() and (gy == ys).all() and (gr_ == rs).all(), "%s: candidates of level %d differ" % (what, l)
    kps, desc = ref["kps"], ref["desc"]
    g_kps, g_desc, g_geo = ctx.features_get(fid)
    assert len(g_kps) == len(kps), "%s: %d keypoints, the oracle %d" % (what, len(g_kps), len(kps))
    for fld in FIELDS:
        assert (g_kps[fld] == kps[fld]).all(), "%s: keypoint field %s differs" % (what, fld)
    assert (g_desc == desc).all(), "%s: descriptors differ" % (what,)
    assert (np.asarray(g_geo).reshape(-1, 2) == orc.geo_at_kps(pose, gr, M, kps)).all(), "%s: geo samples differ" % (what,)


def _device(q, t):
    """(tensor, raw_type keyword) of a frame in HBM.  torch has no uint16 arithmetic on every build: the u16 image travels in int16
    storage with its type given explicitly"""
    import torch
    if t == "u16":
        return torch.from_numpy(q.view(np.int16)).cuda(), R.RAW_U16
    return torch.from_numpy(q).cuda(), None


def _pinned(q, t):
    import torch
    a = torch.from_numpy(q.view(np.int16) if t == "u16" else q).pin_memory()
    assert a.is_pinned()
    return a, (R.RAW_U16 if t == "u16" else None)


# ---------------------------------------------------------------- stage parity
@pytest.mark.parametrize("t", R.NARROW)
@pytest.mark.parametrize("kind", R.KINDS)
def test_stage_parity_with_the_oracle_and_the_f64_path(ctx, orc, kind, t):
    """norm, mask, every level, the candidates and the features of a typed frame: the oracle's on the widened frame, and byte for byte
    the device's own f64 path on the widened frame"""
    for shape in R.SHAPES:
        N, M, nl, _ = shape
        q, w, orb, ref = R.case(orc, kind, t, shape)
        pose, alt, gr = X.dr_inputs(N, M)
        what = "%s %s %d x %d" % (kind, t, N, M)
        with _params(ctx, R.MASK, orb):
            ctx.frame_set(0, q, N, M, pose, alt, gr)
            assert ctx.frame_raw_info(0) == (R.RAW_TYPE[t], OWNED, N * M * R.ESIZE[t])
            assert ctx.extract(0) == len(ref["kps"]), what
            _check_oracle(ctx, orc, 0, ref, pose, gr, what)
            typed = _images(ctx, 0, N, M, nl) + _taps(ctx, 0, nl) + _features(ctx, 0)
            ctx.frame_set(1, w, N, M, pose, alt, gr)
            assert ctx.frame_raw_info(1) == (R.RAW_F64, OWNED, N * M * 8)
            ctx.extract(1)
            assert typed == _images(ctx, 1, N, M, nl) + _taps(ctx, 1, nl) + _features(ctx, 1), what + ": differs from the f64 path"


# ---------------------------------------------------------------- dsss_frame_raw_stats
def _stats_of(ctx, fid, q, raw_type=None):
    N, M = q.shape
    pose, alt, gr = X.dr_inputs(N, M)
    ctx.frame_set(fid, q, N, M, pose, alt, gr, raw_type=raw_type)
    return ctx.frame_raw_stats(fid)


@pytest.mark.parametrize("t", ("f64",) + R.NARROW)
def test_raw_stats_are_the_fixed_tree_mean_and_the_minimum(ctx, orc, t):
    for kind in R.KINDS:
        for N, M, _, _ in R.SHAPES:
            q = R.frame(kind, t, N, M); w = R.widen(q)
            mean, mn = _stats_of(ctx, 2, q)
            assert R.bits(mean, mn) == R.bits(orc.lib().orc_mean(orc.dp(w), N, M), w.min()), (kind, t, N, M, mean, mn)
            if t in R.INTEGER:
                assert R.bits(mean) == R.bits(R.exact_mean(q)), (kind, t, N, M)


def test_raw_stats_of_the_largest_row_sums(ctx, orc):
    """all 65535 in u16 and all 255 in u8 at 69 x 2000: the largest row sums the small shapes reach (131 070 000: past 2^24, so past
    what a float or a 16-bit lane count would hold)"""
    for t, top in (("u16", 65535), ("u8", 255)):
        q = np.full((69, 2000), top, R.DTYPES[t])
        assert R.bits(*_stats_of(ctx, 2, q)) == R.bits(float(top), float(top)) == R.bits(R.exact_mean(q), float(top))
        q[68, 1999] = 0; q[0, 0] = 1
        w = R.widen(q)
        assert R.bits(*_stats_of(ctx, 2, q)) == R.bits(orc.lib().orc_mean(orc.dp(w), 69, 2000), 0.0) == R.bits(R.exact_mean(q), 0.0)


@pytest.mark.parametrize("special", ("nan", "inf"))
def test_raw_stats_of_f32_non_finite_samples_are_the_f64_paths(ctx, special):
    """one NaN, or one +inf, in an f32 frame: mean and minimum are those of the f64 path on the widened frame, non-finite pattern included"""
    for N, M, _, _ in R.SHAPES[:3]:
        q = R.frame("speckle", "f32", N, M).copy()
        q[N // 2, M // 3] = np.float32(special)
        a = _stats_of(ctx, 2, q); b = _stats_of(ctx, 3, R.widen(q))
        assert R.bits(*a) == R.bits(*b), (special, N, M, a, b)
        assert (np.isnan(a[0]) if special == "nan" else a[0] == np.inf) and np.isfinite(a[1])


# ---------------------------------------------------------------- residency
@pytest.mark.parametrize("t", R.NARROW + ("f64",))
def test_every_residence_of_a_typed_image(ctx, orc, t):
    """a borrowed device tensor, a pageable numpy array (copied by dsss_frame_set) and page-locked tensors (twelve frames streamed in by
    dsss_extract_many in three upload batches of four): dsss_frame_raw_info says where the image lives at every point, and the results
    are the oracle's"""
    from diasss_amd.capi import DsssError
    orb = R.orb(1, 60)
    shapes = [(69, 70), (70, 74)]
    frames = [R.quantise(R.shadows(X.speckle(*shapes[k % 2], 300 + k), k) if t == "f32" else X.speckle(*shapes[k % 2], 300 + k), t) for k in range(12)]
    refs = [X.oracle_stages(orc, R.widen(q), R.MASK, orb, key=("raw_res", t, k)) for k, q in enumerate(frames)]
    dr = [X.dr_inputs(*q.shape) for q in frames]
    es = R.ESIZE[t]
    with _params(ctx, R.MASK, orb):
        for k in (0, 1):
            q = frames[k]; N, M = q.shape
            dev, rt = _device(q, t)
            ctx.frame_set(k, dev, N, M, *dr[k], raw_type=rt)
            assert ctx.frame_raw_info(k) == (R.RAW_TYPE[t], BORROWED, 0)
            ctx.extract(k)
            _check_oracle(ctx, orc, k, refs[k], dr[k][0], dr[k][2], "%s device tensor %d" % (t, k))
            ctx.frame_set(k, q, N, M, *dr[k])
            assert ctx.frame_raw_info(k) == (R.RAW_TYPE[t], OWNED, N * M * es)
            ctx.extract(k)
            _check_oracle(ctx, orc, k, refs[k], dr[k][0], dr[k][2], "%s pageable array %d" % (t, k))
        pinned = [_pinned(q, t) for q in frames]
        with _env("DSSS_EX_UPLOAD_BATCH", "4"):
            for k, q in enumerate(frames):
                ctx.frame_set(k, pinned[k][0], q.shape[0], q.shape[1], *dr[k], raw_type=pinned[k][1])
            for k, q in enumerate(frames):
                assert ctx.frame_raw_info(k) == (R.RAW_TYPE[t], PENDING, q.size * es)
            with pytest.raises(DsssError) as ei:
                ctx.frame_raw_stats(5)
            assert ei.value.code == E_STATE
            ctx.extract_many(list(range(12)))
        for k, q in enumerate(frames):
            assert ctx.frame_raw_info(k) == (R.RAW_TYPE[t], OWNED, q.size * es)
            _check_oracle(ctx, orc, k, refs[k], dr[k][0], dr[k][2], "%s page-locked frame %d" % (t, k), taps=False)
        w = R.widen(frames[7])
        assert R.bits(*ctx.frame_raw_stats(7)) == R.bits(orc.lib().orc_mean(orc.dp(w), *w.shape), w.min())


# ---------------------------------------------------------------- alignment
@pytest.mark.parametrize("t", R.NARROW + ("f64",))
def test_borrowed_pointer_at_every_element_alignment(ctx, orc, t):
    """a device image one element past a 256-byte aligned allocation, and at 4, 8 and 12 (mod 16) where the element allows it: the
    16-byte loads of the row reduce start behind a head of their own per row (M = 74), normalize_kernel takes the element loads"""
    import torch
    shape = R.SHAPES[1]
    N, M, nl, _ = shape
    assert (M * R.ESIZE["u8"]) % 16 and (M * R.ESIZE["u16"]) % 16
    q, w, orb, ref = R.case(orc, "speckle", t, shape)
    pose, alt, gr = X.dr_inputs(N, M)
    es = R.ESIZE[t]; nbytes = N * M * es
    tdt = {"f64": torch.float64, "f32": torch.float32, "u16": torch.int16, "u8": torch.uint8}[t]
    rt = R.RAW_U16 if t == "u16" else None
    buf = torch.zeros(nbytes + 64, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    src = torch.from_numpy(q.view(np.uint8).reshape(-1)).cuda()
    outs = []
    with _params(ctx, R.MASK, orb):
        for off in sorted({0, es, 4, 8, 12}):
            if off % es: continue
            view = buf[off:off + nbytes]
            view.copy_(src)
            img = view.view(tdt).view(N, M)
            assert img.data_ptr() % 16 == off % 16 and img.is_contiguous()
            ctx.frame_set(0, img, N, M, pose, alt, gr, raw_type=rt)
            assert ctx.frame_raw_info(0) == (R.RAW_TYPE[t], BORROWED, 0)
            ctx.extract(0)
            _check_oracle(ctx, orc, 0, ref, pose, gr, "%s image at %d (mod 16)" % (t, off))
            outs.append(_images(ctx, 0, N, M, nl) + _taps(ctx, 0, nl) + _features(ctx, 0))
            assert R.bits(*ctx.frame_raw_stats(0)) == R.bits(orc.lib().orc_mean(orc.dp(w), N, M), w.min()), (t, off)
    assert len(outs) >= 2 and all(o == outs[0] for o in outs)


# ---------------------------------------------------------------- mixed batch
def test_mixed_types_in_one_frames_set(ctx, orc):
    """eight frames, f64 u8 u16 f32 u8 f64 f32 u16, of two geometries in ONE dsss_frames_set: the eager start and dsss_extract_many, then
    the fall-backs (another list order, parameters changed after the start, the frames set twice, a single-frame extraction in
    between).  Every frame equals its own single-frame result under the parameters in force, and the oracle's"""
    frames = R.mixed_frames()
    ids = list(range(8))
    orb_a, orb_b = R.orb(1, 60), R.orb(1, 40)
    dr = [X.dr_inputs(*q.shape) for q, _ in frames]
    dev = [_device(q, t) for (q, _), t in zip(frames, R.MIXED_ORDER)]
    assert len({q.shape for q, _ in frames}) == 2

    def set_all():
        ctx.frames_set(ids, [d for d, _ in dev], [q.shape[0] for q, _ in frames], [q.shape[1] for q, _ in frames],
                       [d[0] for d in dr], [d[1] for d in dr], [d[2] for d in dr], raw_types=[R.RAW_TYPE[t] for t in R.MIXED_ORDER])
        for k, t in enumerate(R.MIXED_ORDER):
            assert ctx.frame_raw_info(k) == (R.RAW_TYPE[t], BORROWED, 0)

    single = {}
    for name, orb in (("a", orb_a), ("b", orb_b)):
        with _params(ctx, R.MASK, orb):
            for k, (q, w) in enumerate(frames):
                ref = X.oracle_stages(orc, w, R.MASK, orb, key=("raw_mixed", name, k))
                ctx.frame_set(k, dev[k][0], q.shape[0], q.shape[1], *dr[k], raw_type=dev[k][1])
                ctx.extract(k)
                _check_oracle(ctx, orc, k, ref, dr[k][0], dr[k][2], "frame %d (%s) alone, parameters %s" % (k, R.MIXED_ORDER[k], name))
                single[name, k] = _images(ctx, k, q.shape[0], q.shape[1], 1) + _features(ctx, k)

    def check(name, what):
        for k, (q, _) in enumerate(frames):
            assert _images(ctx, k, q.shape[0], q.shape[1], 1) + _features(ctx, k) == single[name, k], "frame %d (%s): %s" % (k, R.MIXED_ORDER[k], what)

    with _params(ctx, R.MASK, orb_a):
        set_all(); ctx.extract_many(ids); check("a", "eager start, then extract_many")
        set_all(); ctx.extract_many([5, 2, 7, 0, 3, 6, 1, 4]); check("a", "another list order")
        set_all(); set_all(); ctx.extract_many(ids); check("a", "set twice")
        set_all(); assert ctx.extract(3) > 0; ctx.extract_many(ids); check("a", "a single-frame extraction in between")
        set_all()
        mp, op = X.device_params(ctx, R.MASK, orb_b)
        ctx.set_params(mask=mp, orb=op)
        ctx.extract_many(ids); check("b", "parameters changed after the start")
    with _params(ctx, R.MASK, orb_a):
        # the same list from host memory: no eager start, one batch that holds all four types
        ctx.frames_set(ids, [q for q, _ in frames], [q.shape[0] for q, _ in frames], [q.shape[1] for q, _ in frames],
                       [d[0] for d in dr], [d[1] for d in dr], [d[2] for d in dr])
        for k, ((q, _), t) in enumerate(zip(frames, R.MIXED_ORDER)):
            assert ctx.frame_raw_info(k) == (R.RAW_TYPE[t], OWNED, q.size * R.ESIZE[t])
        ctx.extract_many(ids); check("a", "pageable host images, types from the dtypes")


# ---------------------------------------------------------------- the same frame set again with another type
def test_frame_set_again_with_another_type(ctx, orc):
    """u8, then f64, then u16 on one id with one geometry, an extraction after each: the owned copy follows the type (the f64 image is
    eight times the u8 one it replaces in the same block), then another geometry with another type"""
    shape = R.SHAPES[3]
    N, M, nl, _ = shape
    pose, alt, gr = X.dr_inputs(N, M)
    with _params(ctx, R.MASK, R.orb(nl, 60)):
        for t in ("u8", "f64", "u16", "u8"):
            q, w, orb, ref = R.case(orc, "speckle", t, shape)
            ctx.frame_set(4, q, N, M, pose, alt, gr)
            assert ctx.frame_raw_info(4) == (R.RAW_TYPE[t], OWNED, N * M * R.ESIZE[t])
            ctx.extract(4)
            _check_oracle(ctx, orc, 4, ref, pose, gr, "%s after another type" % t)
            assert R.bits(*ctx.frame_raw_stats(4)) == R.bits(orc.lib().orc_mean(orc.dp(w), N, M), w.min())
        shape2 = R.SHAPES[5]
        N2, M2, _, _ = shape2
        q, w, orb, ref = R.case(orc, "flat_with_hot", "f32", shape2)
        dr2 = X.dr_inputs(N2, M2)
        ctx.frame_set(4, q, N2, M2, *dr2)
        assert ctx.frame_raw_info(4) == (R.RAW_F32, OWNED, N2 * M2 * 4)
        ctx.extract(4)
        _check_oracle(ctx, orc, 4, ref, dr2[0], dr2[2], "another geometry and another type")


# ---------------------------------------------------------------- end to end
def test_u16_survey_through_the_pipeline(orc):
    """a 4-frame synthetic survey recorded as u16 through Pipeline.run: poses and LM statistics identical to the run on the widened f64
    frames -- from level 0 on the two are the same computation"""
    import torch
    from diasss_amd import pipeline, synth
    S = synth.Survey(4, 600, 256, tile=512)
    u16 = [S.frame(f, "uint16") for f in range(4)]
    assert all(a.dtype == torch.uint16 for a in u16)
    wide = [a.to(torch.float64) for a in u16]
    ins = [S.inputs(f) for f in range(4)]
    out = []
    for raws in (u16, wide):
        p = pipeline.Pipeline(4)
        try:
            poses, stats = p.run(raws, [i[0] for i in ins], [i[1] for i in ins], [i[2] for i in ins])
            out.append((np.array(poses, copy=True), stats, [p.ctx.frame_raw_info(f)[0] for f in range(4)], [_features(p.ctx, f) for f in range(4)]))
        finally:
            p.close()
    assert out[0][2] == [R.RAW_U16] * 4 and out[1][2] == [R.RAW_F64] * 4
    assert out[0][3] == out[1][3]
    assert out[0][0].tobytes() == out[1][0].tobytes() and np.isfinite(out[0][0]).all()
    assert repr(out[0][1]) == repr(out[1][1]), (out[0][1], out[1][1])


# ---------------------------------------------------------------- argument checks
def test_unknown_type_is_refused_before_anything_is_touched(ctx, orc):
    from diasss_amd.capi import DsssError, _ptr
    shape = R.SHAPES[0]
    N, M, nl, _ = shape
    q, w, orb, ref = R.case(orc, "speckle", "u8", shape)
    pose, alt, gr = X.dr_inputs(N, M)
    other = np.zeros((80, 96), np.float32)
    with _params(ctx, R.MASK, orb):
        for fid in (6, 7):
            ctx.frame_set(fid, q, N, M, pose, alt, gr)
        before = [ctx.frame_raw_info(f) for f in (6, 7)]
        assert before == [(R.RAW_U8, OWNED, N * M)] * 2
        for bad in (4, -1, 255):
            rc = ctx.L.dsss_frame_set_typed(ctx.h, 6, _ptr(other), bad, 80, 96, _ptr(np.zeros((80, 6))), _ptr(np.zeros(80)), _ptr(np.zeros(48)))
            assert rc == E_ARG
        # one call for both frames in which the SECOND frame's type is bad: the first must not have been touched either
        a = ctx.frames_args([6, 7], [other, other], [80, 80], [96, 96], [np.zeros((80, 6))] * 2, [np.zeros(80)] * 2, [np.zeros(48)] * 2)
        a.raw_type[1] = 9
        with pytest.raises(DsssError) as ei:
            ctx.frames_set(a)
        assert ei.value.code == E_ARG
        assert [ctx.frame_raw_info(f) for f in (6, 7)] == before
        for fid in (6, 7):
            ctx.extract(fid)
            _check_oracle(ctx, orc, fid, ref, pose, gr, "frame %d after the refused calls" % fid)


def test_raw_stats_needs_an_image_on_the_device(ctx):
    from diasss_amd.capi import DsssError
    N, M = 69, 70
    pose, alt, gr = X.dr_inputs(N, M)
    ctx.frame_set(9, None, N, M, pose, alt, gr)                      # geometry only
    assert ctx.frame_raw_info(9)[1:] == (NONE, 0)
    with pytest.raises(DsssError) as ei:
        ctx.frame_raw_stats(9)
    assert ei.value.code == E_STATE
    pin, _ = _pinned(R.frame("speckle", "u8", N, M), "u8")
    ctx.frame_set(9, pin, N, M, pose, alt, gr)
    assert ctx.frame_raw_info(9) == (R.RAW_U8, PENDING, N * M)
    with pytest.raises(DsssError) as ei:
        ctx.frame_raw_stats(9)
    assert ei.value.code == E_STATE
    with pytest.raises(DsssError) as ei:
        ctx.frame_raw_stats(12)
    assert ei.value.code == E_ARG

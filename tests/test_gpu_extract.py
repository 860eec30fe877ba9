"""GPU parity: preprocessing + ORB extraction kernels against the CPU oracle, stage by stage, bit-exact."""
import ctypes as C
import numpy as np
import pytest

from tests.helpers import survey_frame as _frame

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from diasss_amd import capi
    c = capi.Context(max_frames=4)
    yield c
    c.close()


@pytest.mark.parametrize("N,M,seed", [(640, 400, 3), (500, 700, 4), (1000, 512, 5)])
def test_extract_stage_parity(ctx, orc, N, M, seed):
    raw, pose, alt, gr = _frame(N, M, seed)
    ctx.frame_set(0, raw, N, M, pose, alt, gr)
    n = ctx.extract(0)
    # K1: normalised image + mask
    norm, mask = ctx.frame_norm(0, N, M)
    o_norm = orc.normalize(raw); o_mask = orc.mask(raw)
    assert (norm == o_norm).all(), "normalised image differs"
    assert (mask == o_mask).all(), "filter mask differs"
    # K2: pyramid
    p = orc.orb_params()
    lr = (C.c_int * 8)(); lc = (C.c_int * 8)()
    orc.lib().orc_orb_level_sizes(N, M, C.byref(p), lr, lc)
    prev = o_norm
    levels = [o_norm]
    for l in range(1, 6):
        dst = np.zeros((lr[l], lc[l]), np.uint8)
        orc.lib().orc_resize_linear_u8(orc.u8(prev), prev.shape[0], prev.shape[1], orc.u8(dst), lr[l], lc[l])
        g = ctx.frame_level(0, l, lr[l], lc[l])
        assert g.shape == dst.shape and (g == dst).all(), "pyramid level %d differs" % l
        prev = dst; levels.append(dst)
    # K3: FAST candidates per level, reference order
    for l in range(6):
        cap = 200000
        xs = np.zeros(cap, np.float32); ys = np.zeros(cap, np.float32); rs = np.zeros(cap, np.float32)
        k = orc.lib().orc_fast_level(orc.u8(levels[l]), lr[l], lc[l], 12, 7, orc.fp(xs), orc.fp(ys), orc.fp(rs), cap)
        gx, gy, gr_ = ctx.frame_candidates(0, l)
        assert len(gx) == k, "level %d: %d candidates vs oracle %d" % (l, len(gx), k)
        assert (gx == xs[:k]).all() and (gy == ys[:k]).all() and (gr_ == rs[:k]).all()
    # K4-K7 + mask filter: final features
    kps, desc, norm2, mask2 = orc.detect_feature(raw)
    g_kps, g_desc, g_geo = ctx.features_get(0)
    assert n == len(kps) == len(g_kps)
    for fld in ("x", "y", "size", "angle", "response", "octave"):
        assert (g_kps[fld] == kps[fld]).all(), "keypoint field %s differs" % fld
    assert (g_desc == desc).all(), "descriptors differ"
    assert (g_geo == orc.geo_at_kps(pose, gr, M, kps)).all()
    assert n > 200


def test_extract_small_orb_config_and_reuse(ctx, orc):
    """non-default ORB parameters (nfeatures 500, 4 levels) and context reuse with a different frame size"""
    N, M = 640, 400
    raw, pose, alt, gr = _frame(N, M, 9, hot=False)
    mp, op, mt, pg = ctx.default_params()
    op.nfeatures = 500; op.nlevels = 4
    ctx.set_params(orb=op)
    ctx.frame_set(1, raw, N, M, pose, alt, gr)
    n = ctx.extract(1)
    po = orc.orb_params(); po.nfeatures = 500; po.nlevels = 4
    kps, desc, _, _ = orc.detect_feature(raw, None, po)
    g_kps, g_desc, _ = ctx.features_get(1)
    assert n == len(kps) and (g_desc == desc).all() and (g_kps["x"] == kps["x"]).all() and (g_kps["angle"] == kps["angle"]).all()
    dp = ctx.default_params()[1]
    ctx.set_params(orb=dp)


@pytest.mark.parametrize("scale,N,M", [(2.0, 1000, 802), (1.5, 801, 598), (1.1, 501, 334)])
def test_extract_other_scale_factors(ctx, orc, scale, N, M):
    """pyramid scale factors other than 1.2 and odd sizes: at 2.0 and 1.5 the source bytes of four output pixels do not fit the
    12-byte windows of resize_strip_kernel and the flat form (resize_kernel) runs; every level must match the oracle's byte for byte"""
    raw, pose, alt, gr = _frame(N, M, 11, hot=False)
    mp, op, mt, pg = ctx.default_params()
    op.nfeatures = 600; op.nlevels = 4; op.scale = scale
    ctx.set_params(orb=op)
    try:
        ctx.frame_set(2, raw, N, M, pose, alt, gr)
        n = ctx.extract(2)
        po = orc.orb_params(); po.nfeatures = 600; po.nlevels = 4; po.scale = scale
        kps, desc, _, _ = orc.detect_feature(raw, None, po)
        g_kps, g_desc, _ = ctx.features_get(2)
        assert n == len(kps) and n > 50
        for fld in ("x", "y", "octave", "angle", "response"):
            assert (g_kps[fld] == kps[fld]).all(), fld
        assert (g_desc == desc).all()
    finally:
        ctx.set_params(orb=ctx.default_params()[1])


def test_resize_strips_and_flat_form_in_one_batch(ctx, orc):
    """at a scale of 1.334 the 12-byte windows fit the 500 x 300 frame's first level (resize_strip_kernel) and do not fit the
    500 x 302 frame's (resize_kernel, which then skips the frames the strips did): both in ONE extract_many, every keypoint and
    descriptor as the oracle's"""
    mp, op, mt, pg = ctx.default_params()
    op.nfeatures = 500; op.nlevels = 4; op.scale = 1.334
    ctx.set_params(orb=op)
    try:
        frames = [_frame(500, M, 21 + i, hot=False) for i, M in enumerate((300, 302))]
        for i, (raw, pose, alt, gr) in enumerate(frames): ctx.frame_set(i, raw, 500, raw.shape[1], pose, alt, gr)
        ctx.extract_many([0, 1])
        po = orc.orb_params(); po.nfeatures = 500; po.nlevels = 4; po.scale = 1.334
        for i, (raw, pose, alt, gr) in enumerate(frames):
            kps, desc, _, _ = orc.detect_feature(raw, None, po)
            g_kps, g_desc, _ = ctx.features_get(i)
            assert len(g_kps) == len(kps) and len(kps) > 50
            for fld in ("x", "y", "octave", "angle", "response"):
                assert (g_kps[fld] == kps[fld]).all(), (i, fld)
            assert (g_desc == desc).all()
    finally:
        ctx.set_params(orb=ctx.default_params()[1])


def test_extract_device_resident_input(ctx, orc):
    """raw image handed over as a device pointer (torch tensor in HBM): same result, no host copy"""
    import torch
    N, M = 640, 400
    raw, pose, alt, gr = _frame(N, M, 12, hot=False)
    t = torch.from_numpy(raw).cuda()
    ctx.frame_set(2, t, N, M, pose, alt, gr)
    n = ctx.extract(2)
    kps, desc, _, _ = orc.detect_feature(raw)
    g_kps, g_desc, _ = ctx.features_get(2)
    assert n == len(kps) and (g_desc == desc).all()


def test_eager_extraction_started_by_frames_set_and_its_fallbacks(ctx, orc):
    """dsss_frames_set starts the extraction of device-resident frames (as the reference's Frame constructor runs DetectFeature);
    dsss_extract_many over the same list only finishes it.  Whatever happens in between -- another list of frames, parameters changed,
    frames set again -- the features must be those of the oracle for the parameters in force at the extraction."""
    import torch
    N, M = 640, 400
    frames = [_frame(N, M, 20 + k, hot=(k == 0)) for k in range(3)]
    dev = [torch.from_numpy(f[0]).cuda() for f in frames]
    ids = [0, 1, 2]

    def set_all():
        ctx.frames_set(ids, dev, [N] * 3, [M] * 3, [f[1] for f in frames], [f[2] for f in frames], [f[3] for f in frames])

    def check(po=None):
        for k in ids:
            kps, desc, _, _ = orc.detect_feature(frames[k][0], None, po) if po is not None else orc.detect_feature(frames[k][0])
            g_kps, g_desc, g_geo = ctx.features_get(k)
            assert len(g_kps) == len(kps) and (g_desc == desc).all() and (g_kps["x"] == kps["x"]).all() and (g_kps["angle"] == kps["angle"]).all()
            ref_geo = orc.geo_at_kps(frames[k][1], frames[k][3], M, kps)
            assert (np.asarray(g_geo).reshape(-1, 2) == np.asarray(ref_geo).reshape(-1, 2)).all()       # the one kernel that waits for the geometry upload

    set_all(); ctx.extract_many(ids); check()                                   # the plain pair: only the tail runs in extract_many
    set_all(); ctx.extract_many([2, 0, 1]); check()                             # another order: the started extraction is dropped, all of it runs again
    set_all(); set_all(); ctx.extract_many(ids); check()                        # set twice: the second start is the one that counts
    mp, op, mt, pg = ctx.default_params()
    op.nfeatures = 500; op.nlevels = 4
    try:
        set_all(); ctx.set_params(orb=op); ctx.extract_many(ids)                # parameters changed after the start: extracted with the NEW ones
        po = orc.orb_params(); po.nfeatures = 500; po.nlevels = 4
        check(po)
    finally:
        ctx.set_params(orb=ctx.default_params()[1])
    set_all(); assert ctx.extract(1) > 0; ctx.extract_many(ids); check()        # a single-frame extraction in between


E_ARG, E_STATE = -2, -4
FIELDS = ("x", "y", "size", "angle", "response", "octave")


def _assert_oracle(ctx, orc, fid, frame, po=None):
    """keypoints, descriptors and geo of frame `fid` are bit for bit the oracle's"""
    raw, pose, alt, gr = frame
    kps, desc, _, _ = orc.detect_feature(raw, None, po) if po is not None else orc.detect_feature(raw)
    g_kps, g_desc, g_geo = ctx.features_get(fid)
    assert len(g_kps) == len(kps) and len(kps) > 50
    for fld in FIELDS:
        assert (g_kps[fld] == kps[fld]).all(), (fid, fld)
    assert (g_desc == desc).all(), fid
    assert (np.asarray(g_geo).reshape(-1, 2) == np.asarray(orc.geo_at_kps(pose, gr, raw.shape[1], kps)).reshape(-1, 2)).all(), fid


def _set_many(ctx, ids, frames, raws):
    ctx.frames_set(ids, raws, [f[0].shape[0] for f in frames], [f[0].shape[1] for f in frames], [f[1] for f in frames], [f[2] for f in frames], [f[3] for f in frames])


def test_ragged_eager_start_equals_oracle_and_whole_run(ctx, orc):
    """three device-resident frames of three geometries, both resize kernels in the started half (scale 1.334: strips fit 500 x 300, not
    500 x 302): dsss_frames_set starts, dsss_extract_many resumes -- the oracle's features, and those of the whole-run path bit for bit"""
    import torch
    mp, op, mt, pg = ctx.default_params()
    op.nfeatures = 500; op.nlevels = 4; op.scale = 1.334
    ctx.set_params(orb=op)
    try:
        frames = [_frame(N, M, 31 + i, hot=False) for i, (N, M) in enumerate(((500, 300), (500, 302), (640, 400)))]
        dev = [torch.from_numpy(f[0]).cuda() for f in frames]
        ids = [0, 1, 2]
        _set_many(ctx, ids, frames, dev)
        ctx.extract_many(ids)                                                       # start + resume
        po = orc.orb_params(); po.nfeatures = 500; po.nlevels = 4; po.scale = 1.334
        split = []
        for k in ids:
            _assert_oracle(ctx, orc, k, frames[k], po)
            split.append([np.asarray(a).tobytes() for a in ctx.features_get(k)])
        for k in ids:                                                               # the whole run, frame by frame
            raw, pose, alt, gr = frames[k]
            ctx.frame_set(k, dev[k], raw.shape[0], raw.shape[1], pose, alt, gr)
            assert ctx.extract(k) > 50
            assert [np.asarray(a).tobytes() for a in ctx.features_get(k)] == split[k], k
    finally:
        ctx.set_params(orb=ctx.default_params()[1])


def test_start_and_resume_issue_what_the_whole_run_issues(ctx):
    """the profile's launch counts and work figures of every extraction family are the same whether dsss_frames_set starts the
    extraction and dsss_extract_many resumes it, or dsss_extract_many runs all of it"""
    import torch
    N, M = 640, 400
    frames = [_frame(N, M, 40 + k, hot=False) for k in range(3)]
    dev = [torch.from_numpy(f[0]).cuda() for f in frames]
    ids = [0, 1, 2]
    families = ("row_reduce", "pre_misc", "normalize", "pyramid", "fast", "fast_compact", "quadtree", "desc", "filter", "sift")
    ctx.profile(True)
    try:
        ctx.profile_reset()
        _set_many(ctx, ids, frames, dev)
        ctx.extract_many(ids)
        split = ctx.profile_get()
        ctx.profile_reset()
        for k in ids: ctx.frame_set(k, dev[k], N, M, frames[k][1], frames[k][2], frames[k][3])
        ctx.extract_many(ids)
        whole = ctx.profile_get()
    finally:
        ctx.profile(False)
    for fam in families:
        print(fam, split[fam][1:], whole[fam][1:])
        assert split[fam][1] == whole[fam][1], "launches of %s: %d started + resumed, %d whole run" % (fam, split[fam][1], whole[fam][1])
        assert split[fam][2] == whole[fam][2], "work of %s: %r started + resumed, %r whole run" % (fam, split[fam][2], whole[fam][2])
    assert all(whole[fam][1] > 0 for fam in ("row_reduce", "pyramid", "fast", "quadtree", "desc", "filter"))


def test_error_exits_of_start_and_resume_leave_a_usable_context(ctx, orc):
    """host-side refusals (they return before any launch) on either side of an early start; the context extracts correctly afterwards"""
    import torch
    from diasss_amd.capi import DsssError
    N, M = 640, 400
    frames = [_frame(N, M, 50 + k, hot=False) for k in range(4)]
    dev = [torch.from_numpy(f[0]).cuda() for f in frames]
    ids = [0, 1, 2, 3]
    _set_many(ctx, ids, frames, [dev[0], None, dev[2], None])                       # two frames carry no image: the start covers the other two
    ctx.extract_many([0, 2])                                                        # (resume)
    for k in (0, 2): _assert_oracle(ctx, orc, k, frames[k])
    with pytest.raises(DsssError) as ei:
        ctx.extract_many(ids)
    assert ei.value.code == E_STATE and "no raw image" in str(ei.value)
    ctx.extract_many([0, 2])                                                        # (whole run)
    for k in (0, 2): _assert_oracle(ctx, orc, k, frames[k])
    # a frame too small for the top pyramid level: at eight levels and 1.2 the last one of 200 x 200 is 56 x 56, below 2 * 19 + 31 = 69
    mp, op, mt, pg = ctx.default_params()
    op.nlevels = 8
    assert round(200 / 1.2 ** 7) < 2 * 19 + 31 <= round(200 / 1.2 ** 5)                 # (the default six levels would fit)
    ctx.set_params(orb=op)
    try:
        small = _frame(200, 200, 60, hot=False)
        _set_many(ctx, [0], [small], [torch.from_numpy(small[0]).cuda()])           # succeeds: the early start declines silently
        with pytest.raises(DsssError) as ei:
            ctx.extract_many([0])
        assert ei.value.code == E_ARG and "too small" in str(ei.value)
    finally:
        ctx.set_params(orb=ctx.default_params()[1])
    _set_many(ctx, [0], [frames[1]], [dev[1]])
    ctx.extract_many([0])
    _assert_oracle(ctx, orc, 0, frames[1])


def test_full_geo_image_on_request(ctx, orc):
    """Frame::geo_img as the reference holds it (frame.cpp:126-165: the N x M pair) through dsss_frame_get_geo -- the hot path only
    ever uses its extremes (dsss_frame_bbox) and its samples at the keypoints; a caller that reads the field gets the full image,
    bit for bit the oracle's, and Util::ComputeIntersection sees the same extremes on either form"""
    from tests import helpers as H
    for leg, (N, M) in enumerate(((700, 480), (333, 130))):
        pose, alt, gr = H.track(N, M, leg, seed=9)
        raw = np.random.default_rng(leg).rayleigh(1.0, (N, M)) * 100.0
        ctx.frame_set(leg, raw, N, M, pose, alt, gr)
        gx, gy = ctx.frame_geo(leg, N, M)
        ox, oy = orc.geo_img(pose, gr, M)
        assert (gx == ox).all() and (gy == oy).all()
        bb = ctx.frame_bbox(leg)
        assert bb[0] == gx.min() and bb[1] == gx.max() and bb[2] == gy.min() and bb[3] == gy.max()

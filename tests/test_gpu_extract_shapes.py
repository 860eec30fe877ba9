"""GPU parity of the extraction kernels at small, wide and border-heavy frames: every stage bit for bit the oracle's, with the same
parameters, on the frames of tests/extract_shapes_ref.py (tests/test_extract_shapes_cpu.py holds each of them to the class it is named
for).  What the survey-sized tests of test_gpu_extract.py never read: the byte-wise reflect-101 patch of orient_desc_kernel, the retry of
fast_cells_kernel at minThFAST, more than one quadtree root, FAST windows of 30 to 59 px on one to three cells an axis under both LDS
strides, mask parameters other than the defaults, hot pixels at the image borders, one, two and eight pyramid levels, and a borrowed
device image that is only 8-byte aligned."""
import numpy as np
import pytest

from tests import extract_shapes_ref as X

pytestmark = pytest.mark.gpu

FIELDS = ("x", "y", "size", "angle", "response", "octave")


@pytest.fixture(scope="module")
def ctx():
    from diasss_amd import capi
    c = capi.Context(max_frames=4)
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


def _check_images(ctx, fid, ref, what):
    N, M = ref["norm"].shape
    norm, mask = ctx.frame_norm(fid, N, M)
    assert (norm == ref["norm"]).all(), "%s: normalised image differs" % (what,)
    assert (mask == ref["mask"]).all(), "%s: filter mask differs at %d pixels" % (what, int((mask != ref["mask"]).sum()))


def _check_stages(ctx, fid, ref, what):
    """norm, mask, every pyramid level and the candidates of every level in order (the taps of a single-frame extraction)"""
    _check_images(ctx, fid, ref, what)
    for l, lv in enumerate(ref["levels"]):
        g = ctx.frame_level(fid, l, lv.shape[0], lv.shape[1])
        assert g.shape == lv.shape and (g == lv).all(), "%s: pyramid level %d differs" % (what, l)
    for l, (xs, ys, rs) in enumerate(ref["cands"]):
        gx, gy, gr = ctx.frame_candidates(fid, l)
        assert len(gx) == len(xs), "%s: level %d has %d candidates, the oracle %d" % (what, l, len(gx), len(xs))
        assert (gx == xs).all() and (gy == ys).all() and (gr == rs).all(), "%s: candidates of level %d differ" % (what, l)


def _check_features(ctx, orc, fid, ref, pose, gr, what, sel=None):
    """final keypoints in order, descriptors and geo samples; sel: a boolean pick of the oracle's keypoints (the counts are compared first)"""
    kps, desc = ref["kps"], ref["desc"]
    g_kps, g_desc, g_geo = ctx.features_get(fid, cap=max(16384, len(kps) + 64))
    assert len(g_kps) == len(kps), "%s: %d keypoints, the oracle %d" % (what, len(g_kps), len(kps))
    s = slice(None) if sel is None else sel
    for fld in FIELDS:
        assert (g_kps[fld][s] == kps[fld][s]).all(), "%s: keypoint field %s differs" % (what, fld)
    assert (g_desc[s] == desc[s]).all(), "%s: descriptors differ" % (what,)
    geo = orc.geo_at_kps(pose, gr, ref["norm"].shape[1], kps)
    assert (np.asarray(g_geo).reshape(-1, 2)[s] == geo[s]).all(), "%s: geo samples differ" % (what,)


def _run(ctx, orc, fid, raw, ref, what, image=None):
    N, M = raw.shape
    pose, alt, gr = X.dr_inputs(N, M)
    ctx.frame_set(fid, raw if image is None else image, N, M, pose, alt, gr)
    n = ctx.extract(fid)
    assert n == len(ref["kps"]), "%s: %d keypoints, the oracle %d" % (what, n, len(ref["kps"]))
    _check_stages(ctx, fid, ref, what)
    _check_features(ctx, orc, fid, ref, pose, gr, what)
    return pose, gr


@pytest.mark.parametrize("rows", X.SMALL_ROWS + (100,))
def test_small_frame_cell_classes(ctx, orc, rows):
    """one to three FAST cells an axis, windows from 30 to 59 px, max_cw of 40 (fast_cells_kernel<40>) and above (<68>), one pyramid level
    (and two for the 59-px window across a 91-px level): dpr, mg, mg_g, the overrun dwords at the image end, the zero border of A"""
    for r, c, nl, sc in X.SMALL_SHAPES:
        if r != rows: continue
        raw, orb, ref = X.small_case(orc, r, c, nl, sc)
        with _params(ctx, X.SMALL_MASK, orb):
            _run(ctx, orc, 0, raw, ref, "%d x %d %s" % (r, c, X.shape_class(orc, r, c, nl, sc)))


@pytest.mark.parametrize("shape", X.PYRAMID_SHAPES, ids=lambda s: "%dx%d@%g" % (s[0], s[1], s[3]))
def test_pyramid_levels_of_the_flat_resize(ctx, orc, shape):
    """three levels at scale 2.0, 1.5 and 1.334 on the smallest frames whose top level is still a FAST cell: resize_kernel (the flat form)
    makes every level at 2.0 and 1.5, and at 1.334 one level of the frame while resize_strip_kernel makes the other, in either order.
    Every level byte for byte orc_resize_linear_u8's, then candidates, keypoints and descriptors"""
    rows, cols, nl, sc, strips = shape
    raw, orb, ref = X.small_case(orc, rows, cols, nl, sc)
    with _params(ctx, X.SMALL_MASK, orb):
        _run(ctx, orc, 0, raw, ref, "%d x %d at %g, strips %s" % (rows, cols, sc, strips))


def test_pyramid_strips_and_flat_levels_swap_in_one_batch(ctx, orc):
    """the two 1.334 frames of the table in ONE extract_many: at level 1 the first takes resize_kernel and the second resize_strip_kernel,
    at level 2 the other way round -- both kernels run over the batch at both levels and each leaves the other's frame alone"""
    shapes = [s for s in X.PYRAMID_SHAPES if s[3] == 1.334]
    assert [s[4] for s in shapes] == [(False, True), (True, False)]
    cases = [X.small_case(orc, *s[:4]) for s in shapes]
    dr = [X.dr_inputs(*c[0].shape) for c in cases]
    with _params(ctx, X.SMALL_MASK, cases[0][1]):
        for order in ([0, 1], [1, 0]):
            for i, (raw, _, _) in enumerate(cases): ctx.frame_set(i, raw, raw.shape[0], raw.shape[1], *dr[i])
            ctx.extract_many(order)
            for i in order:
                _check_images(ctx, i, cases[i][2], "frame %d in the batch %s" % (i, order))
                _check_features(ctx, orc, i, cases[i][2], dr[i][0], dr[i][2], "frame %d in the batch %s" % (i, order))


@pytest.mark.parametrize("shape", X.WIDE_SHAPES + X.QUOTA_SHAPES, ids=lambda s: "%dx%d" % s[:2])
def test_wide_frames_and_quadtree_roots(ctx, orc, shape):
    """1, 2, 3, 10 / 11, 32, 33 and 53 initial nodes: the stable partition by root, its pcnt bookkeeping, the passes without the pre-sort.
    The ORDER of the final keypoints is the tree's list order, which is what a different set of roots changes first.  Then the two quotas
    of QUOTA_SHAPES on one root: (1, 0), and one whose refinement ranks more nodes than the kernel stages in LDS"""
    rows, cols, nl, nf, roots = shape
    raw, orb, ref = X.wide_case(orc, rows, cols, nl, nf)
    with _params(ctx, X.SMALL_MASK, orb):
        _run(ctx, orc, 0, raw, ref, "%d x %d, %d roots" % (rows, cols, roots))


@pytest.mark.parametrize("ini,mn", X.THRESHOLDS)
def test_fast_thresholds_and_retry(ctx, orc, ini, mn):
    """the gain-ramp frames hold cells with corners above iniThFAST, cells that only the second pass at minThFAST fills, and empty ones;
    (20, 20) and (7, 12) skip the retry (tmin = min(ini, min)), (254, 1) empties every cell at iniThFAST"""
    for N, M in X.RAMP_SHAPES:
        raw, orb, ref = X.ramp_case(orc, N, M, ini, mn)
        with _params(ctx, X.SMALL_MASK, orb):
            _run(ctx, orc, 1, raw, ref, "%d x %d at thresholds (%d, %d)" % (N, M, ini, mn))


def test_border_band_keypoints(ctx, orc):
    """keypoints 19 to 26 px from a border of their level load their patch byte by byte through reflect-101 indices; the small mask lets
    them through the filter.  Eight levels (levels 5 to 7 share one FAST / scan / gather launch group), then two and one"""
    N, M = X.BAND_SHAPE
    pose, alt, gr = X.dr_inputs(N, M)
    for nl in (8, 2, 1):
        raw, orb, ref = X.band_case(orc, nl)
        band = X.band_sides(orc, ref["kps"], N, M, ref["op"]) != 0
        with _params(ctx, X.SMALL_MASK, orb):
            ctx.frame_set(2, raw, N, M, pose, alt, gr)
            assert ctx.extract(2) == len(ref["kps"])
            _check_stages(ctx, 2, ref, "%d levels" % nl)
            _check_features(ctx, orc, 2, ref, pose, gr, "%d levels, dword patches" % nl, ~band)
            _check_features(ctx, orc, 2, ref, pose, gr, "%d levels, reflect-101 patches" % nl, band)
    from diasss_amd import capi
    raw, orb, ref = X.band_case(orc, 8, sift=True)
    band = X.band_sides(orc, ref["kps"], N, M, ref["op"]) != 0
    with _params(ctx, X.SMALL_MASK, dict(orb, descriptor=capi.DESC_SIFT128)):
        ctx.frame_set(2, raw, N, M, pose, alt, gr)
        assert ctx.extract(2) == len(ref["kps"])
        _check_features(ctx, orc, 2, ref, pose, gr, "SIFT call site")
        d = ctx.features_get_sift(2)
        assert d.shape == ref["d128"].shape
        assert (d[~band] == ref["d128"][~band]).all(), "128-element rows differ away from the border"
        assert (d[band] == ref["d128"][band]).all(), "128-element rows differ in the border band"


def test_mask_parameters_and_border_hot_pixels(ctx, orc):
    """the eraser's rule at the borders (nothing is erased for i < r or j < r, the square is cut at the far edges) for r = 6, 2 and 0, a
    threshold factor that is not a float, the static mask of other parameters, and 16-byte mask groups that wrap rows (M = 2 mod 4)"""
    N, M = X.HOT_SHAPE
    Nw, Mw = X.HOT_WRAP_SHAPE
    orb = dict(nfeatures=60, nlevels=1)
    frames = [(X.flat_with_hot(N, M, 1, [pos]), "hot pixel at %s" % (pos,)) for pos, _ in X.HOT_ERASED]
    frames.append((X.flat_with_hot(N, M, 1, [p for p, _ in X.HOT_ERASED]), "all hot pixels"))
    frames.append((X.flat_with_hot(N, M, 2, [], knife=(60, 40), factor=2.3, orc=orc), "pixel between mean * 2.3f and mean * 2.3"))
    frames += [(X.flat_with_hot(Nw, Mw, 3, [pos]), "%d x %d, hot pixel at %s" % (Nw, Mw, pos)) for pos in ((0, 0), (Nw - 1, Mw - 1), (Nw - 1, 0), (0, Mw - 1), (6, 6), (Nw - 2, 7))]
    masks = [X.NO_STATIC_MASK, dict(X.NO_STATIC_MASK, r=2), dict(X.NO_STATIC_MASK, r=0), dict(X.NO_STATIC_MASK, factor=2.3),
             X.SMALL_MASK, X.MASK_INEXACT, X.MASK_R0, dict(factor=2.3, width=10, r=6, side=9)]
    for mi, mask in enumerate(masks):
        mp = X.mask_params(orc, **mask)
        with _params(ctx, mask, orb):
            for raw, what in frames:
                n, m = raw.shape
                pose, alt, gr = X.dr_inputs(n, m)
                ctx.frame_set(3, raw, n, m, pose, alt, gr)
                ctx.extract(3)
                _check_images(ctx, 3, dict(norm=orc.normalize(raw), mask=orc.mask(raw, mp)), "%s, mask %r" % (what, mask))


def test_mixed_shapes_in_one_batch(ctx, orc):
    """69 x 70 (one root), 91 x 272 (windows 59 px tall, four roots) and 69 x 1236 (33 roots) in ONE extract_many, then with 92 x 74 (a
    window 42 px wide: the whole batch runs fast_cells_kernel<68>, alone the other three run <40>).  The launches are sized by the
    batch's maxima; every frame's result is the single-frame call's and the oracle's"""
    cases = [X.small_case(orc, 69, 70, 1, 1.2), X.small_case(orc, 91, 272, 1, 1.2), X.wide_case(orc, 69, 1236, 1, 100), X.small_case(orc, 92, 74, 1, 1.2)]
    cls = [X.shape_class(orc, *c[0].shape) for c in cases]
    assert [c["stride"] for c in cls] == [40, 40, 40, 68] and cls[1]["max_ch"] == 59 and [c["roots"][0] for c in cls] == [1, 4, 33, 1]
    orb = dict(nfeatures=100, nlevels=1)          # (the 33 roots keep up to 132 keypoints: see test_roots_beyond_the_keypoint_store_are_refused)
    refs = [X.oracle_stages(orc, c[0], X.SMALL_MASK, orb, key=("mixed", i)) for i, c in enumerate(cases)]
    dr = [X.dr_inputs(*c[0].shape) for c in cases]
    with _params(ctx, X.SMALL_MASK, orb):
        single = []
        for i, (raw, _, _) in enumerate(cases):
            _run(ctx, orc, i, raw, refs[i], "frame %d alone" % i)
            single.append([np.asarray(a).tobytes() for a in ctx.features_get(i)])
        for order in ([0, 1, 2], [2, 0, 1], [3, 2, 0, 1]):
            for i, (raw, _, _) in enumerate(cases): ctx.frame_set(i, raw, raw.shape[0], raw.shape[1], *dr[i])
            ctx.extract_many(order)
            for i in order:
                _check_images(ctx, i, refs[i], "frame %d in the batch %s" % (i, order))
                _check_features(ctx, orc, i, refs[i], dr[i][0], dr[i][2], "frame %d in the batch %s" % (i, order))
                assert [np.asarray(a).tobytes() for a in ctx.features_get(i)] == single[i], "frame %d: batch %s and single call differ" % (i, order)


def test_roots_beyond_the_keypoint_store_are_refused(ctx, orc):
    """the first pass of the tree divides every root whatever the quota is: 33 roots keep up to 132 keypoints, the store of nfeatures = 60
    holds 128.  Refused on the host with DSSS_E_ARG before any launch -- never another tree, never an overrun; at nfeatures = 100 the
    same frame is the oracle's (test_wide_frames_and_quadtree_roots), and the context extracts correctly after the refusal"""
    from diasss_amd.capi import DsssError
    raw, orb, ref = X.wide_case(orc, 69, 1236, 1, 100)
    assert len(X.unfiltered_keypoints(orc, ref)) > 128
    pose, alt, gr = X.dr_inputs(69, 1236)
    with _params(ctx, X.SMALL_MASK, dict(nfeatures=60, nlevels=1)):
        ctx.frame_set(0, raw, 69, 1236, pose, alt, gr)
        with pytest.raises(DsssError) as ei:
            ctx.extract(0)
        assert ei.value.code == -2 and "roots" in str(ei.value)
        with pytest.raises(DsssError) as ei:
            ctx.extract_many([0])
        assert ei.value.code == -2
    with _params(ctx, X.SMALL_MASK, orb):
        _run(ctx, orc, 0, raw, ref, "69 x 1236 after the refusal")


def test_device_input_at_eight_byte_alignment(ctx, orc):
    """a borrowed device image whose address is 8 (mod 16): the view from element 1 of a tensor of N M + 1 doubles.  row_reduce_kernel and
    normalize_kernel read pairs of doubles; neither may assume more alignment than a double has"""
    import torch
    N, M = 121, 122
    raw, orb, ref = X.small_case(orc, N, M, 1, 1.2)
    buf = torch.zeros(N * M + 1, dtype=torch.float64, device="cuda")
    view = buf[1:].view(N, M)
    view.copy_(torch.from_numpy(raw))
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 8 and view.is_contiguous()
    with _params(ctx, X.SMALL_MASK, orb):
        _run(ctx, orc, 0, raw, ref, "image at 8 (mod 16)", image=view)
        aligned = torch.from_numpy(raw).cuda()
        assert aligned.data_ptr() % 16 == 0
        _run(ctx, orc, 1, raw, ref, "image at 0 (mod 16)", image=aligned)

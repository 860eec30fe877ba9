"""GPU parity of sift_desc_kernel (dsss_sift.hip) at its edges: the frames of tests/sift_shapes_ref.py (tests/test_sift_shapes_cpu.py holds
them to the classes they are named for) extracted with DSSS_DESC_SIFT128, every stage of _check_features as the ORB tests have it, the
128-byte rows of the surviving keypoints, and -- under DSSS_SIFT_HIST_DUMP -- the raw 2^-12 histogram of EVERY pre-filter keypoint against
orc_sift_hist on the oracle's blurred level.  Failures are counted per window class, so that a message names the loading path: levels of
69 px where the 71 x 71 window is clipped on opposite sides or on all four, keypoints on either side of each equality of the dword
condition, IC angles of exactly 0, designed flat-field frames, and batches of frames of different shapes in both orders."""
import numpy as np
import pytest

from tests import extract_shapes_ref as X
from tests import sift_shapes_ref as S
from tests.test_gpu_extract_shapes import _check_features, _check_images, _params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from diasss_amd import capi
    c = capi.Context(max_frames=4)
    yield c
    c.close()


def _sift_params(ctx, mask, orb):
    from diasss_amd import capi
    return _params(ctx, mask, dict(orb, descriptor=capi.DESC_SIFT128))


def _per_class(bad, cls):
    """'3 of 17 left+top (reflect-101 path), ...' for the keypoints flagged in `bad`"""
    return ", ".join("%d of %d %s" % (int(bad[cls == k].sum()), int((cls == k).sum()), S.CLASS_NAME[k]) for k in np.unique(cls[bad]))


def _check_rows(ctx, fid, c, what):
    d = ctx.features_get_sift(fid)
    want = c["ref"]["d128"]
    assert d.dtype == np.float32 and d.shape == want.shape, "%s: rows of shape %s, the oracle %s" % (what, d.shape, want.shape)
    bad = (d != want.astype(np.float32)).any(1)
    assert not bad.any(), "%s: 128-byte rows differ: %s" % (what, _per_class(bad, c["surv_cls"]))


def _check_hist(H, c, what):
    """H: int32[kcap][128], the slice of one frame of the dump"""
    n = len(c["pre"])
    assert n <= len(H), "%s: %d pre-filter keypoints, the dump holds %d" % (what, n, len(H))
    bad = (H[:n] != c["hist"]).any(1)
    assert not bad.any(), "%s: raw histograms differ: %s" % (what, _per_class(bad, c["cls"]))
    assert (H[n:] == 0).all(), "%s: the dump is not zero behind keypoint %d" % (what, n)


def _extract_with_dump(ctx, monkeypatch, path, call):
    monkeypatch.setenv("DSSS_SIFT_HIST_DUMP", str(path))
    try:
        out = call()
    finally:
        monkeypatch.delenv("DSSS_SIFT_HIST_DUMP")
    return out, np.fromfile(str(path), np.int32).reshape(-1, 128)


def _run(ctx, orc, fid, c, what, monkeypatch, path):
    raw, ref = c["raw"], c["ref"]
    N, M = raw.shape
    pose, alt, gr = X.dr_inputs(N, M)
    ctx.frame_set(fid, raw, N, M, pose, alt, gr)
    n, H = _extract_with_dump(ctx, monkeypatch, path, lambda: ctx.extract(fid))
    assert n == len(ref["kps"]), "%s: %d keypoints, the oracle %d" % (what, n, len(ref["kps"]))
    _check_images(ctx, fid, ref, what)
    _check_features(ctx, orc, fid, ref, pose, gr, what)
    _check_rows(ctx, fid, c, what)
    _check_hist(H, c, what)
    return H


@pytest.mark.parametrize("name", S.NAMES)
def test_sift_rows_and_histograms_per_window_class(ctx, orc, name, tmp_path, monkeypatch):
    """one frame of the table: small levels (69 to 122 px, the window clipped on up to four sides), pyramids, wide frames, the border band
    at eight and two levels, the mirror frames (IC angle exactly 0: ori = 360 is reset to 0), the diag frames (IC angle on a diagonal at the
    equalities of the dword condition and one step outside them: where an off-by-one of that condition shows), the flat-field designs"""
    c = S.case(orc, name)
    with _sift_params(ctx, c["mask"], c["orb"]):
        _run(ctx, orc, 0, c, name, monkeypatch, tmp_path / "hist.bin")


def test_sift_batch_of_different_shapes_in_both_orders(ctx, orc, tmp_path, monkeypatch):
    """69 x 70, 69 x 1236, 100 x 100 and a flat 72 x 76 without a keypoint in ONE extract_many at two levels: sift_desc_kernel runs
    dim3(kcap, 4) and every block past its frame's keypoint count returns.  Rows and raw histograms of every frame are its single-frame
    reference's; the dump is int32[4][kcap][128] in the order of the call, zero for the empty frame and behind every frame's keypoints"""
    cases = [S.case(orc, b) for b in S.BATCH]
    dr = [X.dr_inputs(*c["raw"].shape) for c in cases]
    assert [len(c["pre"]) == 0 for c in cases] == [False, False, False, True]
    with _sift_params(ctx, cases[0]["mask"], cases[0]["orb"]):
        kcap = None
        for i, c in enumerate(cases):
            H = _run(ctx, orc, i, c, "%s alone" % c["name"], monkeypatch, tmp_path / "one.bin")
            assert kcap in (None, len(H)); kcap = len(H)
        for order in ([0, 1, 2, 3], [3, 2, 1, 0]):
            for i, c in enumerate(cases): ctx.frame_set(i, c["raw"], c["raw"].shape[0], c["raw"].shape[1], *dr[i])
            _, H = _extract_with_dump(ctx, monkeypatch, tmp_path / "many.bin", lambda: ctx.extract_many(order))
            assert H.shape == (4 * kcap, 128), "the dump of a batch of four is int32[4][kcap = %d][128], not %d rows" % (kcap, len(H))
            H = H.reshape(4, kcap, 128)
            for s, i in enumerate(order):
                what = "%s as frame %d of the batch %s" % (cases[i]["name"], s, order)
                _check_images(ctx, i, cases[i]["ref"], what)
                _check_features(ctx, orc, i, cases[i]["ref"], dr[i][0], dr[i][2], what)
                _check_rows(ctx, i, cases[i], what)
                _check_hist(H[s], cases[i], what)
            assert (H[order.index(3)] == 0).all(), "the slice of the frame without keypoints is zero"

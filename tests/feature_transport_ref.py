"""The packed per-frame feature record that travels between ranks, built and parsed in numpy from its documented layout
(include/dsss.h, the comment over dsss_features_pack_bytes):

    [int32 n, N, M, 0][bbox 4 f64][kps K][desc K x 32][geo K x 2 f64]   ( + [desc128 K x 128] under DSSS_DESC_SIFT128)

K is the per-frame capacity of the context; every section has K rows whatever n is.  Also the block rule that says which rank owns
which frame, the size of a rank's slice of the all-gather, and the case tables of tests/test_gpu_feature_transport.py and of the
uneven lock-step cases of tests/test_gpu_multirank.py.  No device code: the expected side of those tests."""
import numpy as np

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4")])
HEADER = 16 + 32                                   # four int32, four float64
ROW_BYTES = KP_DTYPE.itemsize + 32 + 16            # one keypoint, its 32 descriptor bytes, its geo sample
SIFT_ROW_BYTES = 128


def record_bytes(K, sift):
    return HEADER + K * (ROW_BYTES + (SIFT_ROW_BYTES if sift else 0))


def capacity(nbytes, sift):
    """K of a context from its dsss_features_pack_bytes"""
    per_row = ROW_BYTES + (SIFT_ROW_BYTES if sift else 0)
    K, rest = divmod(nbytes - HEADER, per_row)
    assert rest == 0 and K > 0, (nbytes, sift)
    return K


def _sections(K, sift):
    """(name, offset, bytes per row) of the record's sections, in order"""
    off = HEADER
    out = []
    for name, w in (("kps", KP_DTYPE.itemsize), ("desc", 32), ("geo", 16)) + ((("d128", SIFT_ROW_BYTES),) if sift else ()):
        out.append((name, off, w)); off += K * w
    assert off == record_bytes(K, sift)
    return out


def build_record(K, n, N, M, bbox, kps, desc, geo, d128=None, fill=0):
    """The record's bytes (uint8 array).  n, N, M go into the header as they are (n may lie outside [0, K]: a hostile peer); the rows
    written are those of kps / desc / geo (/ d128), at most K; every byte of a section behind them is `fill`."""
    kps = np.ascontiguousarray(kps, KP_DTYPE); rows = len(kps)
    desc = np.ascontiguousarray(desc, np.uint8).reshape(rows, 32)
    geo = np.ascontiguousarray(geo, np.float64).reshape(rows, 2)
    assert rows <= K
    sift = d128 is not None
    buf = np.full(record_bytes(K, sift), fill, np.uint8)
    buf[:16] = np.array([n, N, M, 0], "<i4").view(np.uint8)
    buf[16:48] = np.ascontiguousarray(bbox, "<f8").reshape(4).view(np.uint8)
    parts = dict(kps=kps, desc=desc, geo=geo)
    if sift:
        parts["d128"] = np.ascontiguousarray(d128, np.uint8).reshape(rows, SIFT_ROW_BYTES)
    for name, off, w in _sections(K, sift):
        buf[off:off + rows * w] = parts[name].view(np.uint8).reshape(-1)
    return buf


def parse_record(buf, K, sift):
    """dict(n, N, M, pad, bbox (4,), kps (K,), desc (K, 32), geo (K, 2), d128 (K, 128) or None): copies, all K rows of every section"""
    buf = np.ascontiguousarray(buf, np.uint8).reshape(-1)
    assert buf.size == record_bytes(K, sift), (buf.size, K, sift)
    h = buf[:16].copy().view("<i4")
    out = dict(n=int(h[0]), N=int(h[1]), M=int(h[2]), pad=int(h[3]), bbox=buf[16:48].copy().view("<f8"), d128=None)
    for name, off, w in _sections(K, sift):
        sec = buf[off:off + K * w].copy()
        out[name] = {"kps": lambda s: s.view(KP_DTYPE), "desc": lambda s: s.reshape(K, 32), "geo": lambda s: s.view("<f8").reshape(K, 2),
                     "d128": lambda s: s.reshape(K, SIFT_ROW_BYTES)}[name](sec)
    return out


# ---------------------------------------------------------------- who owns what
def block(F, r, W):
    """frames of rank r of W: [F r // W, F (r + 1) // W)"""
    return F * r // W, F * (r + 1) // W


def owner(F, W, f):
    return next(r for r in range(W) if block(F, r, W)[0] <= f < block(F, r, W)[1])


def per(F, W):
    """records in a rank's slice of the all-gather: the longest block"""
    return max(block(F, r, W)[1] - block(F, r, W)[0] for r in range(W))


def slice_bytes(F, W, nbytes):
    return per(F, W) * nbytes


def record_at(row, F, W, f, nbytes):
    """the bytes of frame f's record inside its owner's row of the gathered (W, slice) array"""
    i = f - block(F, owner(F, W, f), W)[0]
    return row[i * nbytes:(i + 1) * nbytes]


# ---------------------------------------------------------------- case tables
# (F, W) of the gather tests: (7, 3) blocks of 2, 2, 3; (5, 4) blocks of 1, 1, 1, 2; (3, 4) blocks of 0, 1, 1, 1: rank 0 owns nothing.
SPLITS = ((7, 3), (5, 4), (3, 4))
# Per case two rounds of per-frame keypoint counts ("K" = the capacity): the second gather of a context meets frames whose count went
# down and frames whose count went up, and the two rounds of a case hold 0, 1, 63, 64, 65 and K between them ((7, 3) in each).
COUNTS = {
    (7, 3): (("K", 1, 63, 64, 65, 0, 150), (0, 65, "K", 63, 1, 64, 150)),
    (5, 4): (("K", 0, 65, 150, 64), (63, "K", 1, 64, 150)),
    (3, 4): (("K", 0, 65), (64, 1, 63)),
}
EDGE_COUNTS = (0, 1, 63, 64, 65, "K")
# Pairs the matcher runs after a round's gather; every pair has its frames on two ranks.  The first pairs of a round are of one parity
# (the matcher takes frames of one parity for legs of one heading) and hold at least 63 keypoints each; the last is of mixed parity.
MATCH_PAIRS = {
    (7, 3): (((2, 4), (0, 6), (0, 3)), ((2, 6), (1, 5), (1, 2))),
    (5, 4): (((0, 2), (2, 4), (0, 3)), ((1, 3), (0, 4), (0, 1))),
    (3, 4): (((0, 2), (0, 1)), ((0, 2), (1, 2))),
}
# (F, W) of the whole pipeline in lock step: every rank owns a frame; in (5, 4) rank 0 owns frame 0 alone and matches no pair
LOCKSTEP = ((7, 3), (5, 4))


def counts(case, rnd, K):
    return [K if n == "K" else n for n in COUNTS[case][rnd]]


# ---------------------------------------------------------------- designed frames
FRAME_N, FRAME_M = 700, 480
_FRAMES = {}


def design_frames(orc, case, rnd, K, sift=False):
    """The F frames of a case's round, laid out as test_gpu_matcher._same_leg_pair lays its two: all on leg 0 (helpers.track), frame f 0.15 f m
    to the side, keypoints = the first n of ONE list of K landmarks moved by a few pixels and descriptor bits per frame, so that frames
    of one parity match.  geo is the oracle's sample at the keypoints; the box is the oracle's with margins of the frame's own: wider across
    the track and some metres SHORTER at both ends (past the margin the keypoints keep), so that a box that stayed behind, or landed in another frame, reads differently
    and, since the matcher skips keypoints outside the other frame's box, matches differently.  d128 (sift): the landmarks' 128-byte rows with a few
    elements moved by one.  Made once per (case, rnd, K, sift), arrays read-only.
    -> list of dict(N, M, pose, alt, gr, kps, desc, geo, bb, d128)"""
    key = (case, rnd, K, sift)
    if key in _FRAMES:
        return _FRAMES[key]
    from tests import helpers as H
    F = case[0]
    N, M = FRAME_N, FRAME_M
    pose0, alt, gr = H.track(N, M, 0, seed=3)
    base_k, base_d = H.random_features(N, M, K, 7000 + K)
    base_s = np.random.default_rng(7100 + K).integers(0, 256, (K, 128), dtype=np.uint8)
    out = []
    for f, n in enumerate(counts(case, rnd, K)):
        rng = np.random.default_rng([K, F, rnd, f])
        pose = pose0.copy(); pose[:, 4] += 0.15 * f
        kps, desc, d128 = base_k[:n].copy(), base_d[:n].copy(), base_s[:n].copy()
        for i in range(n):
            for b in rng.choice(256, rng.integers(0, 20), replace=False):
                desc[i, b // 8] ^= np.uint8(1 << (b % 8))
        kps["y"] += rng.integers(-3, 4, n).astype(np.float32)
        kps["response"] += np.float32(f + 10 * rnd)               # no two frames or rounds share a keypoint row
        step = rng.random((n, 128)) < 0.05
        d128 = np.where(step, np.where(d128 < 255, d128 + 1, d128 - 1), d128).astype(np.uint8)
        geo = orc.geo_at_kps(pose, gr, M, kps) if n else np.zeros((0, 2))
        bb = orc.geo_bbox(pose, gr, M) + np.array([7.0 + 0.5 * f + 0.25 * rnd, -(6.0 + 0.25 * f), -0.125 * (f + 1), 0.125 * (f + 1)])
        fr = dict(N=N, M=M, pose=pose, alt=alt, gr=gr, kps=kps, desc=desc, geo=np.ascontiguousarray(geo), bb=bb, d128=d128 if sift else None)
        for a in fr.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        out.append(fr)
    _FRAMES[key] = out
    return out


def oracle_view(frames, sift):
    """{f: the dict test_gpu_matcher._check_pair reads}: in SIFT mode the matcher's descriptor is the 128-byte row"""
    return {f: dict(fr, desc=fr["d128"] if sift else fr["desc"]) for f, fr in enumerate(frames)}


def frame_record(fr, K, sift, fill=0, n=None, N=None, M=None):
    """the record a frame's owner sends; n, N, M: a header that lies"""
    return build_record(K, len(fr["kps"]) if n is None else n, fr["N"] if N is None else N, fr["M"] if M is None else M, fr["bb"],
                        fr["kps"], fr["desc"], fr["geo"], fr["d128"] if sift else None, fill)


def gathered(frames, F, W, K, sift, fill, lie=None):
    """the (W, slice) array every rank holds after the all-gather: each rank's row holds the records of its block, every other byte is
    `fill`.  lie = (frame, dict(n= / N= / M=)): that frame's header as a hostile owner would send it"""
    nb = record_bytes(K, sift)
    out = np.full((W, slice_bytes(F, W, nb)), fill, np.uint8)
    for f in range(F):
        kw = lie[1] if lie is not None and lie[0] == f else {}
        record_at(out[owner(F, W, f)], F, W, f, nb)[:] = frame_record(frames[f], K, sift, fill, **kw)
    return out

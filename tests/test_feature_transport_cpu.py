"""CPU: the preconditions of tests/test_gpu_feature_transport.py and of the uneven lock-step cases of tests/test_gpu_multirank.py --
the numpy record of tests/feature_transport_ref.py round-trips, its block rule is the pipeline's, and every case of its tables shows
what it is in the table for."""
import numpy as np
import pytest

from tests import feature_transport_ref as R
from tests import helpers as H

K_SMALL, K_DEFAULT = 192, 2112


def test_record_layout_is_the_bindings():
    from diasss_amd import capi
    assert R.KP_DTYPE == capi.KP_DTYPE == np.dtype(H.O.KP_DTYPE)
    assert R.record_bytes(192, False) == 48 + 192 * (24 + 32 + 16) and R.record_bytes(192, True) == 48 + 192 * (24 + 32 + 16 + 128)
    for K in (64, K_SMALL, K_DEFAULT):
        for sift in (False, True):
            assert R.capacity(R.record_bytes(K, sift), sift) == K
            assert R.record_bytes(K, sift) % 16 == 0                   # records are copied 16 bytes at a time


@pytest.mark.parametrize("sift", [False, True])
@pytest.mark.parametrize("K,n", [(64, 0), (64, 1), (64, 64), (K_SMALL, 63), (K_SMALL, 65), (K_SMALL, K_SMALL)])
def test_build_and_parse_round_trip(K, n, sift):
    rng = np.random.default_rng(K + n)
    kps, desc = H.random_features(700, 480, n, 5 + n)
    geo = rng.standard_normal((n, 2)); bb = rng.standard_normal(4)
    d128 = rng.integers(0, 256, (n, 128), dtype=np.uint8) if sift else None
    buf = R.build_record(K, n, 700, 480, bb, kps, desc, geo, d128, fill=0xA5)
    assert buf.dtype == np.uint8 and buf.size == R.record_bytes(K, sift)
    p = R.parse_record(buf, K, sift)
    assert (p["n"], p["N"], p["M"], p["pad"]) == (n, 700, 480, 0)
    assert p["bbox"].tobytes() == bb.tobytes()
    assert p["kps"][:n].tobytes() == kps.tobytes() and p["desc"][:n].tobytes() == desc.tobytes() and p["geo"][:n].tobytes() == geo.tobytes()
    assert (p["d128"] is None) == (not sift) and (not sift or p["d128"][:n].tobytes() == d128.tobytes())
    for name in ("kps", "desc", "geo") + (("d128",) if sift else ()):     # every byte behind the rows is the fill: the sections do not overlap
        assert len(p[name]) == K and (p[name][n:].view(np.uint8) == 0xA5).all()
    # section offsets as the layout documents them: keypoints at 48, descriptors behind K keypoints, geo behind K descriptors
    if n:
        assert buf[48:48 + 24].tobytes() == kps[:1].tobytes()
        assert buf[48 + 24 * K:48 + 24 * K + 32].tobytes() == desc[0].tobytes()
        assert buf[48 + 56 * K:48 + 56 * K + 16].tobytes() == geo[0].tobytes()
        assert not sift or buf[48 + 72 * K:48 + 72 * K + 128].tobytes() == d128[0].tobytes()
    # a header that lies goes in as it is
    q = R.parse_record(R.build_record(K, K + 1, 699, 480, bb, kps, desc, geo, d128), K, sift)
    assert (q["n"], q["N"]) == (K + 1, 699)
    assert R.parse_record(R.build_record(K, -1, 700, 480, bb, kps, desc, geo, d128), K, sift)["n"] == -1


def test_block_rule_is_the_pipelines():
    from diasss_amd.pipeline import shard_frames, frame_owner
    for F in range(1, 13):
        for W in range(1, 10):
            own = frame_owner(F, W)
            seen = []
            for r in range(W):
                lo, hi = R.block(F, r, W)
                assert list(range(lo, hi)) == shard_frames(F, r, W)
                seen += list(range(lo, hi))
            assert seen == list(range(F))                              # the blocks tile the frames in rank order
            assert [R.owner(F, W, f) for f in range(F)] == own.tolist()
            assert R.per(F, W) == max(len(shard_frames(F, r, W)) for r in range(W)) == -(-F // W)
            assert R.slice_bytes(F, W, 1000) == R.per(F, W) * 1000


def test_record_at_addresses_the_owners_row():
    F, W, nb = 7, 3, 10
    rows = np.zeros((W, R.slice_bytes(F, W, nb)), np.uint8)
    for f in range(F):
        R.record_at(rows[R.owner(F, W, f)], F, W, f, nb)[:] = f + 1
    assert rows[0].tolist() == [1] * 10 + [2] * 10 + [0] * 10 and rows[2].tolist() == [5] * 10 + [6] * 10 + [7] * 10


@pytest.mark.parametrize("case", R.SPLITS)
def test_split_cases_show_what_they_are_for(case):
    F, W = case
    lens = [R.block(F, r, W)[1] - R.block(F, r, W)[0] for r in range(W)]
    assert any(n < R.per(F, W) for n in lens)                          # a rank shorter than the padded slice
    if case == (3, 4):
        assert lens[0] == 0 and F < W                                  # a rank with no frames
    for K in (K_SMALL, K_DEFAULT):
        rounds = [R.counts(case, rnd, K) for rnd in (0, 1)]
        assert all(len(c) == F and all(0 <= n <= K for n in c) for c in rounds)
        edge = {K if n == "K" else n for n in R.EDGE_COUNTS}
        assert edge <= set(rounds[0]) | set(rounds[1])
        if case == (7, 3):
            assert edge <= set(rounds[0]) and edge <= set(rounds[1])
        assert any(a > b for a, b in zip(*rounds)) and any(a < b for a, b in zip(*rounds))      # the second gather: counts went down and up
        for rnd in (0, 1):
            pairs = R.MATCH_PAIRS[case][rnd]
            for a, b in pairs:
                assert a < b < F and R.owner(F, W, a) != R.owner(F, W, b)
            a, b = pairs[0]
            assert a % 2 == b % 2 and min(rounds[rnd][a], rounds[rnd][b]) >= 63
            assert pairs[-1][0] % 2 != pairs[-1][1] % 2


@pytest.mark.parametrize("case", R.SPLITS)
def test_designed_frames_match_under_the_oracle(orc, case):
    """the first pair of every round has more than 5 accepted rows under the oracle, in ORB mode and by L2 on the 128-byte rows"""
    from tests.test_gpu_matcher import _oracle_pair
    po = orc.match_params(); po.use_l2 = 2
    for rnd in (0, 1):
        for K, sift, params in ((K_SMALL, False, None), (K_SMALL, True, po), (K_DEFAULT, False, None)):
            fr = R.oracle_view(R.design_frames(orc, case, rnd, K, sift), sift)
            a, b = R.MATCH_PAIRS[case][rnd][0]
            d01, d10, rows, _ = _oracle_pair(orc, a, b, fr, params)
            assert len(rows) > 5, (case, rnd, K, sift, len(rows))
            # the designed boxes decide matches: with the boxes the geometry alone gives (what a context computes for a frame whose record
            # never arrived) the first stage answers differently
            full = {f: dict(v, bb=orc.geo_bbox(v["pose"], v["gr"], v["M"])) for f, v in fr.items()}
            e01, e10, _, _ = _oracle_pair(orc, a, b, full, params)
            assert (d01["nn"] != e01["nn"]).any() and (d10["nn"] != e10["nn"]).any()
    frames = R.design_frames(orc, case, 0, K_SMALL)
    assert [len(f["kps"]) for f in frames] == R.counts(case, 0, K_SMALL)
    assert len({f["bb"].tobytes() for f in frames}) == len(frames)     # no two frames share a box
    g = R.gathered(frames, *case, K_SMALL, False, 0x5A)
    nb = R.record_bytes(K_SMALL, False)
    for f, fr in enumerate(frames):
        p = R.parse_record(R.record_at(g[R.owner(*case, f)], *case, f, nb), K_SMALL, False)
        assert p["n"] == len(fr["kps"]) and p["kps"][:p["n"]].tobytes() == fr["kps"].tobytes() and p["bbox"].tobytes() == fr["bb"].tobytes()
    lens = [R.block(case[0], r, case[1]) for r in range(case[1])]
    for r, (lo, hi) in enumerate(lens):                                # slots behind a rank's block hold the fill alone
        assert (g[r][(hi - lo) * nb:] == 0x5A).all()


@pytest.mark.parametrize("case", R.LOCKSTEP)
def test_lockstep_cases_show_what_they_are_for(case):
    from diasss_amd.pipeline import all_pairs, shard_pairs
    F, W = case
    lens = [R.block(F, r, W)[1] - R.block(F, r, W)[0] for r in range(W)]
    assert min(lens) >= 1 and any(n < R.per(F, W) for n in lens)        # every rank owns a frame (and poses); the blocks are uneven
    src, tgt = all_pairs(F)
    npairs = [len(shard_pairs(src, tgt, r, W, F)[0]) for r in range(W)]
    assert sum(npairs) == F * (F - 1) // 2 and len(set(npairs)) > 1
    if case == (5, 4):
        assert R.block(F, 0, W) == (0, 1) and npairs[0] == 0            # rank 0 owns frame 0 alone: no pair has it as its target

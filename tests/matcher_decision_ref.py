"""Decision table of the matcher's FIRST stage (dsss_match.hip: mt_best2::accept behind match_grid_kernel and match_nn_kernel): one designed
query per exit of the acceptance rule, the expected CorresID of every keypoint written out.  Shared by tests/test_matcher_tail_cpu.py (the
oracle gives exactly the table) and tests/test_gpu_matcher.py (the device gives what the oracle gives).

Three frames of 8 keypoints with explicit geo points and boxes; the pairs (0, 1) and (0, 2) have ids of different and of the same parity
(Hamming bound 80 and 88).  "Sites" lie 30 m apart (radius 8: only keypoints of one site are ever candidates of each other).  Keypoint k of
frame 0 sits on site k; what frames 1 and 2 hold there, as the distance of each of their keypoints to frame 0's descriptor of the site
(Hamming: flipped bits; L2 on the 32 bytes: the squared distance, from byte differences):

    site  frame 0    frame 1 (index: Hamming | L2 squared)          frame 2
    A     k0         --                                             --                                  nothing inside the radius
    B     k1, 3 m    1.0: 10 | 100     (inside the box, 5 m away)   --                                  query outside the other box
          outside
    C     k2         1.1: 50 | 122499  (349.998 < 350)              2.0: 100 | 122500  (350 < 350 is false)   one candidate, in / beyond the bound
    D     k3         1.2: 85 | 122500                               2.1: 85 | 122499                    85: beyond 80, inside 88
    E     k4         1.3: 40 | 1600,  1.4: 10 | 100   (ratio .25)   2.2: 30 | 900,  2.3: 40 | 1600  (ratio .75)   two candidates, ratio passes / fails
    F     k5         --                                             2.4: 89 | 122500,  2.5: 255 | 1036800    ratio passes (.349 | .344), best beyond the bound
    G     k6         1.5: 20 | 400,  1.6: 20 | 400                  2.6: 20 | 400,  2.7: 20 | 400       tie: ratio 1 rejects; lowest index under ratio = 1
    H     k7         1.7: 81 | 900                                  --                                  one candidate, 81 > 80 (L2: accepted)

In the other direction every keypoint of frames 1 and 2 meets exactly the one keypoint of frame 0 on its site (the nc = 1 exit, bound alone).
The tied candidates have different descriptors, and 2.7 lies in a lower cell of the geo grid than 2.6: the grid meets the higher index first.
Each table is given for the default ratio 0.35 and for ratio = 1, where the ratio test passes everything and the tie shows its index.

THE L2-128 DESIGN (use_l2 = 2: the MODE 2 instantiations of both kernels, eight uint4 per row, rows fetched from the feature store).  Same
sites, box and geo offsets, and four more sites (I to L) for the lines that the 32-byte tables do not have; rows of 128 bytes whose first
32 are random (some of them 128 or above) and whose other 96 alternate between 40 and 200.  EVERY difference to frame 0's row of the site
lies in bytes 32 to 127 and in at least two of the eight 16-byte words (difference k of a candidate sits at byte 32 + (start + 17 k) mod
96, added where the base byte is below 128 and subtracted where it is not) -- a kernel that reads 32 bytes of a row sees distance 0
everywhere, one that strides rows by 32 reads other rows.  The one exception is the far candidate, which the issue defines as all 128 bytes
90 away.  Squared distances to frame 0's row:

    site  frame 0    frame 1                                   frame 2
    A     k0         --                                        --                                   nothing inside the radius
    B     k1, 3 m    1.0: 100  (inside the box, 5 m away)      --                                   query outside the other box
          outside
    C     k2         1.1: 122499  (349.998 < 350)              2.0: 122500  (350 < 350 is false)    one candidate, in / at the bound
    D     k3         1.2: 122500                               2.1: 122499
    E     k4         1.3: 1600,  1.4: 100   (ratio .25)        2.2: 900,  2.3: 1600  (ratio .75)    two candidates, ratio passes / fails
    F     k5         --                                        2.4: 122500,  2.5: 1036800           ratio .35 passes, best at the bound
    G     k6         1.5: 400,  1.6: 400  (different rows)     2.6: 400,  2.7: 400                  tie; 2.7 lies in the lower grid cell
    H     k7         1.7: 900                                  --                                   one candidate
    I     k8         1.8: 100,  1.9: 400                       2.8: 400,  2.9: 100                  ratio 10 / 20 = 0.5 exactly: <= 0.5 accepts
    J     k9         1.10: 1036800                             --                                   one candidate above the 1 000 000 sentinel:
                                                                                                    never the best, id stays -1, refused
    K     k10        1.11: 122499,  1.12: 1036800              2.10: 1036800,  2.11: 100            the far one never becomes the second either:
                                                                                                    ratio = best / 1000
    L     k11        1.13: 100, at (8.0, 0.0)                  2.12: 100, at (0.0, -8.0)            exactly `radius` away: d2 < gate_T excludes it

In the other direction every keypoint meets one keypoint of frame 0 or none.  Under L2 a lone candidate inside the bound has ratio
best / 1000 < 0.35, so at the issue's ratios (0.35, 0.5, 1.0) the first line of the rule accepts it already; the table is also given at
ratio 0.2, where 349.998 / 1000 fails the ratio test and the nc == 1 exit decides ALONE (k2 in frame 1, k3 in frame 2, and their
reverse queries)."""
import numpy as np

from oracle import binding as O
from tests import helpers as H

N, M = 700, 480
BB = np.array([-20.0, 200.0, 5.0, 65.0])                        # x0 x1 y0 y1 of all three frames
SITE = {"A": (0.0, 20.0), "B": (203.0, 20.0), "C": (30.0, 20.0), "D": (60.0, 20.0), "E": (90.0, 20.0), "F": (120.0, 20.0), "G": (30.0, 50.0), "H": (60.0, 50.0)}
BELOW = [175, 175, 175, 174, 18, 4, 2, 2]                       # byte differences whose squares sum to 350^2 - 1
AT = [175, 175, 175, 175]                                       # ... to 350^2
FAR = [180] * 32                                                # ... to 1018.2^2
# (site, geo offset, first flipped bit, flipped bits, byte differences from byte 0 on or (first byte, differences))
FRAME = {
    1: [("B", (-5.0, 0.0), 0, 10, [10]), ("C", (1.0, 0.5), 0, 50, BELOW), ("D", (1.0, 0.5), 0, 85, AT), ("E", (1.0, 0.5), 0, 40, [40]),
        ("E", (-1.5, 1.0), 0, 10, [10]), ("G", (1.0, 0.5), 0, 20, [20]), ("G", (-1.5, 1.0), 100, 20, (5, [20])), ("H", (1.0, 0.5), 0, 81, [30])],
    2: [("C", (1.0, 0.5), 0, 100, AT), ("D", (1.0, 0.5), 0, 85, BELOW), ("E", (1.0, 0.5), 0, 30, [30]), ("E", (-1.5, 1.0), 0, 40, [40]),
        ("F", (1.0, 0.5), 0, 89, AT), ("F", (-1.5, 1.0), 0, 255, FAR), ("G", (3.0, 3.0), 0, 20, [20]), ("G", (-3.0, -3.0), 100, 20, (5, [20]))],
}
# expected first-stage CorresID: EXPECT[use_l2][ratio][(other frame, direction)], direction 0 = frame 0 asks
EXPECT = {
    0: {0.35: {(1, 0): [-1, -1, 1, -1, 4, -1, -1, -1], (1, 1): [1, 2, -1, 4, 4, 6, 6, -1],
               (2, 0): [-1, -1, -1, 1, -1, -1, -1, -1], (2, 1): [-1, 3, 4, 4, -1, -1, 6, 6]},
        1.0: {(1, 0): [-1, -1, 1, -1, 4, -1, 5, -1], (1, 1): [1, 2, -1, 4, 4, 6, 6, -1],
              (2, 0): [-1, -1, -1, 1, 2, -1, 6, -1], (2, 1): [-1, 3, 4, 4, -1, -1, 6, 6]}},
    1: {0.35: {(1, 0): [-1, -1, 1, -1, 4, -1, -1, 7], (1, 1): [1, 2, -1, 4, 4, 6, 6, 7],
               (2, 0): [-1, -1, -1, 1, -1, -1, -1, -1], (2, 1): [-1, 3, 4, 4, -1, -1, 6, 6]},
        1.0: {(1, 0): [-1, -1, 1, -1, 4, -1, 5, 7], (1, 1): [1, 2, -1, 4, 4, 6, 6, 7],
              (2, 0): [-1, -1, -1, 1, 2, -1, 6, -1], (2, 1): [-1, 3, 4, 4, -1, -1, 6, 6]}},
}
# ---- the L2-128 design
SITE.update({"I": (90.0, 50.0), "J": (120.0, 50.0), "K": (150.0, 20.0), "L": (150.0, 50.0)})
S100, S400, S400B, S900, S1600 = [6, 8], [12, 16], [16, 12], [18, 24], [24, 32]
# (site, geo offset, byte differences or "far", start)
FRAME128 = {
    1: [("B", (-5.0, 0.0), S100, 0), ("C", (1.0, 0.5), BELOW, 3), ("D", (1.0, 0.5), AT, 7), ("E", (1.0, 0.5), S1600, 1), ("E", (-1.5, 1.0), S100, 20),
        ("G", (1.0, 0.5), S400, 0), ("G", (-1.5, 1.0), S400B, 5), ("H", (1.0, 0.5), S900, 40), ("I", (1.0, 0.5), S100, 9), ("I", (-1.5, 1.0), S400, 33),
        ("J", (1.0, 0.5), "far", 0), ("K", (1.0, 0.5), BELOW, 11), ("K", (-1.5, 1.0), "far", 0), ("L", (8.0, 0.0), S100, 2)],
    2: [("C", (1.0, 0.5), AT, 3), ("D", (1.0, 0.5), BELOW, 7), ("E", (1.0, 0.5), S900, 1), ("E", (-1.5, 1.0), S1600, 20), ("F", (1.0, 0.5), AT, 13),
        ("F", (-1.5, 1.0), "far", 0), ("G", (3.0, 3.0), S400, 0), ("G", (-3.0, -3.0), S400B, 5), ("I", (1.0, 0.5), S400, 33), ("I", (-1.5, 1.0), S100, 9),
        ("K", (1.0, 0.5), "far", 0), ("K", (-1.5, 1.0), S100, 11), ("L", (0.0, -8.0), S100, 2)],
}
RATIOS128 = (0.2, 0.35, 0.5, 1.0)
_REV1, _REV2 = [1, 2, -1, 4, 4, 6, 6, 7, 8, 8, -1, 10, -1, -1], [-1, 3, 4, 4, -1, -1, 6, 6, 8, 8, -1, 10, -1]      # one candidate or none: no ratio moves them
EXPECT[2] = {
    0.2: {(1, 0): [-1, -1, 1, -1, -1, -1, -1, 7, -1, -1, -1, -1], (1, 1): _REV1,
          (2, 0): [-1, -1, -1, 1, -1, -1, -1, -1, -1, -1, 11, -1], (2, 1): _REV2},
    0.35: {(1, 0): [-1, -1, 1, -1, 4, -1, -1, 7, -1, -1, 11, -1], (1, 1): _REV1,
           (2, 0): [-1, -1, -1, 1, -1, -1, -1, -1, -1, -1, 11, -1], (2, 1): _REV2},
    0.5: {(1, 0): [-1, -1, 1, -1, 4, -1, -1, 7, 8, -1, 11, -1], (1, 1): _REV1,
          (2, 0): [-1, -1, -1, 1, -1, -1, -1, -1, 9, -1, 11, -1], (2, 1): _REV2},
    1.0: {(1, 0): [-1, -1, 1, -1, 4, -1, 5, 7, 8, -1, 11, -1], (1, 1): _REV1,
          (2, 0): [-1, -1, -1, 1, 2, -1, 6, -1, 9, -1, 11, -1], (2, 1): _REV2},
}
_CACHE = {}


def row128(base, diffs, start):
    """the 128-byte row `diffs` away from `base`"""
    d = base.astype(np.int64)
    if isinstance(diffs, str):
        pos, diffs = range(128), [90] * 128
    else:
        pos = [32 + (start + 17 * k) % 96 for k in range(len(diffs))]
    for p, v in zip(pos, diffs):
        d[p] += v if base[p] < 128 else -v
    assert d.min() >= 0 and d.max() <= 255
    return d.astype(np.uint8)


def _frames128():
    rng = np.random.default_rng(128)
    base = {}
    for s in "ABCDEFGHIJKL":
        b = np.where(np.arange(128) % 2 == 0, 40, 200).astype(np.uint8)
        b[:32] = rng.integers(0, 256, 32, dtype=np.uint8)
        base[s] = b
    spec = {0: [(s, (0.0, 0.0), [], 0) for s in "ABCDEFGHIJKL"], 1: FRAME128[1], 2: FRAME128[2]}
    fr = {}
    for f, ents in spec.items():
        pose, alt, gr = H.track(N, M, f, seed=3)
        kps, orb = H.random_features(N, M, len(ents), 7 + f)
        geo = np.array([[SITE[e[0]][0] + e[1][0], SITE[e[0]][1] + e[1][1]] for e in ents], np.float64)
        desc = np.array([row128(base[e[0]], e[2], e[3]) for e in ents], np.uint8)
        fr[f] = dict(N=N, M=M, pose=pose, alt=alt, gr=gr, kps=kps, desc=desc, orb=orb, geo=geo, bb=BB.copy())      # desc: what the L2-128 matcher compares
        for a in fr[f].values():
            if isinstance(a, np.ndarray): a.setflags(write=False)
    return fr


def frames(use_l2):
    """{id: frame dict as test_gpu_matcher._check_pair takes it} of the three frames under the Hamming (0), the L2-on-bytes (1) or the L2-128
    (2: desc holds the 128-byte rows, orb the 32 bytes that dsss_features_set wants) design"""
    if use_l2 in _CACHE:
        return _CACHE[use_l2]
    if use_l2 == 2:
        _CACHE[2] = _frames128()
        return _CACHE[2]
    rng = np.random.default_rng(5)
    base = {s: (np.full(32, 40, np.uint8) if use_l2 else rng.integers(0, 256, 32, dtype=np.uint8)) for s in SITE}

    def desc_of(site, bit0, nbits, diffs):
        d = base[site].copy()
        if use_l2:
            b0, diffs = diffs if isinstance(diffs, tuple) else (0, diffs)
            d[b0:b0 + len(diffs)] += np.array(diffs, np.uint8)
        else:
            for b in range(bit0, bit0 + nbits):
                d[b // 8] ^= np.uint8(1 << (b % 8))
        return d
    spec = {0: [(s, (0.0, 0.0), 0, 0, []) for s in "ABCDEFGH"], 1: FRAME[1], 2: FRAME[2]}
    fr = {}
    for f, ents in spec.items():
        pose, alt, gr = H.track(N, M, f, seed=3)
        kps, _ = H.random_features(N, M, len(ents), 7 + f)
        geo = np.array([[SITE[e[0]][0] + e[1][0], SITE[e[0]][1] + e[1][1]] for e in ents], np.float64)
        desc = np.array([desc_of(e[0], e[2], e[3], e[4]) for e in ents], np.uint8)
        fr[f] = dict(N=N, M=M, pose=pose, alt=alt, gr=gr, kps=kps, desc=desc, geo=geo, bb=BB.copy())
        for a in fr[f].values():
            if isinstance(a, np.ndarray): a.setflags(write=False)
    _CACHE[use_l2] = fr
    return fr


def params(use_l2, ratio):
    p = O.match_params(); p.use_l2 = use_l2; p.ratio = ratio
    return p


def oracle_nn(use_l2, ratio, other, direction):
    """the oracle's first-stage CorresID of one directed pair, computed once"""
    key = (use_l2, ratio, other, direction)
    if key not in _CACHE:
        fr = frames(use_l2)
        (ia, a), (ib, b) = ((0, fr[0]), (other, fr[other])) if direction == 0 else ((other, fr[other]), (0, fr[0]))
        nn = O.match_dir(ia, ib, b["N"], a["kps"], a["desc"], a["geo"], b["kps"], b["desc"], b["geo"], b["bb"], params(use_l2, ratio), scc=False)["nn"]
        nn.setflags(write=False)
        _CACHE[key] = nn
    return _CACHE[key]

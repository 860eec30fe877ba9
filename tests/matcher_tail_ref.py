"""Designed correspondences for everything BEHIND the nearest-neighbour kernels of dsss_match.hip: scc_kernel, pair_rows_kernel<false/true>
(ConsistentCheck, the rows, GetKpsPairs, the sticky yaw flags of kp7_flip) and scan2_kernel.  Shared by tests/test_matcher_tail_cpu.py
(oracle only: every case reaches the branch it is named for) and tests/test_gpu_matcher_tail.py.

dsss_features_set takes explicit geo points and an explicit box, so the gate is decoupled from the keypoint coordinates: "sites" sit on a
lattice 20 m apart (more than twice the radius of 8: nothing at different sites is ever a candidate), each site has one random 32-byte
descriptor D, and D2 = D with 60 bits flipped (60 <= both Hamming bounds, 80 and 88).  What a site holds decides the first stage exactly:

    kind      frame A holds     frame B holds     A->B                 B->A
    mutual    i : D             j : D             i -> j  (nc = 1)     j -> i
    extraA    i1 : D, i2 : D2   j : D             i1 -> j, i2 -> j     j -> i1  (0 / 60), so i2 -> j is a non-mutual row
    extraB    i : D             j1 : D, j2 : D2   i -> j1              j1 -> i, j2 -> i
    rejA2B    i : D             j1 : D, j2 : D    none (0 / 0 is NaN)  j1 -> i, j2 -> i
    rejB2A    i1 : D, i2 : D    j : D             i1 -> j, i2 -> j     none
    onlyA     i : D             --                none                 --
    onlyB     --                j : D             --                   none

and the (y, x) of the keypoints are free to steer what follows: the SCC abscissa of a match is |ya - yb|, or |ya - (rows_ref - yb + 1)| for ids
of different parity; every y here is an integer + {0, .25, .5, .75}, exact in float.  With opposite parity the builder sets
yb = Nb + 1 - ya + offset, so the A->B abscissa is `offset` and the B->A abscissa |offset + Nb - Na|.

Plain functions, no fixtures; cases and oracle records are computed once per session and never edited.
"""
import numpy as np

from oracle import binding as O
from tests import helpers as H

SPACING, PER_ROW = 20.0, 40
KINDS = {"mutual": (1, 1), "extraA": (2, 1), "extraB": (1, 2), "rejA2B": (1, 2), "rejB2A": (2, 1), "onlyA": (1, 0), "onlyB": (0, 1)}
YAW_THR = 2 * np.pi / 3
_CACHE = {}


def S(kind, n, off, **ov):
    """n sites of one kind and one SCC offset: (kind, offset, overrides) each"""
    return [(kind, off, ov)] * n


def _flip_bits(rng, d, k):
    d = d.copy()
    for b in rng.choice(256, k, replace=False):
        d[b // 8] ^= np.uint8(1 << (b % 8))
    return d


def build_pair(sites, ids=(0, 2), N=(700, 700), M=(480, 480), seed=0, shuffle=True, tracks=None):
    """The two frames of a designed pair.  sites: list of (kind, offset) or (kind, offset, overrides); overrides: dict with any of ya, xa,
    yb, xb (the coordinates of every keypoint the site has in that frame; with ya and yb both given the offset is not used).  tracks:
    {id: (pose6, alt, gr)}, default helpers.track(N, M, id, seed=3).  Keypoints are shuffled (seeded) unless shuffle is False: then they
    stand in site order, i1 before i2.  Returns dict(ids, fr={id: frame dict as test_gpu_matcher._check_pair takes it}, map_ab, map_ba):
    the designed first-stage maps (index into the other frame, or -1)."""
    rng = np.random.default_rng([77, seed])
    ia, ib = ids
    Na, Nb = N; Ma, Mb = M
    flip = ia % 2 != ib % 2
    quarter = np.array([0.0, 0.25, 0.5, 0.75])
    ents = ([], [])                                                   # per frame: (site, slot, y, x, desc)
    for k, site in enumerate(sites):
        kind, off = site[0], site[1]
        ov = site[2] if len(site) > 2 else {}
        ca, cb = KINDS[kind]
        D = rng.integers(0, 256, 32, dtype=np.uint8)
        D2 = _flip_bits(rng, D, 60)
        if "ya" in ov and "yb" in ov:
            ya, yb = float(ov["ya"]), float(ov["yb"])
        else:
            o = float(off)
            assert o * 4 == int(o * 4) and o >= 0
            if flip:
                lo, hi = int(np.ceil(o)) + 2, min(Na, Nb + int(o)) - 2
                ya = float(ov["ya"]) if "ya" in ov else float(rng.integers(lo, hi)) + float(rng.choice(quarter))
                yb = Nb + 1 - ya + o
            else:
                ya = float(ov["ya"]) if "ya" in ov else float(rng.integers(2, min(Na, Nb) - 2)) + float(rng.choice(quarter))
                ok = [s for s in (1, -1) if 1 <= ya + s * o <= Nb - 2]
                assert ok, (k, ya, o)
                yb = ya + float(rng.choice(ok)) * o
        def xr(Mf):
            side = rng.integers(0, 2)
            return float(rng.integers(30, Mf // 2 - 30) if side == 0 else rng.integers(Mf // 2 + 30, Mf - 30))
        for slot in range(ca):
            ents[0].append((k, slot, ya, float(ov["xa"]) if "xa" in ov else xr(Ma), D if (slot == 0 or kind == "rejB2A") else D2))
        for slot in range(cb):
            ents[1].append((k, slot, yb, float(ov["xb"]) if "xb" in ov else xr(Mb), D if (slot == 0 or kind == "rejA2B") else D2))
    ns = len(sites)
    rows = (ns + PER_ROW - 1) // PER_ROW
    bb = np.array([-5.0, SPACING * (PER_ROW - 1) + 5.0, -5.0, SPACING * max(rows - 1, 0) + 5.0])
    fr, index = {}, []
    for f, (fid, Nf, Mf) in enumerate(((ia, Na, Ma), (ib, Nb, Mb))):
        e = ents[f]
        order = rng.permutation(len(e)) if shuffle else np.arange(len(e))
        e = [e[q] for q in order]
        n = len(e)
        kps = np.zeros(n, O.KP_DTYPE)
        kps["y"] = np.array([q[2] for q in e], np.float32); kps["x"] = np.array([q[3] for q in e], np.float32)
        kps["size"] = 31; kps["response"] = 50
        # every keypoint is a valid (ping, bin) for GetKpsPairs: alt[int(y)] and gr[|int(x) - M / 2|] are inside their arrays (no bin 0)
        assert n == 0 or ((kps["y"] >= 0) & (kps["y"] < Nf) & (kps["x"] >= 1) & (kps["x"] < Mf)).all()
        assert (kps["y"].astype(np.float64) == np.array([q[2] for q in e])).all()
        desc = np.array([q[4] for q in e], np.uint8).reshape(n, 32)
        site = np.array([q[0] for q in e], np.int64)
        geo = np.stack([SPACING * (site % PER_ROW), SPACING * (site // PER_ROW)], 1).astype(np.float64).reshape(n, 2) + rng.uniform(-1, 1, (n, 2))
        pose, alt, gr = tracks[fid] if tracks else H.track(Nf, Mf, fid, seed=3)
        assert pose.shape == (Nf, 6) and len(gr) == Mf // 2
        fr[fid] = dict(N=Nf, M=Mf, pose=pose, alt=alt, gr=gr, kps=kps, desc=desc, geo=np.ascontiguousarray(geo), bb=bb)
        index.append({(q[0], q[1]): i for i, q in enumerate(e)})
    map_ab = np.full(len(ents[0]), -1, np.int32); map_ba = np.full(len(ents[1]), -1, np.int32)
    for k, site in enumerate(sites):
        kind = site[0]
        A, B = index
        if kind == "mutual":
            map_ab[A[k, 0]] = B[k, 0]; map_ba[B[k, 0]] = A[k, 0]
        elif kind == "extraA":
            map_ab[A[k, 0]] = map_ab[A[k, 1]] = B[k, 0]; map_ba[B[k, 0]] = A[k, 0]
        elif kind == "extraB":
            map_ab[A[k, 0]] = B[k, 0]; map_ba[B[k, 0]] = map_ba[B[k, 1]] = A[k, 0]
        elif kind == "rejA2B":
            map_ba[B[k, 0]] = map_ba[B[k, 1]] = A[k, 0]
        elif kind == "rejB2A":
            map_ab[A[k, 0]] = map_ab[A[k, 1]] = B[k, 0]
    for f in fr.values():
        for a in f.values():
            if isinstance(a, np.ndarray): a.setflags(write=False)
    return dict(ids=ids, fr=fr, map_ab=map_ab, map_ba=map_ba)


def match_params(**kw):
    p = O.match_params()
    for k, v in kw.items(): setattr(p, k, v)
    return p


def branch_record(case, params=None, key=None):
    """what the oracle does with a pair, stage by stage: dict(d01, d10 (orc.match_dir of both directions), hist, count, model (pairs),
    img_diff, kp_diff, merge, inl, branch ("merge", 1 or 2), rows, kp7, n_phase1): the ConsistentCheck decision restated from the oracle's
    own SCC results, and held to the oracle's rows by the row count the branch must give."""
    if key is not None and ("rec", key) in _CACHE:
        return _CACHE["rec", key]
    p = params or O.match_params()
    i, j = case["ids"]
    a, b = case["fr"][i], case["fr"][j]
    d01 = O.match_dir(i, j, b["N"], a["kps"], a["desc"], a["geo"], b["kps"], b["desc"], b["geo"], b["bb"], p)
    d10 = O.match_dir(j, i, a["N"], b["kps"], b["desc"], b["geo"], a["kps"], a["desc"], a["geo"], a["bb"], p)
    rows = O.robust_matching(i, j, a["N"], b["N"], a["kps"], a["desc"], a["geo"], a["bb"], b["kps"], b["desc"], b["geo"], b["bb"], p)
    kp7 = O.get_kps_pairs(rows, j, a["alt"], a["gr"], b["alt"], b["gr"])
    img_diff = float(abs(a["N"] - b["N"])) if i % 2 != j % 2 else 0.0
    kp_diff = abs(abs(d01["scc_model"] - d10["scc_model"]) - img_diff)
    merge = d01["hist"] > 0 and d10["hist"] > 0 and kp_diff <= p.merge_thr
    c1, c2 = d01["corres"], d10["corres"]
    inl = (int((c1 != -1).sum()), int((c2 != -1).sum()))
    n_phase1 = int(sum(1 for q, m in enumerate(c1) if m != -1 and c2[m] != q))
    if merge:
        branch, want = "merge", n_phase1 + inl[1]
    elif inl[0] > inl[1]:
        branch, want = 1, inl[0]
    else:
        branch, want = 2, inl[1]
    assert len(rows) == want, "the restated ConsistentCheck decision is not the oracle's"
    rec = dict(d01=d01, d10=d10, hist=(d01["hist"], d10["hist"]), count=(d01["scc_count"], d10["scc_count"]), model=(d01["scc_model"], d10["scc_model"]),
               img_diff=img_diff, kp_diff=kp_diff, merge=merge, inl=inl, branch=branch, rows=rows, kp7=kp7, n_phase1=n_phase1)
    if key is not None:
        _CACHE["rec", key] = rec
    return rec


# ---------------------------------------------------------------- the case table: name -> (sites, keyword arguments of build_pair)
TABLE_ROW_1 = S("mutual", 300, 7) + S("extraA", 40, 7) + S("extraB", 40, 7) + S("mutual", 30, 40) + S("mutual", 20, 90.5)
PARITY_NO_MERGE = S("mutual", 300, 7) + S("extraA", 40, 7) + S("extraB", 40, 7) + S("mutual", 30, 40)
PARITY_MERGE = S("mutual", 300, 67) + S("extraA", 40, 67) + S("extraB", 40, 67) + S("mutual", 30, 100)
GRADED = [("mutual", o) for n, o in ((6, 5), (12, 25), (25, 45), (50, 65), (100, 85)) for _ in range(n)]
GRADED_SEED = 75         # fixed after a search on the CPU: tests/test_matcher_tail_cpu.py asserts hist >= 3 in both directions
# a cluster of three among 50 matches that stand alone (6 px apart: a hypothesis over two of them counts one match or none): the only hypotheses
# that count three draw both samples from the cluster, one iteration in 300.  Seeds searched on the CPU so that the first of them is iteration
# 255 (the last thread of the first stride of scc_kernel) or iteration 256 (the first thread of the second)
LATE = S("mutual", 3, 5) + [("mutual", 20 + 6 * k) for k in range(50)]
LATE_SEEDS = {"late-255": 19, "late-256": 563}
SCC_ITERS = (1, 2, 255, 256, 257, 1000)
NLOCS = (1, 2, 256, 257)

CASES = {
    # ---- 1. merged pairs
    "merge-table": (TABLE_ROW_1, {}),
    # more than 256 valid rows in EACH phase with invalid entries between them; na = 1140, nb = 1130
    "merge-long": (S("mutual", 200, 7) + S("extraA", 300, 7) + S("extraB", 290, 7) + S("mutual", 30, 40) + S("mutual", 20, 90.5), {}),
    # ---- 2. the branches without a merge
    "dir1": (S("extraA", 150, 7) + S("extraB", 100, 40), {}),
    "dir2": (S("extraA", 100, 7) + S("extraB", 150, 40), {}),
    "tie": (S("extraA", 100, 7) + S("extraB", 100, 40), {}),
    "empty-hist-1": (S("rejA2B", 50, 7), {}),
    "empty-hist-2": (S("rejB2A", 50, 7), {}),
    "empty-hist-both": (S("onlyA", 30, 7) + S("onlyB", 20, 7), {}),
    # ---- 3. merge_thr at equality: each direction has matches of its own only, so both models are designed
    "merge-thr-eq": (S("rejB2A", 60, 7) + S("rejA2B", 50, 9.5), {}),
    "merge-thr-eq-rev": (S("rejB2A", 60, 9.5) + S("rejA2B", 50, 7), {}),
    "merge-thr-above": (S("rejB2A", 60, 7) + S("rejA2B", 50, 9.75), {}),
    # ---- 4. opposite parity with different row counts, and the same parity with different row counts
    "parity-no-merge": (PARITY_NO_MERGE, dict(ids=(0, 1), N=(700, 640))),
    "parity-merge": (PARITY_MERGE, dict(ids=(0, 1), N=(700, 640))),
    "same-parity-different-rows": (S("mutual", 100, 7) + S("extraA", 40, 7) + S("extraB", 30, 7), dict(ids=(0, 2), N=(700, 640))),
    # ---- 5. SCC
    "pix-err-eq": (S("mutual", 20, 5) + S("mutual", 20, 10) + S("mutual", 3, 7.5), {}),
    "two-equal": (S("mutual", 30, 5) + S("mutual", 30, 50), {}),
    "two-equal-reversed": (S("mutual", 30, 50) + S("mutual", 30, 5), {}),
    "graded": (GRADED, dict(seed=GRADED_SEED)),
}
for _name, _seed in LATE_SEEDS.items():
    CASES[_name] = (LATE, dict(seed=_seed))
for _n in NLOCS:
    CASES["nloc-%d" % _n] = (S("mutual", _n, 7), {})


def _nadir_sites():
    """GetKpsPairs: bins at M / 2 +- 19, 20, 21 with and without a .75 fraction (truncation, not rounding) on the source side (M = 480), on the
    target side (M = 320) and on both; bins 1 and M - 1; y with .75 fractions; mixed into a merged pair of more than 256 keypoints a phase in
    which a third of the ordinary sites is nadir-rejected too, so that the kp7 offset leaves a chunk with another count than the row offset"""
    rng = np.random.default_rng(6)
    Ma, Mb = 480, 320
    edge = lambda Mf: [Mf // 2 + s * d + fr_ for s in (1, -1) for d in (19, 20, 21) for fr_ in (0.0, 0.75)] + [1.0, 1.75, Mf - 1.0, Mf - 0.25]
    sites = []
    for xa in edge(Ma): sites.append(("mutual", 7, dict(xa=xa)))
    for xb in edge(Mb): sites.append(("mutual", 7, dict(xb=xb)))
    for xa, xb in zip(edge(Ma), edge(Mb)): sites.append(("extraA", 7, dict(xa=xa, xb=xb)))
    for xa, xb in zip(edge(Ma), reversed(edge(Mb))): sites.append(("extraB", 7, dict(xa=xa, xb=xb)))
    for kind, n in (("mutual", 150), ("extraA", 150), ("extraB", 140)):
        for _ in range(n):
            ov = {}
            u = rng.integers(0, 6)
            if u == 0: ov["xa"] = float(Ma // 2 + rng.integers(-19, 20))
            if u == 1: ov["xb"] = float(Mb // 2 + rng.integers(-19, 20))
            ov["ya"] = float(rng.integers(120, 560)) + 0.75
            sites.append((kind, 7, ov))
    return [sites[q] for q in rng.permutation(len(sites))]


CASES["nadir"] = (_nadir_sites(), dict(M=(480, 320)))


SWAPPED = {"parity-no-merge-swapped": "parity-no-merge", "parity-merge-swapped": "parity-merge"}      # the same frames, source and target exchanged
NAMES = sorted(CASES) + sorted(SWAPPED)


def case(name):
    """the designed pair of a name of NAMES (built once)"""
    if ("case", name) not in _CACHE:
        if name in SWAPPED:
            c = case(SWAPPED[name])
            _CACHE["case", name] = dict(ids=c["ids"][::-1], fr=c["fr"], map_ab=c["map_ba"], map_ba=c["map_ab"])
        else:
            sites, kw = CASES[name]
            _CACHE["case", name] = build_pair(sites, **kw)
    return _CACHE["case", name]


# ---------------------------------------------------------------- 7. sticky yaw flags from the matcher's own path
STICKY_N, STICKY_M = H.LC_N, H.LC_M
RUN_A, RUN_B = (300, 303), (500, 503)             # the pings with |yaw| > 2 pi / 3 in frame A (source) and in frame B (target)
STICKY = ("src-a", "src-b", "src-c", "tgt-a", "tgt-b", "tgt-c", "both", "nadir-only", "nadir-only-tgt")


def _with_run(frame, run):
    pose = frame[0].copy(); pose[run[0]:run[1], 2] = 3.14
    return (pose, frame[1], frame[2])


def _sticky_rows(fs, ft, n, rng, s_in=None, t_in=None):
    """n geometrically consistent kp7 rows (helpers.lc_consistent_rows) of frames fs -> ft whose source ping is inside (s_in) or outside every
    run, likewise the target ping, and whose pings differ by what most rows' do (to within 1: inliers of one SCC model)"""
    inside = lambda p, run: (p >= run[0]) & (p < run[1])
    out_s = lambda p: ~inside(p, RUN_A); out_t = lambda p: ~inside(p, RUN_B)
    if s_in is not None:            # search from the target's side so that the predicate picks the source pings
        r = H.lc_consistent_rows(O, ft, fs, 8 * n, rng, t_ping=lambda p: inside(p, s_in))[:, [3, 4, 5, 0, 1, 2, 6]]
        r = r[out_t(r[:, 3].astype(int))] if t_in is None else r[inside(r[:, 3].astype(int), t_in)]
    else:
        r = H.lc_consistent_rows(O, fs, ft, 8 * n, rng, t_ping=(lambda p: inside(p, t_in)) if t_in is not None else out_t)
        r = r[out_s(r[:, 0].astype(int))]
    r = r[np.abs(r[:, 0] - r[:, 3]) <= 1]
    assert len(r) >= n, (len(r), n)
    return r[:n]


def _site(kind, row):
    return (kind, None, dict(ya=row[0], xa=row[1], yb=row[3], xb=row[4]))


def sticky_case(name):
    """One list of case 7.  Frames: legs 0 and 2 of helpers.track(700, 480, leg, seed=9) (ids 0 and 2, same heading: consistent rows have
    ps ~ pt, one SCC model near 0), yaw 3.14 on the three pings of RUN_A in the source and / or RUN_B in the target.  Keypoints in site order.
    Returns the build_pair dict + frames=(source, target) as (pose, alt, gr) + switch: the index in the kp7 list of the first row with a large
    yaw (None: there is none), and which flags ("s", "t") it sets."""
    if ("sticky", name) in _CACHE:
        return _CACHE["sticky", name]
    f0, f2 = (H.track(STICKY_N, STICKY_M, leg, seed=9) for leg in (0, 2))
    on_s = name in ("src-a", "src-b", "src-c", "both", "nadir-only"); on_t = name in ("tgt-a", "tgt-b", "tgt-c", "both", "nadir-only-tgt")
    fs = _with_run(f0, RUN_A) if on_s else f0
    ft = _with_run(f2, RUN_B) if on_t else f2
    rng = np.random.default_rng([7, STICKY.index(name)])
    lo = _sticky_rows(fs, ft, 40, rng)
    hi_s = _sticky_rows(fs, ft, 2, rng, s_in=RUN_A) if on_s else None
    hi_t = _sticky_rows(fs, ft, 2, rng, t_in=RUN_B) if on_t else None
    hi = hi_s if hi_s is not None else hi_t
    L = lambda kind, rows: [_site(kind, r) for r in rows]
    pad = lambda kind, n: S(kind, n, 7)
    if name.endswith("-a"):        # all mutual: merged, every row in phase 2; the switch sits mid-chunk
        sites = L("mutual", lo[:12]) + L("mutual", hi[:1]) + L("mutual", lo[12:24])
    elif name.endswith("-b"):      # the switch at A index 269, in the second chunk of phase 1; small-yaw rows at A indices past 512
        sites = pad("onlyA", 260) + L("extraA", lo[:4]) + L("extraA", hi[:1]) + L("extraA", lo[4:6]) + pad("onlyA", 250) + pad("onlyB", 270) + L("extraA", lo[6:12])
    elif name.endswith("-c"):      # the switch in phase 1 of a merged pair; phase 2 opens with small-yaw rows
        sites = L("extraA", lo[:3]) + L("extraA", hi[:1]) + L("extraA", lo[3:5]) + L("mutual", lo[5:15])
    elif name == "both":
        sites = L("mutual", lo[:5]) + L("mutual", hi_s[:1]) + L("mutual", lo[5:10]) + L("mutual", hi_t[:1]) + L("mutual", lo[10:15])
    else:                          # the only large-yaw row is 5 bins off nadir, on the side that has the large yaw: no kp7 row, no flag
        h = hi[0].copy(); h[1 if on_s else 4] = STICKY_M // 2 + 5
        sites = L("mutual", lo[:8]) + [_site("mutual", h)] + L("mutual", lo[8:16])
    c = build_pair(sites, ids=(0, 2), N=(STICKY_N, STICKY_N), M=(STICKY_M, STICKY_M), shuffle=False, tracks={0: fs, 2: ft})
    c["frames"] = (fs, ft)
    _CACHE["sticky", name] = c
    return c


def rows_behind_switch(large, sw):
    """how many rows follow row sw before the next row with a large yaw (or the end of the list)"""
    later = np.nonzero(np.asarray(large)[sw + 1:])[0]
    return int(later[0]) if len(later) else len(large) - sw - 1


def large_yaw(case_, kp7):
    """per kp7 row: (source ping has a large yaw, target ping has one)"""
    fs, ft = case_["frames"]
    return np.abs(fs[0][kp7[:, 0].astype(int), 2]) > YAW_THR, np.abs(ft[0][kp7[:, 3].astype(int), 2]) > YAW_THR


# ---------------------------------------------------------------- 8. many active pairs in one call
MANY_F = 26
MANY_EMPTY, MANY_APART, MANY_ALONE = 13, 7, (4, 19)      # no keypoints; a box of its own; sites nobody else has (active pairs without rows)


def many_case():
    """26 frames of 12 to 40 keypoints over 60 shared sites (N = 700, M = 480, one box for all but frame 7), every pair of them in one list:
    325 pairs, of which those with frame 13 (no keypoints) or frame 7 (disjoint explicit box) are inactive, in the middle of the list, and
    those of frames 4 and 19 (sites of their own) are active without rows.  dict(fr={id: frame}, src, tgt)"""
    if "many" in _CACHE:
        return _CACHE["many"]
    rng = np.random.default_rng(8)
    N, M, ns = 700, 480, 60
    D = rng.integers(0, 256, (ns + 40, 32), dtype=np.uint8)
    base_y = rng.integers(150, 550, ns + 40).astype(np.float64)
    base_x = np.where(rng.integers(0, 2, ns + 40) == 0, rng.integers(30, 200, ns + 40), rng.integers(280, 450, ns + 40)).astype(np.float64)
    bb = np.array([-5.0, SPACING * (PER_ROW - 1) + 5.0, -5.0, SPACING * 2 + 5.0])
    fr = {}
    for f in range(MANY_F):
        n = 0 if f == MANY_EMPTY else int(rng.integers(12, 41))
        if f in MANY_ALONE:
            n = 20; site = ns + 20 * MANY_ALONE.index(f) + np.arange(20)
        else:
            site = rng.choice(ns, n, replace=False)
        kps = np.zeros(n, O.KP_DTYPE)
        kps["y"] = (base_y[site] + rng.integers(-1, 2, n) + rng.choice([0.0, 0.25, 0.5, 0.75], n)).astype(np.float32)
        kps["x"] = (base_x[site] + rng.integers(-3, 4, n)).astype(np.float32)
        kps["size"] = 31; kps["response"] = 50
        desc = D[site].copy().reshape(n, 32)
        for q in range(n): desc[q] = _flip_bits(rng, desc[q], int(rng.integers(0, 9)))
        geo = np.stack([SPACING * (site % PER_ROW), SPACING * (site // PER_ROW)], 1).astype(np.float64).reshape(n, 2) + rng.uniform(-1, 1, (n, 2))
        box = bb
        if f == MANY_APART:
            geo = geo + np.array([5000.0, 0.0]); box = bb + np.array([5000.0, 5000.0, 0.0, 0.0])
        pose, alt, gr = H.track(N, M, f % 4, seed=3)
        fr[f] = dict(N=N, M=M, pose=pose, alt=alt, gr=gr, kps=kps, desc=desc, geo=np.ascontiguousarray(geo), bb=box)
    pairs = [(i, j) for i in range(MANY_F) for j in range(i + 1, MANY_F)]
    pairs = [pairs[q] for q in rng.permutation(len(pairs))]
    pairs = [(j, i) if rng.integers(0, 4) == 0 else (i, j) for i, j in pairs]      # a quarter of them with the larger id as the source
    _CACHE["many"] = dict(fr=fr, src=[p[0] for p in pairs], tgt=[p[1] for p in pairs])
    return _CACHE["many"]


def many_active(c, i, j):
    a, b = c["fr"][i], c["fr"][j]
    disjoint = a["bb"][1] < b["bb"][0] or b["bb"][1] < a["bb"][0] or a["bb"][3] < b["bb"][2] or b["bb"][3] < a["bb"][2]
    return not (disjoint or len(a["kps"]) == 0 or len(b["kps"]) == 0)

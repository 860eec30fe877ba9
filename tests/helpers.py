"""shared builders for the parity tests (seeded, small)"""
import ctypes

import numpy as np
from oracle import binding as O


def track(N, M, leg, res=0.05, spacing=None, seed=0):
    """DR pose / altitude / ground range of one straight leg (even legs head +x, odd legs -x)"""
    rng = np.random.default_rng(1000 + seed + leg)
    half = M // 2
    gr = res * np.arange(half, dtype=np.float64)
    spacing = spacing if spacing is not None else 0.39 * 2 * half * res
    s = (np.arange(N) + 0.5) * res
    fwd = leg % 2 == 0
    pose = np.zeros((N, 6))
    pose[:, 2] = (0.0 if fwd else 3.14159265359) + 0.002 * rng.standard_normal()
    pose[:, 3] = (s if fwd else N * res - s) + 0.01 * rng.standard_normal(N).cumsum() * 0.1
    pose[:, 4] = leg * spacing + 0.02 * np.sin(s)
    alt = 9.0 + np.sin(s / 7.0)
    return pose, alt, gr


def random_features(N, M, n, seed, margin=100):
    """n keypoints with integer level-0-like coordinates and random descriptors"""
    rng = np.random.default_rng(seed)
    kps = np.zeros(n, O.KP_DTYPE)
    kps["y"] = rng.integers(margin, N - margin, n).astype(np.float32) + rng.choice([0.0, 0.25, 0.5], n).astype(np.float32)
    xs = rng.integers(margin // 2, M - margin // 2, n)
    kps["x"] = xs.astype(np.float32)
    kps["size"] = 31; kps["angle"] = rng.uniform(0, 360, n).astype(np.float32); kps["response"] = rng.integers(7, 200, n)
    kps["octave"] = rng.integers(0, 6, n)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    return kps, desc


def paired_features(N, M, n, seed, flip_bits=12, reverse=False, margin=100):
    """frame A random; frame B sees the same 'landmarks' (descriptor + a few flipped bits) at the image position
    that maps to (almost) the same geo point when B runs the neighbouring leg"""
    rng = np.random.default_rng(seed + 7)
    ka, da = random_features(N, M, n, seed, margin)
    kb = ka.copy(); db = da.copy()
    for i in range(n):
        bits = rng.choice(256, rng.integers(0, flip_bits + 1), replace=False)
        for b in bits:
            db[i, b // 8] ^= np.uint8(1 << (b % 8))
    return ka, da, kb, db


# ---------------------------------------------------------------- hard cases of the loop-closure and triangulation LMs
LC_N, LC_M = 700, 480
_LC_CACHE = {}          # lc_cases by seed and oracle references by (group, list): computed once per session, arrays read-only, results never edited


def lc_bin_ok(b, M=LC_M):
    """bins the library's range check admits and GetKpsPairs can emit: [1, M) and at least 20 off nadir"""
    b = np.asarray(b)
    return (b >= 1) & (b < M) & (np.abs(b - M // 2) >= 20)


def lc_slant(frame, ping, b, M=LC_M):
    pose, alt, gr = frame
    return np.sqrt(alt[ping] ** 2 + gr[abs(int(b) - M // 2)] ** 2)


class _Geo:
    """geo image of a frame (orc.geo_img) with a nearest-point search over the admissible bins"""

    _made = {}

    @classmethod
    def of(cls, orc, frame):
        """one search tree per frame object (a tree costs 0.3 s and lc_cases asks for the same three frames a dozen times).  The key is the id
        of the frame's pose array; the entry holds the frame itself, so that the array stays alive and its id cannot be handed to another one."""
        k = id(frame[0])
        if k not in cls._made:
            cls._made[k] = (frame, cls(orc, frame))
        return cls._made[k][1]

    def __init__(self, orc, frame, M=LC_M):
        from scipy.spatial import cKDTree
        self.gx, self.gy = orc.geo_img(frame[0], frame[2], M)
        ok = lc_bin_ok(np.arange(M), M)
        self.cols = np.nonzero(ok)[0]
        pts = np.stack([self.gx[:, ok].ravel(), self.gy[:, ok].ravel()], 1)
        self.tree = cKDTree(pts)

    def nearest(self, x, y):
        d, k = self.tree.query(np.stack([np.atleast_1d(x), np.atleast_1d(y)], 1))
        return d, k // len(self.cols), self.cols[k % len(self.cols)]


def _row(fs, ft, ps, bs, pt, bt):
    return [ps, bs, lc_slant(fs, ps, bs), pt, bt, lc_slant(ft, pt, bt), 0.0]


def lc_consistent_rows(orc, fs, ft, n, rng, max_dist=0.05, t_ping=None, geo_t=None, s_ping=None):
    """n kp7 rows that see one ground point from both frames: a random source ping / bin, the target ping / bin whose geo point is
    nearest (within max_dist), slant ranges from altitude and ground range.  t_ping, s_ping: optional predicates on the target / source ping."""
    gs = _Geo.of(orc, fs); gt = geo_t or _Geo.of(orc, ft)
    N = len(fs[0])
    rows = []
    for _ in range(20):
        ps = rng.integers(0, N, 4000); bs = rng.choice(gs.cols, 4000)
        d, pt, bt = gt.nearest(gs.gx[ps, bs], gs.gy[ps, bs])
        keep = d <= max_dist
        if t_ping is not None:
            keep &= t_ping(pt)
        if s_ping is not None:
            keep &= s_ping(ps)
        for k in np.nonzero(keep)[0]:
            rows.append(_row(fs, ft, int(ps[k]), int(bs[k]), int(pt[k]), int(bt[k])))
            if len(rows) == n:
                return np.array(rows)
    raise AssertionError("only %d of %d consistent rows found" % (len(rows), n))


def lc_cases(orc, seed=0):
    """Named groups of kp7 lists that drive the mini-LM (and the triangulation LM) through every exit it has.
    Returns {name: dict(frames=[(pose, alt, gr), ...], lists=[(src slot, tgt slot, kp7 (n x 7, n <= 64)), ...])}; frames come from
    track(700, 480, leg, seed=9).  Every row passes the library's range check (ping in [0, N), bin in [1, M), |bin - M/2| >= 20)."""
    if seed in _LC_CACHE:
        return _LC_CACHE[seed]
    N, M, n = LC_N, LC_M, 40
    sub = lambda i: np.random.default_rng([4000 + seed, i])          # a stream per group: changing one group leaves the others as they are
    rng = sub(0)
    f0, f1, f2 = (track(N, M, leg, seed=9) for leg in range(3))
    r01 = lc_consistent_rows(orc, f0, f1, n, rng)
    r02 = lc_consistent_rows(orc, f0, f2, n, rng)
    r12 = lc_consistent_rows(orc, f1, f2, n, rng)
    G = {}
    G["consistent-opposite"] = dict(frames=[f0, f1], lists=[(0, 1, r01)])
    G["consistent-same"] = dict(frames=[f0, f1, f2], lists=[(0, 2, r02)])
    rng = sub(1)
    noisy = r01.copy(); noisy[:, 2] += rng.normal(0, 20, n); noisy[:, 5] += rng.normal(0, 20, n)
    G["noisy-slant"] = dict(frames=[f0, f1], lists=[(0, 1, noisy)])
    p22 = f1[0].copy(); p22[:, 2] = 2.2                                # over 2 pi / 3: flipped, but the heading is not the reverse
    # (64 rows of their own: one row in twenty of this group runs into the 100-iteration cap, and three of them are wanted)
    G["wrong-flip"] = dict(frames=[f0, (p22, f1[1], f1[2])], lists=[(0, 1, lc_consistent_rows(orc, f0, f1, 64, sub(7)))])
    tiny = r01.copy(); tiny[:, 2] = 1e-3
    G["tiny-slant"] = dict(frames=[f0, f1], lists=[(0, 1, tiny)])
    long_ = r01.copy(); long_[:, 5] *= 3
    G["long-slant"] = dict(frames=[f0, f1], lists=[(0, 1, long_)])
    zero = r01.copy(); zero[:, 2] = 0.0
    G["zero-slant"] = dict(frames=[f0, f1], lists=[(0, 1, zero)])
    # target = the source frame again in another slot: the baseline between a ping and its copy is exactly zero, so sig_odo[3], sig_odo[4] and
    # the triangulation's sig_p[2] sit on their 1e-9 clamps.  The nearest target point of a source ping / bin is that same ping / bin; with it
    # both sss factors see the landmark from one pose along one ray, its 3 x 3 block of the information matrix has rank 2, and whether the
    # marginal's Cholesky finds the third pivot positive is settled by rounding alone; ini = 0 exactly, so the score is 0 / fin - 2: NaN
    # when fin = 0 too, -2 otherwise.  Measured on 256 random rows of this kind: 66 % are knife-edge by lc_reference's one-ulp test, every
    # row with a non-finite score among them (moving the target's x makes ini > 0), and no variant of the group tried (copy shifted by
    # 1e-10 m in x or y, by 1 m in z) brings the share under 40 %.  The same ping seen 10 bins further out IS decided by the oracle (256
    # of 256 path-stable, variances finite, clamps active).  The group is therefore 58 rows of the second kind and 6 of the first, all random,
    # none looked at: at most 6 of 64 can be knife-edge, and those 6 carry the NaN variances and the NaN scores of the group.
    f0c = tuple(a.copy() for a in f0)
    rng = sub(2)
    adm = np.nonzero(lc_bin_ok(np.arange(M)))[0]
    zb = []
    for i in range(64):
        p = int(rng.integers(0, N)); b = int(rng.choice(adm))
        same = i % 10 == 5
        bt = b if same else (b + 10 if b + 10 < M and lc_bin_ok(b + 10) else b - 10)
        zb.append(_row(f0, f0c, p, b, p, bt))
    zb = np.array(zb)
    zb_same = np.arange(64) % 10 == 5
    G["zero-baseline"] = dict(frames=[f0, f0c], lists=[(0, 1, zb)], same_point=zb_same)
    rng = sub(3)
    pt_ = f0[0].copy(); pt_[:, 0] = 0.3; pt_[:, 1] = -0.2
    ft_ = (pt_, f0[1], f0[2])
    G["tilted"] = dict(frames=[ft_, f1], lists=[(0, 1, lc_consistent_rows(orc, ft_, f1, n, rng))])
    # sticky flip switching on in the middle of a list: target yaw 0.5 below N / 2 (no flip), 2.5 above (flip); after the first row
    # above the threshold come rows with the small yaw again, which stay flipped (optimizer.cpp:650,700-703)
    rng = sub(4)
    pm = f1[0].copy(); pm[:, 2] = np.where(np.arange(N) < N // 2, 0.5, 2.5)
    fm = (pm, f1[1], f1[2]); gm = _Geo.of(orc, fm)
    lo = lc_consistent_rows(orc, f0, fm, 20, rng, t_ping=lambda p: p < N // 2, geo_t=gm)
    hi = lc_consistent_rows(orc, f0, fm, 4, rng, t_ping=lambda p: p >= N // 2, geo_t=gm)
    G["mid-list-flip"] = dict(frames=[f0, fm], lists=[(0, 1, np.concatenate([lo[:12], hi[:1], lo[12:], hi[1:]]))], switch=12)
    # the same with the yaw step on the SOURCE frame (flag bit 0): 24 rows, switch at row 12
    rng = sub(8)
    ps_ = f0[0].copy(); ps_[:, 2] = np.where(np.arange(N) < N // 2, 0.5, 2.5)
    fms = (ps_, f0[1], f0[2])
    lo = lc_consistent_rows(orc, fms, f1, 20, rng, s_ping=lambda p: p < N // 2)
    hi = lc_consistent_rows(orc, fms, f1, 4, rng, s_ping=lambda p: p >= N // 2)
    G["mid-list-flip-src"] = dict(frames=[fms, f1], lists=[(0, 1, np.concatenate([lo[:12], hi[:1], lo[12:], hi[1:]]))], switch=12)
    # the borders the range check admits, on the source side and on the target side; the partner is the nearest admissible point
    rng = sub(5)
    g0, g1 = _Geo.of(orc, f0), _Geo.of(orc, f1)
    edge = []
    for b in (1, M - 1, M // 2 - 20, M // 2 + 20):
        for p in rng.integers(0, N, 3):
            _, pt, bt = g1.nearest(g0.gx[p, b], g0.gy[p, b]); edge.append(_row(f0, f1, int(p), b, int(pt[0]), int(bt[0])))
            _, pq, bq = g0.nearest(g1.gx[p, b], g1.gy[p, b]); edge.append(_row(f0, f1, int(pq[0]), int(bq[0]), int(p), b))
    for p in (0, N - 1):
        for b in rng.choice(g0.cols, 3):
            _, pt, bt = g1.nearest(g0.gx[p, b], g0.gy[p, b]); edge.append(_row(f0, f1, p, int(b), int(pt[0]), int(bt[0])))
            _, pq, bq = g0.nearest(g1.gx[p, b], g1.gy[p, b]); edge.append(_row(f0, f1, int(pq[0]), int(bq[0]), p, int(b)))
    G["edges"] = dict(frames=[f0, f1], lists=[(0, 1, np.array(edge))])
    # lists that do not fill a wavefront (four problems each)
    G["ragged"] = dict(frames=[f0, f1, f2], lists=[(0, 1, noisy[:1]), (0, 1, r01[3:5]), (0, 2, r02[:3]),
                                                   (0, 1, np.concatenate([tiny[5:7], zero[7:9], long_[9:10]])),
                                                   (0, 2, np.concatenate([r02[10:14], r02[20:23] * [1, 1, 1, 1, 1, 3, 1]]))])
    # one launch over pairs with different frames and flip flags, an empty list, a reversed pair; every wavefront straddles two pairs
    r21 = r12[:, [3, 4, 5, 0, 1, 2, 6]]
    t12 = r12[5:10].copy(); t12[3:, 2] = 1e-3
    G["pairs"] = dict(frames=[f0, f1, f2], lists=[(0, 1, noisy[10:13]), (0, 2, r02[:0]), (1, 2, t12), (2, 1, r21[20:21]),
                                                  (0, 1, np.concatenate([r01[20:22], zero[22:24], long_[24:26], noisy[26:27]]))])
    # what a survey with bad matches hands to the selection: frame 2 is a copy of frame 0 (zero baseline against it).  The good rows see a
    # point that dead reckoning puts 0.5 m further along the track in the target frame: the mini-LM closes that gap, the score is positive
    # and the row becomes an edge (rows built from the DR poses themselves have nothing to gain and score below 0).
    rng = sub(6)
    def shifted(fs, ft, n):
        gs, gt = _Geo.of(orc, fs), _Geo.of(orc, ft)
        rows = []
        while len(rows) < n:
            p = int(rng.integers(0, N)); b = int(rng.choice(gs.cols))
            d, pt, bt = gt.nearest(gs.gx[p, b] + 0.5, gs.gy[p, b])
            if d[0] <= 0.05:
                rows.append(_row(fs, ft, p, b, int(pt[0]), int(bt[0])))
        return np.array(rows)
    s01 = shifted(f0, f1, 24); z01 = s01.copy(); z01[:, 2] = 0.0
    s12 = shifted(f1, f0c, 12)
    zsel = np.concatenate([zb[:9], zb[zb_same][1:3], zb[9:18], zb[zb_same][3:]])[:24]          # all six same-point rows among 24
    G["select"] = dict(frames=[f0, f1, f0c], lists=[(0, 1, np.concatenate([s01[:12], z01[12:18], s01[18:]])), (0, 2, zsel), (1, 2, s12)])
    for g in G.values():
        for s, t, k in g["lists"]:
            assert k.shape[1] == 7 and len(k) <= 64
            assert ((k[:, 0] >= 0) & (k[:, 0] < N) & (k[:, 3] >= 0) & (k[:, 3] < N) & lc_bin_ok(k[:, 1]) & lc_bin_ok(k[:, 4])).all()
            k.setflags(write=False)                          # the groups are shared by every test of a session: nobody edits them in place
        for f in g["frames"]:
            for a in f:
                a.setflags(write=False)
    _LC_CACHE[seed] = G
    return G


def lc_long_flip_list(orc):
    """65 rows over the frames of lc_cases' mid-list-flip group: more than one block of tri_kernel (64 problems).  The target's yaw crosses
    2 pi / 3 at row 63, the last of the first block; row 64, the only one of the second block, has the small yaw again and is flipped only
    because the flag is sticky over the whole list.  dict(frames, list=(0, 1, kp7), switch=63)"""
    if "long-flip" not in _LC_CACHE:
        g = lc_cases(orc, 0)["mid-list-flip"]
        f0, fm = g["frames"]
        rng = np.random.default_rng([4000, 9]); gm = _Geo.of(orc, fm)
        lo = lc_consistent_rows(orc, f0, fm, 64, rng, t_ping=lambda p: p < LC_N // 2, geo_t=gm)
        hi = lc_consistent_rows(orc, f0, fm, 1, rng, t_ping=lambda p: p >= LC_N // 2, geo_t=gm)
        k = np.concatenate([lo[:63], hi, lo[63:]]); k.setflags(write=False)
        _LC_CACHE["long-flip"] = dict(frames=g["frames"], list=(0, 1, k), switch=63)
    return _LC_CACHE["long-flip"]


LC_SEAM_N = 1400
LC_SEAM_RESIDUES = (0, 63, 64, 255)
LC_SEAM_POSES = (4095, 4096, 4097, 4199)


def lc_seam_case(orc):
    """Loop closures whose target poses sit on the seams of the ordered compaction behind dsss_posegraph_select (blocks of 4096 poses scanned
    in chunks of 256 by wavefronts of 64).  Three frames track(1400, LC_M, leg, seed=9): 4 200 pings, more than one block and no multiple of
    256.  Wanted are the global poses g >= 1400 with g mod 256 in LC_SEAM_RESIDUES, plus LC_SEAM_POSES; every pair (0,1), (0,2), (1,2) whose
    target frame holds a wanted pose gets two rows for it, built like `shifted` of lc_cases: the source point whose image 0.5 m further
    along the track is nearest to a point of the wanted target ping, within 0.05 m (such a row scores above 0 and becomes an edge).
    Returns dict(frames, lists, wanted, lcs, edges): lcs and edges are the oracle's (orc_lc_solve per list, orc_pg_select_lc)."""
    if "seam" in _LC_CACHE:
        return _LC_CACHE["seam"]
    N, M = LC_SEAM_N, LC_M
    frames = [track(N, M, leg, seed=9) for leg in range(3)]
    geo = [_Geo(orc, f) for f in frames]
    wanted = sorted({g for g in range(N, 3 * N) if g % 256 in LC_SEAM_RESIDUES} | set(LC_SEAM_POSES))
    rng = np.random.default_rng(5)
    lists = []
    for s, t in ((0, 1), (0, 2), (1, 2)):
        gs, gt = geo[s], geo[t]
        rows = []
        for g in wanted:
            if g // N != t:
                continue
            pt, found = g - t * N, 0
            for _ in range(200):
                bt = int(rng.choice(gt.cols))                       # a point of the wanted ping, and the source point that lands on it
                _, p, b = gs.nearest(gt.gx[pt, bt] - 0.5, gt.gy[pt, bt])
                d, pt2, bt2 = gt.nearest(gs.gx[p[0], b[0]] + 0.5, gs.gy[p[0], b[0]])
                if d[0] <= 0.05 and int(pt2[0]) == pt:
                    rows.append(_row(frames[s], frames[t], int(p[0]), int(b[0]), pt, int(bt2[0])))
                    found += 1
                    if found == 2:
                        break
            assert found == 2, (s, t, g)
        lists.append((s, t, np.array(rows)))
    lcs = [orc.lc_solve(k, *frames[s], M, *frames[t], M) for s, t, k in lists]
    off = np.cumsum([0] + [len(l[2]) for l in lists])
    edges = orc.pg_select_lc([N] * 3, [l[0] for l in lists], [l[1] for l in lists], off, np.concatenate([l[2] for l in lists]), np.concatenate(lcs))
    for a in [x for f in frames for x in f] + [l[2] for l in lists] + lcs + [edges]:
        a.setflags(write=False)
    _LC_CACHE["seam"] = dict(frames=frames, lists=lists, wanted=wanted, lcs=lcs, edges=edges)
    return _LC_CACHE["seam"]


def _spread(stack):
    """largest difference among the runs, element-wise (NaN where every run is NaN counts as 0)"""
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            d = np.nanmax(stack, 0) - np.nanmin(stack, 0)
    return np.where(np.isfinite(d), d, 0.0)


def _nonfinite_code(a):
    """0 finite, 1 NaN, 2 +inf, 3 -inf"""
    a = np.asarray(a)
    return np.where(np.isnan(a), 1, np.where(np.isposinf(a), 2, np.where(np.isneginf(a), 3, 0)))


def _neighbours(kp7, pose_t):
    """the row itself and its six one-ulp neighbours: both slant ranges and the target pings' x, each up and down"""
    yield kp7, pose_t
    for col in (2, 5):
        for to in (np.inf, -np.inf):
            k = kp7.copy(); k[:, col] = np.nextafter(k[:, col], to); yield k, pose_t
    for to in (np.inf, -np.inf):
        p = pose_t.copy(); p[:, 3] = np.nextafter(p[:, 3], to); yield kp7, p


def lc_reference(orc, frames, s, t, kp7, key=None):
    """The oracle on one list, and what the oracle itself can say about every row: its trace, whether its path survives a one-ulp move
    of the inputs (path-stable: same iteration count, counters and non-finite pattern in all seven runs) and, per output element, the
    spread among the seven.  Decided on the oracle alone.  dict(lcs, trace, stable, spread={rel, var, err1, score})"""
    if key is not None and ("lc", key) in _LC_CACHE:
        return _LC_CACHE[("lc", key)]
    (ps, as_, gs), (pt, at, gt) = frames[s], frames[t]
    runs = [orc.lc_solve_trace(k, ps, as_, gs, LC_M, p, at, gt, LC_M) for k, p in _neighbours(np.asarray(kp7, np.float64), pt)]
    lcs, tr = runs[0]
    stable = np.ones(len(lcs), bool)
    for l2, t2 in runs[1:]:
        for c in orc.TRACE_COUNTERS:
            stable &= t2[c] == tr[c]
        for f in ("rel", "var", "score", "err1"):
            same = _nonfinite_code(l2[f]) == _nonfinite_code(lcs[f])
            stable &= same.reshape(len(lcs), -1).all(1)
    spread = {f: _spread(np.stack([r[0][f] for r in runs])) for f in ("rel", "var", "err1", "score")}
    out = dict(lcs=lcs, trace=tr, stable=stable, spread=spread)
    if key is not None:
        _LC_CACHE[("lc", key)] = out
    return out


def tri_reference(orc, frames, s, t, kp7, key=None):
    """lc_reference for orc_triangulate: dict(out (n x 7), trace, stable, spread (n x 7))"""
    if key is not None and ("tri", key) in _LC_CACHE:
        return _LC_CACHE[("tri", key)]
    (ps, as_, gs), (pt, at, gt) = frames[s], frames[t]
    runs = [orc.triangulate_trace(k, ps, as_, gs, LC_M, p, at, gt, LC_M) for k, p in _neighbours(np.asarray(kp7, np.float64), pt)]
    out, tr = runs[0]
    stable = np.ones(len(out), bool)
    for o2, t2 in runs[1:]:
        for c in orc.TRACE_COUNTERS:
            stable &= t2[c] == tr[c]
        stable &= (_nonfinite_code(o2) == _nonfinite_code(out)).all(1)
    res = dict(out=out, trace=tr, stable=stable, spread=_spread(np.stack([r[0] for r in runs])))
    if key is not None:
        _LC_CACHE[("tri", key)] = res
    return res


# ---------------------------------------------------------------- results as bytes
def result_bytes(x):
    """the bytes of a result: arrays (NaNs compare as their bits), scalars, nested tuples and lists"""
    if isinstance(x, (tuple, list)):
        return b"|".join(result_bytes(v) for v in x)
    return np.ascontiguousarray(x).tobytes() if x is not None else b"none"


def first_difference(a, b, where="result"):
    """None when two nested results have the same bytes (result_bytes), else the path of the first leaf that differs with what differs
    there: "result[3][0]: 2 of 4800 bytes differ, first at byte 17".  One flipped bit anywhere is reported; NaNs count by their bits."""
    if isinstance(a, (tuple, list)) or isinstance(b, (tuple, list)):
        if not (isinstance(a, (tuple, list)) and isinstance(b, (tuple, list))):
            return "%s: a %s against a %s" % (where, type(a).__name__, type(b).__name__)
        if len(a) != len(b):
            return "%s: %d items against %d" % (where, len(a), len(b))
        for k, (u, v) in enumerate(zip(a, b)):
            d = first_difference(u, v, "%s[%d]" % (where, k))
            if d is not None:
                return d
        return None
    x, y = result_bytes(a), result_bytes(b)
    if x == y:
        return None
    if len(x) != len(y):
        return "%s: %d bytes against %d" % (where, len(x), len(y))
    u = np.frombuffer(x, np.uint8); v = np.frombuffer(y, np.uint8)
    bad = np.nonzero(u != v)[0]
    return "%s: %d of %d bytes differ, first at byte %d (0x%02x against 0x%02x)" % (where, len(bad), len(x), bad[0], u[bad[0]], v[bad[0]])


# ---------------------------------------------------------------- small inputs shared by several GPU test modules
MOSAIC_SIZES = ((640, 400), (500, 700))          # the two legs of the mosaic tests: the smallest sizes test_gpu_extract.py extracts at


def survey_frame(N, M, seed, hot=True):
    """raw image and DR inputs of frame 1 of a two-frame synthetic survey (the extraction tests' frame)"""
    from diasss_amd.synth import Survey
    sv = Survey(2, N, M, seed=seed)
    raw = sv.frame(1).numpy().copy()
    if hot:   # a few "sensor buggy line" pixels inside the valid area (frame.cpp:98-103)
        rng = np.random.default_rng(seed)
        for _ in range(5):
            raw[rng.integers(160, N - 160), rng.integers(100, M - 100)] = 4.0 * raw.mean()
        raw[200, 150] = 3.0 * raw.mean()
    pose, alt, gr = sv.inputs(1)
    return raw, pose, alt, gr


def pg_edge(orc, dr, a, b, dy, var=(1e-6, 1e-6, 1e-5, 1e-3, 0.5, 1e-2)):
    e = np.zeros(1, orc.LCEDGE_DTYPE)
    e["a"] = a; e["b"] = b
    Ta, Tb, Tr = orc.Pose(), orc.Pose(), orc.Pose()
    orc.lib().orc_pose_from_rodrigues(orc.dp(np.ascontiguousarray(dr[a])), ctypes.byref(Ta))
    orc.lib().orc_pose_from_rodrigues(orc.dp(np.ascontiguousarray(dr[b])), ctypes.byref(Tb))
    orc.lib().orc_pose_between(ctypes.byref(Ta), ctypes.byref(Tb), ctypes.byref(Tr))
    rel = np.concatenate([np.array(Tr.R), np.array(Tr.t)]); rel[10] += dy
    e["rel"][0] = rel; e["var"][0] = var
    return e


def pg_small_graph(orc):
    """the 300-pose chain of test_posegraph_edges_api_small_cases with its 9-edge case: duplicates, reversed edges, neighbouring poses"""
    n = 300
    dr = np.zeros((n, 6)); dr[:, 3] = 0.05 * np.arange(n); dr[:, 2] = 0.01 * np.sin(np.arange(n) / 30.0)
    dr[150:, 2] += 3.14159265359; dr[150:, 4] += 5.0; dr[150:, 3] = dr[149, 3] - 0.05 * np.arange(150)
    spec = [(240, 60, 0.08), (10, 290, 0.2), (60, 240, -0.1), (290, 10, 0.22), (10, 290, 0.25), (60, 240, -0.05), (149, 150, 0.05),
            (150, 149, -0.02), (10, 290, 0.21)]
    return dr, np.concatenate([pg_edge(orc, dr, a, b, dy) for a, b, dy in spec])

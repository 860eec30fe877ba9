"""Cases and references for the device probe (diasss_amd/host/dev_probe.hip): the kernels' shared __device__ helpers evaluated on the GPU one
function at a time.  Shared by tests/test_dev_probe_cpu.py and tests/test_gpu_dev_probe.py.

  * the records of function ids 0-11 are the ones tests/test_pose_algebra_cpu.py::_records makes from tests/golden/pose_algebra.npz, plus
    pose_rpy at and next to gimbal lock;
  * the 50-digit references the pose fixture does not hold are in a second fixture, tests/golden/dev_probe.npz (python -m tests.dev_probe_ref
    writes it): pose_rpy on every log case and the gimbal cases, pose_retract on the interior log classes x the exp classes, sss_factor;
    per class the floor F = max |oracle - reference| is stored with them, as in the pose fixture;
  * everything else is compared bit for bit, with the oracle or with a literal numpy restatement, and needs no fixture: the case lists
    (dsss_sincos, fast_atan2_dev, dsss_geo_at, factor_eval, chol6_*, the scans, the LM table) are made here from fixed seeds.

The upper part needs numpy alone; mpmath is imported where a 50-digit number is made."""
import ctypes as C
import math
import os

import numpy as np

from tests import pose_algebra_ref as P

EPS = P.EPS
SEED = 20261021
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dev_probe.npz")
IN_W, OUT_W = 64, 48
F_SSS, F_SINCOS, F_GEO, F_ATAN2, F_FACTOR, F_CHOL_RECIP, F_CHOL_RDIAG, F_LM = range(12, 20)
SINCOS_PER_REC, ATAN2_PER_REC = 24, 31
NAMES = ["so3_exp", "so3_log", "pose_exp", "pose_log", "pose_between", "pose_inverse", "pose_compose", "pose_adjoint", "pose_retract",
         "pose_rpy", "pose_from_rodrigues", "edge error", "sss_factor", "dsss_sincos", "dsss_geo_at", "fast_atan2_dev", "factor_eval",
         "chol6_recip", "chol6_rdiag", "lm rule"]

RPY_GIMBAL = len(P.LOG_CLASSES)                      # class ids of the rpy floors: the log classes, then the gimbal cases
RPY_CLASS_NAMES = [c for c, _ in P.LOG_CLASSES] + ["rpy_gimbal"]
RETRACT_CLASS_NAMES = [c for c, _ in P.EXP_CLASSES]  # a retract case is in the class of its tangent
SSS_CLASS_NAMES = ["sss_range", "sss_two_ulp", "sss_zero"]
SSS_RANGES = [0.5, 2.0, 10.0, 50.0, 150.0]
SSS_POSES = 8


# ------------------------------------------------------------------ pose_rpy at and next to gimbal lock
def gimbal_cases():
    """R20 = +-1 with R21 = R22 = +-0 (both signs of each zero, and of the two zeros yaw is made of), R20 one ulp inside and outside +-1
    with the same zeros, and one ulp inside with the R21, R22 of size sqrt(1 - R20^2) a rotation would have -> n x 12"""
    out = []
    z = (0.0, -0.0)
    for s in (1.0, -1.0):
        for r20 in (s, s * (1.0 - EPS / 2), s * (1.0 + EPS)):
            for r21 in z:
                for r22 in z:
                    for r10, r00 in ((0.0, 0.0), (-0.0, -0.0), (0.0, -0.0), (-0.0, 0.0)):
                        # the rows a rotation with pitch -+pi/2 has: R = [0 a b; 0 c d; -+1 0 0] with a 2 x 2 rotation block
                        out.append([r00, 0.6, 0.8, r10, -0.8 * s, 0.6 * s, r20, r21, r22, 1.0, 2.0, 3.0])
        h = math.sqrt(EPS)                            # 1.49e-8 = sqrt(1 - (1 - eps / 2)^2)
        for a in (0.3, 2.0, -1.2, -2.8):
            out.append([h * 0.5, 0.6, 0.8, -h * 0.5, -0.8 * s, 0.6 * s, s * (1.0 - EPS / 2), h * math.sin(a), h * math.cos(a), 1.0, 2.0, 3.0])
    return np.array(out, np.float64)


def gimbal_kind(T):
    """0: |R20| == 1 and R21 = R22 = 0; 1: one ulp inside; 2: one ulp outside"""
    a = abs(float(T[6]))
    return 0 if a == 1.0 else 1 if a == 1.0 - EPS / 2 else 2 if a == 1.0 + EPS else -1


# ------------------------------------------------------------------ retract: which pose meets which tangent
def retract_index(fx):
    """the log cases of the interior classes, each with the tangent _records pairs it with -> (indices into log_T, indices into exp_xi)"""
    ids = [P.CLASS_ID[c] for c in P.INTERIOR]
    i = np.flatnonzero(np.isin(fx["log_class"], ids))
    return i, i % len(fx["exp_xi"])


# ------------------------------------------------------------------ sss_factor
def sss_cases():
    """-> (in17 [p(3) T(12) mx my], class ids, slant range |p - T.t| in double).  Tilted poses (roll, pitch up to 0.3 rad, any yaw) at
    coordinates of a kilometre; slant ranges 0.5 ... 150 m with mx next to the range (nrm - mx cancels) and my next to the across-track
    component; p two ulps from T.t in one coordinate or in all three; p == T.t."""
    rng = np.random.default_rng(SEED)
    rows, cls = [], []
    poses = []
    for _ in range(SSS_POSES):
        rv = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(-math.pi, math.pi)])
        th = np.linalg.norm(rv); k = rv / th
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)
        t = rng.uniform(-1000.0, 1000.0, 3)
        poses.append(np.concatenate([R.ravel(), t]))
    for T in poses:
        R, t = T[:9].reshape(3, 3), T[9:]
        for r in SSS_RANGES:
            u = rng.normal(size=3); u /= np.linalg.norm(u)
            p = t + R @ (u * r)
            rows.append(np.concatenate([p, T, [r, u[0] * r + rng.uniform(-0.01, 0.01)]])); cls.append(0)
    for T in poses:
        t = T[9:]
        for pat in ((2, 0, 0), (0, -2, 0), (0, 0, 2), (2, -2, 2)):
            p = t.copy()
            for a, steps in enumerate(pat):
                for _ in range(abs(steps)): p[a] = np.nextafter(p[a], np.inf if steps > 0 else -np.inf)
            rows.append(np.concatenate([p, T, [0.0, 0.0]])); cls.append(1)
    for T in poses[:4]:
        rows.append(np.concatenate([T[9:], T, [1.5, -0.25]])); cls.append(2)
    rows = np.array(rows, np.float64)
    return rows, np.array(cls, np.int16), np.sqrt(((rows[:, :3] - rows[:, 12:15]) ** 2).sum(axis=1))


def sss_floor_figure(cls, rng_max):
    """(e, H1, H2): the size the oracle's rounding error may have.  d = p - T.t is rounded relative to d itself (half an ulp), so every
    quantity is conditioned by the slant range r = |d| and not by the kilometre the coordinates have: pm = R^T d is three products and two
    sums of terms <= r (3 eps r), its norm carries that plus a square root, so e = (nrm - mx, pm_x - my) is off by a few eps r however much
    cancels; H1's first row is pm / nrm . R^T, entries <= 1 (a few eps), its second row is copied; H2 is [pm]x and -R^T, copied, and its
    first row the same quotient applied to entries <= max(1, r).  `few` = 4 eps as in pose_algebra_ref.floor_figure.
    sss_zero: nrm = 0, the rows that divide by it are not numbers and are compared as a pattern; what is finite is copied or -mx, -my: exact."""
    few = 4 * EPS
    if cls == "sss_zero":
        return 0.0, 0.0, 0.0
    return few * rng_max, few, few * max(1.0, rng_max)


def rpy_floor_figure():
    """three atan2 of entries the reference reads as the same doubles: a correctly rounded result is within half an ulp of pi; the pitch goes
    through sqrt(R21^2 + R22^2), 1.5 eps relative in one argument, which moves an atan2 by at most half of that.  4 eps pi, `few` ulps of the
    largest result, as the near-pi classes of pose_algebra_ref.floor_figure."""
    return 4 * EPS * math.pi


def retract_floor_figure(cls, thetas):
    """(R entries, t) of T Exp(xi): R = R_T R_E is three products of an entry <= 1 with an entry that carries the exponential's floor figure fw,
    plus the products' own rounding; t = R_T t_E + t_T carries the exponential's translation figure fv through three such products, and rounding
    relative to |t_E| + |t_T| <= 2 T_NORM"""
    fw, fv = P.floor_figure(cls, thetas)
    return 3 * fw + 4 * EPS, math.sqrt(3.0) * fv + 4 * EPS * 2 * P.T_NORM


# ------------------------------------------------------------------ dsss_sincos
INVPIO2 = 6.36619772367581382433e-01
PIO2_1 = 1.57079632673412561417e+00
PIO2_1T = 6.07710050650619224932e-11
SINCOS_NEAR = 4 * math.pi + math.pi / 2              # up to here the project's own bar of 4.5e-16 holds (test_sincos_polynomial_vs_numpy)


def _neigh(x, n=4):
    out = [x]
    lo = hi = x
    for _ in range(n):
        lo = np.nextafter(lo, -np.inf); hi = np.nextafter(hi, np.inf)
        out += [lo, hi]
    return out


def sincos_args():
    """every 0.01 degree of a heading in [-2 pi, 2 pi] and those +- pi / 2 (what dsss_geo_side adds); the double neighbours of k pi / 2,
    |k| <= 8; the arguments where x * invpio2 crosses k + 1/2 (rint changes the quadrant); +-0; |x| up to 1e6 in decades"""
    k = np.arange(-36000, 36001, dtype=np.float64)
    h = k * (math.pi / 18000.0)
    parts = [h, h + math.pi / 2, h - math.pi / 2]
    near = []
    for q in range(-8, 9):
        near += _neigh(np.float64(q * (math.pi / 2)))
        near += _neigh(np.float64((q + 0.5) / INVPIO2))
    parts.append(np.array(near + [0.0, -0.0]))
    rng = np.random.default_rng(SEED + 1)
    far = []
    for d in range(1, 7):
        far += [10.0 ** d, -(10.0 ** d)]
        far += list(rng.uniform(10.0 ** (d - 1), 10.0 ** d, 50) * rng.choice([-1.0, 1.0], 50))
    parts.append(np.array(far))
    return np.concatenate(parts)


def oracle_sincos(orc, x):
    L = orc.lib()
    s, c = C.c_double(), C.c_double()
    out = np.empty((len(x), 2))
    for i, v in enumerate(x):
        L.orc_sincos(float(v), C.byref(s), C.byref(c)); out[i, 0] = s.value; out[i, 1] = c.value
    return out


# ------------------------------------------------------------------ fast_atan2_dev
IC_MAX = 15 * 255 * 709                              # the largest first moment of a radius-15 patch of 8-bit pixels (an exact float)


def atan2_pairs():
    """(y, x) float32: all 511 x 511 integer gradients in [-255, 255] (the SIFT domain, zeros included) and 20 000 pairs of IC-moment size,
    both signs, the axes and the diagonals among them"""
    g = np.arange(-255, 256, dtype=np.float32)
    yy, xx = np.meshgrid(g, g, indexing="ij")
    rng = np.random.default_rng(SEED + 2)
    m = rng.integers(-IC_MAX, IC_MAX + 1, (20000, 2)).astype(np.float32)
    m[:200, 0] = 0; m[200:400, 1] = 0; m[400:500, 1] = m[400:500, 0]; m[500:600, 1] = -m[500:600, 0]
    m[600] = (IC_MAX, IC_MAX); m[601] = (-IC_MAX, IC_MAX); m[602] = (IC_MAX, -IC_MAX); m[603] = (-IC_MAX, -IC_MAX); m[604] = (0, 0)
    return np.concatenate([np.stack([yy.ravel(), xx.ravel()], axis=1), m]).astype(np.float32)


def oracle_atan2(orc, yx):
    f = orc.lib().orc_fast_atan2
    return np.array([f(float(y), float(x)) for y, x in yx], np.float32)


# ------------------------------------------------------------------ dsss_geo_at
def geo_cases():
    """-> rows [pose row(6), M, col, gr(16, the first M / 2 used)]: M in {4, 6, 32}, the columns around the nadir and at both ends (port
    column 0 clamps), yaw at 0, +-pi/2, +-pi and random"""
    rng = np.random.default_rng(SEED + 3)
    yaws = [0.0, math.pi / 2, -math.pi / 2, math.pi, -math.pi] + list(rng.uniform(-math.pi, math.pi, 6))
    rows = []
    for M in (4, 6, 32):
        half = M // 2
        gr = np.zeros(16); gr[:half] = np.sort(rng.uniform(0.5, 150.0, half))
        for col in sorted({0, 1, half - 1, half, half + 1, M - 1}):
            for yaw in yaws:
                pose = [rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), yaw, rng.uniform(-1000, 1000), rng.uniform(-1000, 1000), rng.uniform(-50, 0)]
                rows.append(np.concatenate([pose, [M, col], gr]))
    return np.array(rows, np.float64)


def oracle_geo(orc, rows):
    L = orc.lib()
    x, y = C.c_double(), C.c_double()
    out = np.empty((len(rows), 2))
    for i, r in enumerate(rows):
        pose, gr = np.ascontiguousarray(r[:6]), np.ascontiguousarray(r[8:24])
        L.orc_geo_at(orc.dp(pose), orc.dp(gr), 1, int(r[6]), 0, int(r[7]), C.byref(x), C.byref(y)); out[i] = x.value, y.value
    return out


# ------------------------------------------------------------------ factor_eval<true>, Between form
def factor_cases(fx):
    """the composed cases (kilometre coordinates) with weights over twelve decades -> rows [Xa Xb meas w(6)]"""
    cin = fx["cmp_in"]
    w = 10.0 ** np.random.default_rng(SEED + 4).uniform(-6, 6, (len(cin), 6))
    w[0] = 1.0
    return np.concatenate([cin, w], axis=1)


def oracle_factor_jacobian(orc, rows):
    """Ji = -Ad(h^-1) w, h = Xa^-1 Xb, from the oracle's between, inverse and adjoint with one multiply per entry"""
    L = orc.lib()
    out = np.empty((len(rows), 36)); ad = np.zeros(36)
    h, hi = orc.Pose(), orc.Pose()
    for i, r in enumerate(rows):
        A, B = P._opose(orc, r[:12]), P._opose(orc, r[12:24])
        L.orc_pose_between(C.byref(A), C.byref(B), C.byref(h)); L.orc_pose_inverse(C.byref(h), C.byref(hi)); L.orc_pose_adjoint(C.byref(hi), orc.dp(ad))
        out[i] = ((-ad).reshape(6, 6) * r[36:42][:, None]).ravel()
    return out


# ------------------------------------------------------------------ chol6_recip, chol6_rdiag
def chol_cases():
    """-> (A n x 36 row-major symmetric, kind): kind 0 S (B^T B + I) S with column scales S = 10^U(-6, 6) (positive definite whatever S, the
    2-norm condition number is not), 1 the identity, 2 a third pivot of exactly 0, 3 a negative one, 4 a NaN entry, 5 +inf on the diagonal"""
    rng = np.random.default_rng(SEED + 5)
    A, kind = [], []
    for _ in range(200):
        B = rng.normal(size=(8, 6))
        s = 10.0 ** rng.uniform(-6, 6, 6)
        M = (B.T @ B + np.eye(6)) * s[:, None] * s[None, :]
        M = np.tril(M) + np.tril(M, -1).T
        A.append(M); kind.append(0)
    A.append(np.eye(6)); kind.append(1)
    Lz = np.array([[2, 0, 0, 0, 0, 0], [1, 3, 0, 0, 0, 0], [-1, 2, 0, 0, 0, 0], [3, 1, 1, 2, 0, 0], [1, -2, 2, 1, 3, 0], [2, 1, -1, 1, 1, 2]], np.float64)
    Z = Lz @ Lz.T                                     # small integers: every product and sum is exact, the third pivot is 5 - 1 - 4 = 0
    A.append(Z); kind.append(2)
    N = Z.copy(); N[2, 2] -= 1.0
    A.append(N); kind.append(3)
    G = A[0].copy(); G[3, 1] = G[1, 3] = np.nan
    A.append(G); kind.append(4)
    I = np.eye(6) * 4.0; I[4, 4] = np.inf
    A.append(I); kind.append(5)
    return np.array(A).reshape(-1, 36), np.array(kind)


def chol6_recip_np(A36):
    """csrc/dsss_pg_dev.h's chol6_recip, its loop restated literally in f64 over a batch -> (A' n x 36, ri n x 6, bad n)"""
    A = A36.reshape(-1, 6, 6).copy()
    n = len(A)
    ri = np.zeros((n, 6)); bad = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for j in range(6):
            d = A[:, j, j].copy()
            for k in range(j): d = d - A[:, j, k] * A[:, j, k]
            b = ~(d > 0) | ~np.isfinite(d)
            bad |= b; d[b] = 1.0
            sq = np.sqrt(d); r = 1.0 / sq
            A[:, j, j] = sq; ri[:, j] = r
            for i in range(j + 1, 6):
                s = A[:, i, j].copy()
                for k in range(j): s = s - A[:, i, k] * A[:, j, k]
                A[:, i, j] = s * r
    return A.reshape(n, 36), ri, bad.astype(np.float64)


def rdiag_pivots(A36, L36):
    """the pivots d[j] chol6_rdiag took its rsqrt of, recomputed in f64 in its order from the L it stored: bit for bit the device's, because
    every operand is one the device wrote or read -> n x 6"""
    A, L = A36.reshape(-1, 6, 6), L36.reshape(-1, 6, 6)
    d = np.empty((len(A), 6))
    for j in range(6):
        v = A[:, j, j].copy()
        for k in range(j): v = v - L[:, j, k] * L[:, j, k]
        d[:, j] = v
    return d


def rdiag_backward_error(A36, L36):
    """max over the lower triangle of |A - L L^T| / (gamma_11 |L| |L|^T) in long double, with L[j][j] = 1 / r[j] for the stored reciprocal
    r[j]; gamma_k = k u / (1 - k u), u = 2^-53.  Higham's componentwise bound for a Cholesky factor of order 6 is gamma_7; the product s * r
    instead of a division adds two roundings and an rsqrt within 2 ulp another two: gamma_11 -> n ratios (<= 1 passes)"""
    ld = np.longdouble
    A, L = A36.reshape(-1, 6, 6).astype(ld), np.tril(L36.reshape(-1, 6, 6)).astype(ld)
    for j in range(6): L[:, j, j] = ld(1) / L[:, j, j]
    u = ld(2.0) ** -53
    g = 11 * u / (1 - 11 * u)
    res = np.abs(A - L @ L.transpose(0, 2, 1))
    bound = g * (np.abs(L) @ np.abs(L).transpose(0, 2, 1))
    il = np.tril_indices(6)
    res, bound = res[:, il[0], il[1]], bound[:, il[0], il[1]]
    with np.errstate(divide="ignore", invalid="ignore"):                            # (0 <= 0 holds: an entry whose row of L is zero but for it)
        ratio = np.where(bound > 0, res / bound, np.where(res == 0, 0.0, np.inf))
    return ratio.max(axis=1).astype(np.float64)


# ------------------------------------------------------------------ the scans
SCAN_N = [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097]
SCAN_TYPES = [np.int32, np.uint64, np.float64]


def scan_vectors():
    """per n: int32 counts with zeros, uint64 values whose running sum passes 2^63 (and wraps, as the device's does), f64 of mixed
    magnitude and sign -> list of (type code, array)"""
    rng = np.random.default_rng(SEED + 6)
    out = []
    for n in SCAN_N:
        i32 = rng.integers(0, 5, n).astype(np.int32); i32[rng.random(n) < 0.5] = 0
        u64 = rng.integers(1 << 59, 1 << 62, n, dtype=np.uint64)
        f64 = rng.normal(size=n) * 10.0 ** rng.uniform(-8, 8, n)
        out += [(0, i32), (1, u64), (2, f64)]
    return out


def scan_file(vecs):
    parts = []
    for code, v in vecs:
        parts.append(np.array([code, len(v)], np.int64))
        parts.append(v.astype(np.int64) if code == 0 else v.view(np.int64))
    return np.concatenate(parts)


def scan_parse(vecs, words):
    """the probe's output -> per vector a dict prefix (n), total, incl (P), wsum (P / 64), bsum (P / 256, f64 only), in the vector's type"""
    res, at = [], 0
    for code, v in vecs:
        n = len(v); Pn = (n + 255) // 256 * 256
        def take(m):
            nonlocal at
            w = words[at:at + m]; at += m
            return w.astype(np.int32) if code == 0 else w.view(SCAN_TYPES[code])
        d = dict(prefix=take(n), total=take(1)[0], incl=take(Pn), wsum=take(Pn // 64))
        if code == 2: d["bsum"] = take(Pn // 256)
        res.append(d)
    assert at == len(words), (at, len(words))
    return res


def pad256(v):
    out = np.zeros((len(v) + 255) // 256 * 256, v.dtype); out[:len(v)] = v
    return out


def wave_sum_np(v):
    """dsss_wave_sum on every wavefront of the padded vector: the xor butterfly from 32 down to 1, v += partner -> lane 0's value per wavefront"""
    x = pad256(v).reshape(-1, 64).copy()
    lane = np.arange(64)
    with np.errstate(over="ignore"):
        for o in (32, 16, 8, 4, 2, 1): x = x + x[:, lane ^ o]
    return x[:, 0]


def wave_scan_np(v):
    """dsss_wave_scan_incl: offsets 1, 2, ... 32, lanes >= o add the value o lanes below"""
    x = pad256(v).reshape(-1, 64).copy()
    with np.errstate(over="ignore"):
        for o in (1, 2, 4, 8, 16, 32):
            t = x.copy(); x[:, o:] = t[:, o:] + t[:, :-o]
    return x.ravel()


def block_sum_np(v):
    w = wave_sum_np(v).reshape(-1, 4)
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def carried_scan_np(v):
    """dsss_block_scan_excl<4> carried over chunks of 256 in the vector's own arithmetic (for f64: the device's order of additions)
    -> (exclusive prefixes, total)"""
    x = pad256(v)
    inc = wave_scan_np(v).reshape(-1, 4, 64)
    zero = x.dtype.type(0)
    base = zero
    out = np.empty(len(x), x.dtype)
    with np.errstate(over="ignore"):
        for c in range(len(inc)):
            sw = inc[c, :, 63]
            tot = zero; pre = []
            for k in range(4):
                pre.append(sum_in_order(sw[:k], zero)); tot = tot + sw[k]
            for k in range(4):
                sl = slice(c * 256 + k * 64, c * 256 + k * 64 + 64)
                out[sl] = base + ((pre[k] + inc[c, k]) - x[sl])
            base = base + tot
    return out[:len(v)], base


def sum_in_order(a, zero):
    s = zero
    for t in a: s = s + t
    return s


# ------------------------------------------------------------------ records
def rec(fid, *parts):
    r = np.zeros(IN_W); r[0] = fid
    v = np.concatenate([np.asarray(p, np.float64).ravel() for p in parts]); r[1:1 + len(v)] = v
    return r


def packed(fid, values, per_rec, width):
    """the long lists share records: [count, values ...] with per_rec items of `width` doubles each"""
    values = np.asarray(values, np.float64).reshape(-1, width)
    return [rec(fid, [len(values[i:i + per_rec])], values[i:i + per_rec]) for i in range(0, len(values), per_rec)]


def unpacked(out_rows, n, per_rec, width):
    """the outputs of packed records -> n x width"""
    return np.concatenate([out_rows[i, :min(per_rec, n - i * per_rec) * width] for i in range(len(out_rows))]).reshape(n, width)


LM_KINDS = 3
LM_ROWS_ASKED = 32                                    # more than any kind has: the probe says which exist


# ------------------------------------------------------------------ the fixture
def load():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def oracle_rpy(orc, T12):
    out = np.zeros((len(T12), 3)); o = np.zeros(3)
    for i, row in enumerate(T12):
        T = P._opose(orc, row); orc.lib().orc_pose_rpy(C.byref(T), orc.dp(o)); out[i] = o
    return out


def oracle_retract(orc, T12, xi6):
    out = np.zeros((len(T12), 12)); O = orc.Pose()
    for i, (row, x) in enumerate(zip(T12, xi6)):
        orc.lib().orc_pose_retract(C.byref(P._opose(orc, row)), orc.dp(np.ascontiguousarray(x)), C.byref(O)); out[i] = P._row12(O)
    return out


def oracle_sss(orc, in17):
    L = orc.lib()
    out = np.zeros((len(in17), 20)); e, H1, H2 = np.zeros(2), np.zeros(6), np.zeros(12)
    Ts = P._opose(orc, [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])
    for i, r in enumerate(in17):
        L.orc_sss_factor(orc.dp(np.ascontiguousarray(r[:3])), C.byref(P._opose(orc, r[3:15])), C.byref(Ts), C.c_double(r[15]), C.c_double(r[16]),
                         orc.dp(e), orc.dp(H1), orc.dp(H2))
        out[i] = np.concatenate([e, H1, H2])
    return out


SSS_PARTS = [slice(0, 2), slice(2, 8), slice(8, 20)]   # e, H1, H2


def oracle_floors(orc, d, fx):
    """per class the largest |oracle - reference| (finite references only: sss_zero's divided rows are compared as a pattern)"""
    er = P.diff_to_ref(oracle_rpy(orc, np.concatenate([fx["log_T"], d["gimbal_T"]])), d["rpy_ref_hi"], d["rpy_ref_lo"])
    rcls = np.concatenate([fx["log_class"].astype(int), np.full(len(d["gimbal_T"]), RPY_GIMBAL)])
    ti, xi = retract_index(fx)
    et = P.diff_to_ref(oracle_retract(orc, fx["log_T"][ti], fx["exp_xi"][xi]), d["retract_ref_hi"], d["retract_ref_lo"])
    tcls = fx["exp_class"][xi].astype(int) - P.CLASS_ID[RETRACT_CLASS_NAMES[0]]
    es = P.diff_to_ref(oracle_sss(orc, d["sss_in"]), d["sss_ref_hi"], d["sss_ref_lo"])
    es = np.where(np.isnan(d["sss_ref_hi"]), 0.0, es)
    fs = np.array([[es[d["sss_class"] == c][:, p].max() for p in SSS_PARTS] for c in range(len(SSS_CLASS_NAMES))])
    return dict(floor_rpy=P.class_max(er, rcls, len(RPY_CLASS_NAMES)),
                floor_retract_w=P.class_max(et[:, :9], tcls, len(RETRACT_CLASS_NAMES)),
                floor_retract_v=P.class_max(et[:, 9:], tcls, len(RETRACT_CLASS_NAMES)), floor_sss=fs)


# ================================================================== 50 digits from here on
def ref_atan2(y, x):
    """atan2 of two numbers that are doubles or 50-digit values, with IEEE 754's rules where both the sign of a zero and the result are
    decided by it (mpmath has no signed zero): the reference's atan2 of the same signed zeros"""
    mp = P._mp()
    if y == 0:
        r = mp.pi if (x < 0 or (x == 0 and math.copysign(1.0, float(x)) < 0)) else mp.mpf(0)
        return -r if math.copysign(1.0, float(y)) < 0 else r
    if x == 0:
        return mp.pi / 2 if y > 0 else -mp.pi / 2
    return mp.atan2(P._f(y), P._f(x))


def formula_pose_rpy(T):
    """Rot3::rpy(): roll = atan2(R32, R33), pitch = atan2(-R31, sqrt(R32^2 + R33^2)), yaw = atan2(R21, R11), on the doubles of R.
    -R31 of a zero flips its sign, the square root of a sum of squares is +0 when it is zero."""
    mp = P._mp()
    R = [float(x) for x in T[:9]]
    h = mp.sqrt(P._f(R[7]) * P._f(R[7]) + P._f(R[8]) * P._f(R[8]))
    return [ref_atan2(R[7], R[8]), ref_atan2(-R[6], h if h != 0 else 0.0), ref_atan2(R[3], R[0])]


def formula_pose_retract(T, xi):
    """Pose3::retract = T * Expmap(xi), nothing rounded in between"""
    E = P.formula_pose_exp(xi)
    R = [P._f(x) for x in T[:9]]
    t = P._mv(R, E[9:])
    return P._mul3(R, E[:9]) + [t[i] + P._f(T[9 + i]) for i in range(3)]


def formula_sss_factor(p, T, mx, my):
    """SssPointFactor::evaluateError of the reference project (src/core/SSSpointfactor.cpp:11-80, plan_a) with Ts the identity, restated:
    p_s = Ts^-1 (T^-1 p) = R^T (p - t); J = Rs^T R^T = R^T; H1 = [p_s^T J / |p_s|; e_1^T J]; block_t = -(Rs^T R^T) as written there,
    block_r = Rs^T [p_m]x with p_m = T^-1 p; H2 = [p_s^T [block_r block_t] / |p_s|; e_1^T [block_r block_t]]; error (|p_s| - mx, p_s.x - my).
    A division by |p_s| = 0 is NaN -> 20 numbers e(2) H1(6) H2(12)"""
    mp = P._mp()
    R = [P._f(x) for x in T[:9]]
    d = [P._f(p[i]) - P._f(T[9 + i]) for i in range(3)]
    J = P._tr3(R)
    ps = P._mv(J, d)
    n = P._norm(ps)
    div = (lambda v: v / n) if n != 0 else (lambda v: mp.nan)
    H1 = [div(ps[0] * J[j] + ps[1] * J[3 + j] + ps[2] * J[6 + j]) for j in range(3)] + J[:3]
    br = P._skew(ps)
    Jp = [[br[3 * i + j] for j in range(3)] + [-J[3 * i + j] for j in range(3)] for i in range(3)]
    H2 = [div(ps[0] * Jp[0][j] + ps[1] * Jp[1][j] + ps[2] * Jp[2][j]) for j in range(6)] + Jp[0]
    return [n - P._f(mx), ps[0] - P._f(my)] + H1 + H2


def _split_nan(v):
    mp = P._mp()
    hi = [float("nan") if mp.isnan(x) else float(x) for x in v]
    lo = [0.0 if math.isnan(h) else float(P._f(x) - P._f(h)) for x, h in zip(v, hi)]
    return hi, lo


def generate(orc):
    fx = P.load()
    gT = gimbal_cases()
    rpy = [P._split(formula_pose_rpy(T)) for T in np.concatenate([fx["log_T"], gT])]
    ti, xi = retract_index(fx)
    ret = [P._split(formula_pose_retract(T, x)) for T, x in zip(fx["log_T"][ti], fx["exp_xi"][xi])]
    sin, scls, srange = sss_cases()
    sss = [_split_nan(formula_sss_factor(r[:3], r[3:15], r[15], r[16])) for r in sin]
    d = dict(gimbal_T=gT, rpy_ref_hi=np.array([h for h, _ in rpy]), rpy_ref_lo=np.array([l for _, l in rpy]),
             retract_ref_hi=np.array([h for h, _ in ret]), retract_ref_lo=np.array([l for _, l in ret]),
             sss_in=sin, sss_class=scls, sss_range=srange, sss_ref_hi=np.array([h for h, _ in sss]), sss_ref_lo=np.array([l for _, l in sss]))
    d.update(oracle_floors(orc, d, fx))
    return d


if __name__ == "__main__":
    from oracle import binding
    data = P.to_bytes(generate(binding))
    with open(FIXTURE, "wb") as fh:
        fh.write(data)
    print("%s: %d bytes" % (FIXTURE, len(data)))

"""An independent reference for the SO(3)/SE(3) algebra of diasss_amd/csrc/dsss_pose.h and oracle/orc_pose.c, and the cases that reach
every branch of it.  Shared by tests/test_pose_algebra_cpu.py and tests/test_gpu_pose_algebra.py.

formula_*   GTSAM 4.2's Rot3 / Pose3 text (SO3::ExpmapFunctor, SO3::Logmap, Pose3::Expmap, Pose3::Logmap, AdjointMap)
            restated in mpmath: every branch PREDICATE is decided in IEEE double on the double inputs, in the code's operation order, every
            branch BODY is evaluated in DPS digits on those same doubles -- what the code would return if no operation rounded.  The double
            constant M_PI stays the double it is.
true_*      the exponential and the logarithm themselves in DPS digits (closed forms without thresholds); used for the gap table only:
            GTSAM's near-pi branch is first order in pi - theta and its |omega| < 1e-10 and theta^2 <= eps exits drop the coupling term.

The upper half needs numpy alone (classes, double predicates, bounds, the fixture's reader); mpmath is imported where a 50-digit number
is made, that is by the fixture writer (python -m tests.pose_algebra_ref) and by the one test that regenerates the fixture."""
import io
import math
import os
import zipfile

import numpy as np

EPS = 2.220446049250313e-16
DPS = 60
SEED = 20261020
N_RANDOM_AXES = 10         # random axes per angle (plus the three coordinate axes): the most that keeps the fixture under 200 KB
T_SCALE = 100.0            # |t_i| <= 100 m
T_NORM = T_SCALE * math.sqrt(3.0)
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_algebra.npz")
PI = math.pi

LOG_CLASSES = [
    ("log_small", [0.0, 1e-12, 5e-11, 9.9e-11]),
    ("log_taylor_lo", [1.01e-10, 1e-9, 1e-8, 1e-6]),
    ("log_taylor_hi", [1e-5, 1e-4, 9.99e-4]),
    ("log_seam_taylor_acos", None),
    ("log_acos_lo", [1.001e-3, 2e-3, 1e-2]),
    ("log_acos_mid", [0.1, 1.0, 2.0, 3.0]),
    ("log_acos_hi", [3.1, PI - 0.032]),
    ("log_seam_acos_pi", None),
    ("log_pi_outer", [PI - 0.0316, PI - 0.02, PI - 0.01]),
    ("log_pi_inner", [PI - 1e-3, PI - 1e-5, PI - 1e-8]),
    ("log_pi_exact", None),
    ("log_trace_out", None),
]
EXP_CLASSES = [
    ("exp_first_order", [0.0, 1e-12, 1.4e-8]),
    ("exp_cancel", [1.5e-8, 2e-8, 1e-7, 1e-6]),
    ("exp_mid", [1e-4, 1e-2, 1.0, 3.0]),
]
CLASS_NAMES = [c for c, _ in LOG_CLASSES] + [c for c, _ in EXP_CLASSES] + ["composed"]
CLASS_ID = {c: i for i, c in enumerate(CLASS_NAMES)}
# the classes whose cases also go through the exponential probe of the device test, and (less the angles within 1 % of a threshold) into the composed cases
INTERIOR = ["log_taylor_lo", "log_taylor_hi", "log_acos_lo", "log_acos_mid", "log_pi_inner"]
NEAR_THRESHOLD = [1.01e-10, 9.99e-4, 1.001e-3]
N_COMPOSED_AXES = 4
# branch of so3_log: 0 Taylor, 1 acos, 2 + p near pi with permutation p (0: R33 largest, 1: R22, 2: R11)
BR_TAYLOR, BR_ACOS, BR_PI = 0, 1, 2
# function ids of diasss_amd/host/pose_check.cpp
F_SO3_EXP, F_SO3_LOG, F_POSE_EXP, F_POSE_LOG, F_BETWEEN, F_INVERSE, F_COMPOSE, F_ADJOINT, F_RETRACT, F_RPY, F_RODRIGUES, F_EDGE = range(12)


# ------------------------------------------------------------------ IEEE double predicates, in the code's operation order
def log_branch(R):
    """the branch so3_log takes on the doubles R[9] -> (branch code, sign of Wv as the code decides it: -1 or +1; 0 outside the near-pi branch)"""
    R = [float(x) for x in R]
    R11, R12, R13, R21, R22, R23, R31, R32, R33 = R
    tr = (R11 + R22) + R33
    if tr + 1.0 < 1e-3:
        if R33 > R22 and R33 > R11: p, Wv = 0, R21 - R12
        elif R22 > R11: p, Wv = 1, R13 - R31
        else: p, Wv = 2, R32 - R23
        return BR_PI + p, (-1 if Wv < 0 else 1)
    if tr - 3.0 < -1e-6:
        return BR_ACOS, 0
    return BR_TAYLOR, 0


def exp_first_order(w):
    w = [float(x) for x in w]
    return (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2] <= 2.220446049250313e-16


def log_small(w):
    """pose_log's exit: t < 1e-10 with t the double norm of the double omega"""
    w = [float(x) for x in w]
    return math.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]) < 1e-10


def ulp(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)))


# ------------------------------------------------------------------ derived figures (the tests assert floors against 16 x these)
def _acos_w(th):
    """rounding of the trace (an ulp of 3, halved: 1.5 eps in cos theta) through acos, theta / (2 sin theta) and the product with 2 sin theta k:
    d omega = d theta (1 - theta cot theta), d theta = d cos / sin theta; plus a few ulps of the result.  Never above the eps / sin^2 theta
    the branch is known for: (1 - theta cot theta) sin theta <= pi on (0, pi)."""
    return 1.5 * EPS * abs(1.0 - th / math.tan(th)) / math.sin(th) + 4 * EPS * th


def floor_figure(cls, thetas):
    """(rotation part, translation part): the size the oracle's rounding error may have in class `cls`, from the conditioning of the branch
    body at the class's angles and |t| <= T_NORM.  Exp classes: (R entries, t)."""
    th = [float(t) for t in thetas]
    few = 4 * EPS
    if cls in ("log_small",):
        return few * max(max(th), 1e-300), 0.0                               # omega: a few ulps of the result; v = t, copied
    if cls in ("log_taylor_lo", "log_taylor_hi"):
        return few * max(th), few * T_NORM                                  # a few ulps of the result, eps |t|
    if cls == "log_seam_taylor_acos":
        return max(few * 1e-3, _acos_w(1e-3)), (few + _acos_w(1e-3)) * T_NORM
    if cls in ("log_acos_lo", "log_acos_mid", "log_acos_hi", "log_seam_acos_pi"):
        w = max(_acos_w(t) for t in th)
        return w, (few + w) * T_NORM
    if cls in ("log_pi_outer", "log_pi_inner", "log_pi_exact"):
        return few * PI, 2 * few * T_NORM                                    # a few ulps of pi; v is up to ~3 |t|
    if cls == "log_trace_out":
        return few * PI, 2 * few * T_NORM
    if cls == "exp_first_order":
        return few, 0.0                                                      # R = I + W: exact but for nothing; t = v, copied
    if cls in ("exp_cancel", "exp_mid"):
        return few, EPS * T_NORM * (1.0 / min(th) + 4.0)                     # (w x v - R (w x v) + w (w.v)) / theta^2: three terms of size theta |v|
    if cls == "composed":
        # two 3-term products per entry of the error rotation (4 eps each, 6 eps in cos theta) through the acos branch at theta = 3, the
        # worst interior angle; translations of 2 km through two products
        w = 4 * 1.5 * EPS * abs(1.0 - 3.0 / math.tan(3.0)) / math.sin(3.0) + 8 * EPS * PI
        return w, w * T_NORM + 8 * EPS * 2000.0 * math.sqrt(3.0)
    raise KeyError(cls)


def gap_bound(cls, theta, tnorm):
    """(rotation, translation): how far GTSAM's formula may be from the true map at one case, on top of the class's floor figure"""
    if cls.startswith("log_pi") or cls == "log_seam_acos_pi":
        d = PI - theta
        return d * d, d * d * max(1.0, tnorm)                                # the near-pi branch is first order in pi - theta
    if cls == "log_small":
        return 0.0, 0.5 * theta * tnorm                                      # v = t: the term -0.5 omega x t is dropped
    if cls == "exp_first_order":
        return theta * theta, 0.5 * theta * tnorm + theta * theta * tnorm    # R = I + W, t = v: the second-order terms are dropped
    return 0.0, 0.0


# ------------------------------------------------------------------ the fixture's reader
def load():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def hilo(d, name):
    """the 50-digit reference as a pair of doubles: hi + lo"""
    return d[name + "_hi"], d[name + "_lo"]


def diff_to_ref(q, hi, lo):
    """|q - (hi + lo)| without losing lo: q - hi is exact when q is within a factor 2 of hi, and close otherwise"""
    return np.abs((np.asarray(q, np.float64) - hi) - lo)


def odo_weights():
    """the odometry weights of the pose graph (dsss_pg_report.hip, orc_posegraph.c), as doubles"""
    P, wgt1, wgt2 = 3.14159265359, 0.001, 10
    so = [wgt1 * P / 180, wgt1 * P / 180, 0.1 * wgt1 * wgt2 * P / 180, wgt1 * wgt2, wgt1 * wgt2, wgt1]
    return [1.0 / s for s in so]


# ================================================================== 50 digits from here on
_MP = None


def _mp():
    global _MP
    if _MP is None:
        import mpmath
        _MP = mpmath.mp
        _MP.dps = DPS
    return _MP


def _f(x):
    return _mp().mpf(x)


def _mul3(A, B):
    return [A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j] for i in range(3) for j in range(3)]


def _mv(A, v):
    return [A[3 * i] * v[0] + A[3 * i + 1] * v[1] + A[3 * i + 2] * v[2] for i in range(3)]


def _tr3(A):
    return [A[3 * j + i] for i in range(3) for j in range(3)]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _skew(w):
    return [0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0]


def _norm(v):
    return _mp().sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def formula_so3_exp(w):
    """SO3::ExpmapFunctor: nearZero = theta^2 <= epsilon -> I + W; else I + sin(theta) K + 2 sin^2(theta / 2) K K, K = W / theta"""
    mp = _mp()
    wm = [_f(x) for x in w]
    W = _skew(wm)
    I = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    if exp_first_order(w):
        return [_f(I[i]) + W[i] for i in range(9)]
    th = _norm(wm)
    K = [x / th for x in W]
    KK = _mul3(K, K)
    s, s2 = mp.sin(th), mp.sin(th / 2)
    return [I[i] + s * K[i] + 2 * s2 * s2 * KK[i] for i in range(9)]


def formula_so3_log(R):
    """SO3::Logmap: tr + 1 < 1e-3 -> the first-order form around pi, by the largest diagonal entry; tr - 3 < -1e-6 -> theta / (2 sin theta);
    else 1/2 - (tr - 3) / 12 + (tr - 3)^2 / 60.  -> (omega, branch code)"""
    mp = _mp()
    R11, R12, R13, R21, R22, R23, R31, R32, R33 = [_f(x) for x in R]
    br, sgn = log_branch(R)
    tr = R11 + R22 + R33
    if br >= BR_PI:
        if br == BR_PI: Wv, Q1, Q2, Q3 = R21 - R12, 2 + 2 * R33, R31 + R13, R23 + R32
        elif br == BR_PI + 1: Wv, Q1, Q2, Q3 = R13 - R31, 2 + 2 * R22, R23 + R32, R12 + R21
        else: Wv, Q1, Q2, Q3 = R32 - R23, 2 + 2 * R11, R12 + R21, R31 + R13
        r = mp.sqrt(Q1)
        nrm = mp.sqrt(Q1 * Q1 + Q2 * Q2 + Q3 * Q3 + Wv * Wv)
        mag = _f(math.pi) - (2 * sgn * Wv) / nrm                             # M_PI, the double
        sc = sgn * (_f(0.5) * (1 / r) * mag)
        if br == BR_PI: return [sc * Q2, sc * Q3, sc * Q1], br
        if br == BR_PI + 1: return [sc * Q3, sc * Q1, sc * Q2], br
        return [sc * Q1, sc * Q2, sc * Q3], br
    if br == BR_ACOS:
        th = mp.acos((tr - 1) / 2)
        mag = th / (2 * mp.sin(th))
    else:
        t3 = tr - 3
        mag = _f(0.5) - t3 / 12 + t3 * t3 / 60
    return [mag * (R32 - R23), mag * (R13 - R31), mag * (R21 - R12)], br


def formula_pose_exp(xi):
    """Pose3::Expmap: theta^2 > epsilon -> t = (w x v - R (w x v) + w (w . v)) / theta^2, else t = v -> 12 numbers"""
    w = [_f(x) for x in xi[:3]]; v = [_f(x) for x in xi[3:6]]
    R = formula_so3_exp(xi[:3])
    if exp_first_order(xi[:3]):
        return R + v
    t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    wv = w[0] * v[0] + w[1] * v[1] + w[2] * v[2]
    c = _cross(w, v)
    Rc = _mv(R, c)
    return R + [(c[i] - Rc[i] + w[i] * wv) / t2 for i in range(3)]


def formula_pose_log(T):
    """Pose3::Logmap: omega = Rot3::Logmap(R), t = |omega|; t < 1e-10 -> [omega, T]; else with W = [omega / t]x:
    u = T - (t / 2) W T + (1 - t / (2 tan(t / 2))) W W T -> (xi, branch code of the rotation, whether the small exit was taken)"""
    mp = _mp()
    w, br = formula_so3_log(T[:9])
    t = [_f(x) for x in T[9:12]]
    if log_small(w):
        return w + t, br, True
    th = _norm(w)
    k = [x / th for x in w]
    WT = _cross(k, t)
    WWT = _cross(k, WT)
    c = 1 - th / (2 * mp.tan(th / 2))
    return w + [t[i] - (th / 2) * WT[i] + c * WWT[i] for i in range(3)], br, False


def formula_pose_inverse(A):
    Rt = _tr3([_f(x) for x in A[:9]])
    return Rt + [-x for x in _mv(Rt, [_f(x) for x in A[9:12]])]


def formula_pose_compose(A, B):
    RA = [_f(x) for x in A[:9]]
    t = _mv(RA, [_f(x) for x in B[9:12]])
    return _mul3(RA, [_f(x) for x in B[:9]]) + [t[i] + _f(A[9 + i]) for i in range(3)]


def formula_pose_between(A, B):
    return formula_pose_compose(formula_pose_inverse(A), B)


def formula_pose_adjoint(T):
    """Pose3::AdjointMap: [R 0; [t]x R, R], 36 numbers row-major"""
    R = [_f(x) for x in T[:9]]
    A = _mul3(_skew([_f(x) for x in T[9:12]]), R)
    Ad = [_f(0)] * 36
    for i in range(3):
        for j in range(3):
            Ad[6 * i + j] = R[3 * i + j]; Ad[6 * (i + 3) + j] = A[3 * i + j]; Ad[6 * (i + 3) + j + 3] = R[3 * i + j]
    return Ad


def formula_edge_error(Xa, Xb, rel):
    """the Between factor's error Log(rel^-1 Xa^-1 Xb), nothing rounded in between"""
    return formula_pose_log(formula_pose_between(rel, formula_pose_between(Xa, Xb)))


def formula_probe(p6):
    """the scalar the device's exponential leaves through: 0.5 sum_a (odo_a Log(Pose3(Rodrigues(p[:3]), p[3:])^-1)_a)^2"""
    T = formula_so3_exp(p6[:3]) + [_f(x) for x in p6[3:6]]
    xi = formula_pose_log(formula_pose_inverse(T))[0]
    od = odo_weights()
    return sum((_f(od[a]) * xi[a]) ** 2 for a in range(6)) / 2


# ------------------------------------------------------------------ the maps themselves
def true_so3_exp(w):
    mp = _mp()
    wm = [_f(x) for x in w]
    th = _norm(wm)
    I = [_f(1), _f(0), _f(0), _f(0), _f(1), _f(0), _f(0), _f(0), _f(1)]
    if th == 0:
        return I
    K = [x / th for x in _skew(wm)]
    KK = _mul3(K, K)
    s, c1 = mp.sin(th), 2 * mp.sin(th / 2) ** 2
    return [I[i] + s * K[i] + c1 * KK[i] for i in range(9)]


def true_so3_log(R):
    """theta = atan2(|s| / 2, (tr - 1) / 2) with s the vector of R - R^T; the axis from s below 2 pi / 3 and from the symmetric part
    (R + R^T) / 2 - cos(theta) I = (1 - cos theta) k k^T above, signed by s (at pi exactly, where both signs are logarithms: the sign that
    makes the component of the largest diagonal entry positive, GTSAM's choice)"""
    mp = _mp()
    Rm = [_f(x) for x in R]
    s = [Rm[7] - Rm[5], Rm[2] - Rm[6], Rm[3] - Rm[1]]
    sn, cs = _norm(s) / 2, (Rm[0] + Rm[4] + Rm[8] - 1) / 2
    th = mp.atan2(sn, cs)
    if th == 0:
        return [_f(0)] * 3
    if cs > -0.5:
        return [th * x / (2 * sn) for x in s]
    M = [(Rm[3 * i + j] + Rm[3 * j + i]) / 2 - (cs if i == j else 0) for i in range(3) for j in range(3)]
    j = max(range(3), key=lambda a: (M[4 * a], a))
    k = [M[3 * i + j] for i in range(3)]
    n = _norm(k)
    k = [x / n for x in k]
    if s[0] * k[0] + s[1] * k[1] + s[2] * k[2] < 0:
        k = [-x for x in k]
    return [th * x for x in k]


def true_pose_exp(xi):
    """t = V v, V = I + (1 - cos theta) / theta^2 W + (theta - sin theta) / theta^3 W^2"""
    mp = _mp()
    w = [_f(x) for x in xi[:3]]; v = [_f(x) for x in xi[3:6]]
    R = true_so3_exp(xi[:3])
    th = _norm(w)
    if th == 0:
        return R + v
    a, b = 2 * mp.sin(th / 2) ** 2 / th ** 2, (th - mp.sin(th)) / th ** 3
    wv = _cross(w, v); wwv = _cross(w, wv)
    return R + [v[i] + a * wv[i] + b * wwv[i] for i in range(3)]


def true_pose_log(T):
    """v = V^-1 t = t - omega x t / 2 + (1 - (theta / 2) cot(theta / 2)) / theta^2 omega x (omega x t)"""
    mp = _mp()
    w = true_so3_log(T[:9])
    t = [_f(x) for x in T[9:12]]
    th = _norm(w)
    if th == 0:
        return w + t
    c = (1 - (th / 2) * mp.cos(th / 2) / mp.sin(th / 2)) / th ** 2
    wt = _cross(w, t); wwt = _cross(w, wt)
    return w + [t[i] - wt[i] / 2 + c * wwt[i] for i in range(3)]


# ------------------------------------------------------------------ the cases
def _round(v):
    return [float(x) for x in v]


def _split(v):
    hi = [float(x) for x in v]
    lo = [float(_f(x) - _f(h)) for x, h in zip(v, hi)]
    return hi, lo


def _axes(rng, n):
    out = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)]
    for _ in range(n):
        out.append(tuple(rng.normal(size=3)))
    return out


def _rot(theta, axis):
    """round(Exp_50(theta k)), k = axis normalised in 50 digits"""
    a = [_f(x) for x in axis]
    n = _norm(a)
    return _round(true_so3_exp([_f(theta) * x / n for x in a]))


def _seam_pair(axis, lo, hi, side):
    """bisect theta in [lo, hi] down to two neighbouring doubles between which the branch of so3_log on round(Exp(theta k)) changes"""
    assert side(_rot(lo, axis)) != side(_rot(hi, axis))
    s_lo = side(_rot(lo, axis))
    while True:
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            return lo, hi
        if side(_rot(mid, axis)) == s_lo: lo = mid
        else: hi = mid


def _pi_exact_cases():
    """2 k k^T - I for k = e1, e2, e3, (0,1,1), (1,0,1), (1,1,0), (1,1,1) normalised: entries 0, 1, -1, 2/3, -1/3.  The matrix is the same for
    k and -k; the sign of the result is the sign of Wv, the off-diagonal pair of the permutation taken, moved apart by an ulp either way
    (2^-53 where the entries are zero) or left equal"""
    out = []
    for k in [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 1)]:
        n2 = sum(x * x for x in k)
        R0 = [2.0 * k[i] * k[j] / n2 - (1.0 if i == j else 0.0) for i in range(3) for j in range(3)]
        p = log_branch(R0)[0] - BR_PI
        plus, minus = [(3, 1), (2, 6), (7, 5)][p]                            # Wv = R[plus] - R[minus]
        for sg in (0, 1, -1):
            R = list(R0)
            if sg:
                for idx, d in ((plus, sg), (minus, -sg)):
                    R[idx] = float(np.nextafter(R[idx], d * np.inf)) if R[idx] != 0 else d * 2.0 ** -53
            out.append((R, sg))
    return out


def _trace_out_cases(rng, n):
    """products of rounded rotations, multiplied in double: a trace of 3 + ulp (R R^T of a small rotation) and a trace below -1 (two rotations
    about one axis whose angles add up to pi)"""
    hi, lo = [], []
    while len(hi) < n or len(lo) < n:
        ax = rng.normal(size=3)
        th = float(rng.uniform(0.05, 1.5))
        A = np.array(_rot(th, ax)).reshape(3, 3)
        P = A @ A.T
        if (P[0, 0] + P[1, 1]) + P[2, 2] == 3.0 + 2 * EPS and len(hi) < n:
            hi.append([float(x) for x in P.ravel()])
        B = np.array(_rot(PI - th, ax)).reshape(3, 3)
        Q = A @ B
        if ((Q[0, 0] + Q[1, 1]) + Q[2, 2]) + 1.0 < 0 and len(lo) < n:
            lo.append([float(x) for x in Q.ravel()])
    return hi + lo


def _rand_t(rng):
    return [float(x) for x in rng.uniform(-T_SCALE, T_SCALE, 3)]


def generate(orc):
    """every array of the fixture.  `orc` (oracle.binding) supplies the oracle's outputs, whose distance to the reference is the floor."""
    import ctypes as C
    mp = _mp()
    rng = np.random.default_rng(SEED)
    L = orc.lib()

    # ---- logarithm cases
    log_T, log_cls, log_th = [], [], []

    def add_log(cls, R, t, th):
        log_T.append(list(R) + list(t)); log_cls.append(CLASS_ID[cls]); log_th.append(float(th))

    is_acos = lambda R: log_branch(R)[0] == BR_ACOS
    is_pi = lambda R: log_branch(R)[0] >= BR_PI
    for cls, thetas in LOG_CLASSES:
        if thetas is not None:
            for i, th in enumerate(thetas):
                for ax in _axes(rng, N_RANDOM_AXES):
                    add_log(cls, _rot(th, ax), _rand_t(rng), th)
            add_log(cls, _rot(thetas[0], rng.normal(size=3)), [0.0, 0.0, 0.0], thetas[0])
        elif cls == "log_seam_taylor_acos":
            for i, ax in enumerate(_axes(rng, N_RANDOM_AXES + 1)):              # (the last pair is the class's t = 0 case)
                a, b = _seam_pair(ax, 9.99e-4, 1.001e-3, is_acos)
                t = _rand_t(rng) if i < N_RANDOM_AXES + 3 else [0.0, 0.0, 0.0]
                add_log(cls, _rot(a, ax), t, a); add_log(cls, _rot(b, ax), t, b)
        elif cls == "log_seam_acos_pi":
            for i, ax in enumerate(_axes(rng, N_RANDOM_AXES + 1)):
                a, b = _seam_pair(ax, PI - 0.032, PI - 0.0316, is_pi)
                t = _rand_t(rng) if i < N_RANDOM_AXES + 3 else [0.0, 0.0, 0.0]
                add_log(cls, _rot(a, ax), t, a); add_log(cls, _rot(b, ax), t, b)
        elif cls == "log_pi_exact":
            for R, sg in _pi_exact_cases():
                add_log(cls, R, _rand_t(rng), PI)
            add_log(cls, _pi_exact_cases()[9][0], [0.0, 0.0, 0.0], PI)
        elif cls == "log_trace_out":
            for k, R in enumerate(_trace_out_cases(rng, 6)):
                add_log(cls, R, _rand_t(rng), 0.0 if k < 6 else PI)
            add_log(cls, log_T[-1][:9], [0.0, 0.0, 0.0], PI)
    log_T = np.array(log_T, np.float64)
    n = len(log_T)
    log_ref = [formula_pose_log(T) for T in log_T]
    log_hi, log_lo = zip(*[_split(r[0]) for r in log_ref])
    log_true = [true_pose_log(T) for T in log_T]
    log_gap = [[float(max(abs(a - b) for a, b in zip(r[0][:3], u[:3]))), float(max(abs(a - b) for a, b in zip(r[0][3:], u[3:])))]
               for r, u in zip(log_ref, log_true)]

    # ---- exponential cases
    exp_xi, exp_cls, exp_th = [], [], []
    for cls, thetas in EXP_CLASSES:
        for th in thetas:
            for ax in _axes(rng, N_RANDOM_AXES):
                a = np.asarray(ax, np.float64)
                exp_xi.append([float(x) for x in th * (a / np.linalg.norm(a))] + _rand_t(rng)); exp_cls.append(CLASS_ID[cls]); exp_th.append(th)
        a = rng.normal(size=3)
        exp_xi.append([float(x) for x in thetas[0] * (a / np.linalg.norm(a))] + [0.0, 0.0, 0.0]); exp_cls.append(CLASS_ID[cls]); exp_th.append(thetas[0])
    exp_xi = np.array(exp_xi, np.float64)
    exp_ref = [formula_pose_exp(x) for x in exp_xi]
    exp_hi, exp_lo = zip(*[_split(r) for r in exp_ref])
    exp_true = [true_pose_exp(x) for x in exp_xi]
    exp_gap = [[float(max(abs(a - b) for a, b in zip(r[:9], u[:9]))), float(max(abs(a - b) for a, b in zip(r[9:], u[9:])))]
               for r, u in zip(exp_ref, exp_true)]

    # ---- composed cases: rel = round(between_50(Xa, Xb) Exp_50(xi)), the reference Log(rel^-1 Xa^-1 Xb) on the rounded inputs.
    # Axes are drawn until no component and no two squared components are closer than 0.05: the near-pi permutation and the sign of Wv
    # then sit far from their ties.
    cmp_in, cmp_th = [], []
    for cls in INTERIOR:
        for th in dict(LOG_CLASSES)[cls]:
            if th in NEAR_THRESHOLD:
                continue
            for _ in range(N_COMPOSED_AXES):
                while True:
                    k = rng.normal(size=3); k /= np.linalg.norm(k)
                    q = k * k
                    if np.abs(k).min() > 0.05 and min(abs(q[0] - q[1]), abs(q[1] - q[2]), abs(q[0] - q[2])) > 0.05:
                        break
                X = []
                for _x in range(2):
                    rv = [float(rng.uniform(-0.1, 0.1)), float(rng.uniform(-0.1, 0.1)), float(rng.uniform(-PI, PI))]
                    X.append(_round(true_so3_exp(rv)) + [float(x) for x in rng.uniform(-1000.0, 1000.0, 3)])
                xi = [float(x) for x in th * k] + _rand_t(rng)
                rel = _round(formula_pose_compose(formula_pose_between(X[0], X[1]), true_pose_exp(xi)))
                cmp_in.append(X[0] + X[1] + rel); cmp_th.append(th)
    cmp_in = np.array(cmp_in, np.float64)
    cmp_ref = [formula_edge_error(c[:12], c[12:24], c[24:36]) for c in cmp_in]
    cmp_hi, cmp_lo = zip(*[_split(r[0]) for r in cmp_ref])

    # ---- the exponential probe: the exp cases and the generating tangents of the interior log classes
    probe_xi, probe_cls = [list(x) for x in exp_xi], list(exp_cls)
    rng2 = np.random.default_rng(SEED + 1)
    for cls in INTERIOR:
        for th in dict(LOG_CLASSES)[cls]:
            for ax in _axes(rng2, N_RANDOM_AXES):
                a = np.asarray(ax, np.float64)
                probe_xi.append([float(x) for x in th * (a / np.linalg.norm(a))] + _rand_t(rng2)); probe_cls.append(CLASS_ID[cls])
    probe_xi = np.array(probe_xi, np.float64)
    probe_hi, probe_lo = _split([formula_probe(p) for p in probe_xi])

    d = dict(class_names=np.array(CLASS_NAMES),
             log_T=log_T, log_class=np.array(log_cls, np.int16), log_theta=np.array(log_th), log_branch=np.array([r[1] for r in log_ref], np.int16),
             log_ref_hi=np.array(log_hi), log_ref_lo=np.array(log_lo), log_gap=np.array(log_gap),
             exp_xi=exp_xi, exp_class=np.array(exp_cls, np.int16), exp_theta=np.array(exp_th),
             exp_ref_hi=np.array(exp_hi), exp_ref_lo=np.array(exp_lo), exp_gap=np.array(exp_gap),
             cmp_in=cmp_in, cmp_theta=np.array(cmp_th), cmp_branch=np.array([r[1] for r in cmp_ref], np.int16), cmp_ref_hi=np.array(cmp_hi), cmp_ref_lo=np.array(cmp_lo),
             probe_xi=probe_xi, probe_class=np.array(probe_cls, np.int16), probe_ref_hi=np.array(probe_hi), probe_ref_lo=np.array(probe_lo))
    d.update(oracle_floors(orc, d))
    return d


# ------------------------------------------------------------------ the oracle on the fixture's cases (numpy and ctypes alone)
def _opose(orc, row12):
    T = orc.Pose()
    for k in range(9): T.R[k] = row12[k]
    for k in range(3): T.t[k] = row12[9 + k]
    return T


def _row12(T):
    return list(T.R) + list(T.t)


def oracle_log(orc, T12):
    import ctypes as C
    out = np.zeros((len(T12), 6)); o = np.zeros(6)
    for i, row in enumerate(T12):
        T = _opose(orc, row); orc.lib().orc_pose_log(C.byref(T), orc.dp(o)); out[i] = o
    return out


def oracle_exp(orc, xi6):
    import ctypes as C
    out = np.zeros((len(xi6), 12))
    for i, x in enumerate(xi6):
        T = orc.Pose(); orc.lib().orc_pose_exp(orc.dp(np.ascontiguousarray(x)), C.byref(T)); out[i] = _row12(T)
    return out


def oracle_edge(orc, in36):
    import ctypes as C
    L = orc.lib()
    out = np.zeros((len(in36), 6)); o = np.zeros(6)
    h, er = orc.Pose(), orc.Pose()
    for i, c in enumerate(in36):
        A, B, M = _opose(orc, c[:12]), _opose(orc, c[12:24]), _opose(orc, c[24:36])
        L.orc_pose_between(C.byref(A), C.byref(B), C.byref(h)); L.orc_pose_between(C.byref(M), C.byref(h), C.byref(er))
        L.orc_pose_log(C.byref(er), orc.dp(o)); out[i] = o
    return out


def oracle_probe(orc, p6):
    ident = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64), (2, 1))
    return np.array([orc.pg_error_at(np.stack([np.zeros(6), p]), np.zeros(0, orc.LCEDGE_DTYPE), ident) for p in p6])


def class_max(err, cls, ncls=len(CLASS_NAMES)):
    """per class id the largest entry of err (cases x components)"""
    out = np.zeros(ncls)
    e = np.asarray(err).reshape(len(cls), -1).max(axis=1)
    for c in range(ncls):
        if (cls == c).any(): out[c] = e[cls == c].max()
    return out


def oracle_floors(orc, d):
    """per class the largest |oracle - reference|: rotation part (omega, or the entries of R), translation part (v, or t), the probe's scalar"""
    ncmp = CLASS_ID["composed"]
    el = diff_to_ref(oracle_log(orc, d["log_T"]), d["log_ref_hi"], d["log_ref_lo"])
    ee = diff_to_ref(oracle_exp(orc, d["exp_xi"]), d["exp_ref_hi"], d["exp_ref_lo"])
    ec = diff_to_ref(oracle_edge(orc, d["cmp_in"]), d["cmp_ref_hi"], d["cmp_ref_lo"])
    ep = diff_to_ref(oracle_probe(orc, d["probe_xi"]), d["probe_ref_hi"], d["probe_ref_lo"])
    ccls = np.full(len(ec), ncmp)
    fw = class_max(el[:, :3], d["log_class"]) + class_max(ee[:, :9], d["exp_class"]) + class_max(ec[:, :3], ccls)
    fv = class_max(el[:, 3:], d["log_class"]) + class_max(ee[:, 9:], d["exp_class"]) + class_max(ec[:, 3:], ccls)
    return dict(floor_w=fw, floor_v=fv, floor_probe=class_max(ep, d["probe_class"]))


# ------------------------------------------------------------------ the fixture's writer
def to_bytes(d):
    """an uncompressed .npz with fixed time stamps and a fixed order: the same arrays give the same bytes"""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_STORED) as z:
        for k in sorted(d):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(d[k]), version=(1, 0), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), b.getvalue())
    return buf.getvalue()


if __name__ == "__main__":
    from oracle import binding
    data = to_bytes(generate(binding))
    with open(FIXTURE, "wb") as fh:
        fh.write(data)
    print("%s: %d bytes" % (FIXTURE, len(data)))

"""CPU: the SO(3)/SE(3) algebra every loop-closure and pose-graph number goes through (diasss_amd/csrc/dsss_pose.h, witnessed by
oracle/orc_pose.c) against an independent 50-digit restatement of GTSAM 4.2's formulas (tests/pose_algebra_ref.py), at every branch: the
Taylor, acos and near-pi branches of so3_log with their seams, permutations, ties and sign rule, the |omega| < 1e-10 exit of pose_log, the
theta^2 <= eps exit of so3_exp / pose_exp and the cancellation just above it, traces that rounding pushed outside [-1, 3], and the
Between factor's chain at kilometre coordinates.
  * the oracle is held to the reference: per class max |oracle - ref| is the class's floor F, stored in the fixture, and asserted against
    16 x the figure its conditioning gives (pose_algebra_ref.floor_figure);
  * the header, compiled for the host in a stand-alone program under the host sanitizers (diasss_amd/host/pose_check.cpp), equals the
    oracle bit for bit in every function and case;
  * the distance of GTSAM's formulas to the true exponential and logarithm is printed per class and asserted against its derived bound
    (pose_algebra_ref.gap_bound): the near-pi branch is first order in pi - theta, the small exits drop the coupling term.  That is parity
    with GTSAM, documented, not a defect.
Only the first test needs mpmath; the rest reads tests/golden/pose_algebra.npz."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import pose_algebra_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return P.load()


def _cid(name):
    return P.CLASS_ID[name]


def test_fixture_regenerates_byte_identically(orc):
    pytest.importorskip("mpmath")
    with open(P.FIXTURE, "rb") as fh:
        have = fh.read()
    assert len(have) < 200 * 1024
    assert P.to_bytes(P.generate(orc)) == have


def test_every_class_is_the_class_it_is_named_for(orc, fx):
    names = list(fx["class_names"])
    assert names == P.CLASS_NAMES
    T, cls, th = fx["log_T"], fx["log_class"], fx["log_theta"]
    br = np.array([P.log_branch(t[:9])[0] for t in T])
    sgn = np.array([P.log_branch(t[:9])[1] for t in T])
    assert (br == fx["log_branch"]).all()
    w_or = P.oracle_log(orc, T)[:, :3]
    small = np.array([P.log_small(w) for w in w_or])
    tr = (T[:, 0] + T[:, 4]) + T[:, 8]
    per_angle = P.N_RANDOM_AXES + 3
    for name, thetas in P.LOG_CLASSES:
        m = cls == _cid(name)
        assert m.any(), name
        if thetas is not None:
            assert m.sum() == len(thetas) * per_angle + 1, name                  # every angle on every axis, and one t = 0 case
            for t in thetas:
                assert (th[m] == t).sum() >= per_angle, (name, t)
        assert (np.abs(T[m, 9:]).max(axis=1) == 0).sum() == (1 if thetas is not None or 'seam' not in name else 2), name
        assert (np.abs(T[m, 9:]) <= P.T_SCALE).all()
    want = {"log_small": (P.BR_TAYLOR, True), "log_taylor_lo": (P.BR_TAYLOR, False), "log_taylor_hi": (P.BR_TAYLOR, False),
            "log_acos_lo": (P.BR_ACOS, False), "log_acos_mid": (P.BR_ACOS, False), "log_acos_hi": (P.BR_ACOS, False)}
    for name, (b, s) in want.items():
        m = cls == _cid(name)
        assert (br[m] == b).all() and (small[m] == s).all(), name
    for name in ("log_pi_outer", "log_pi_inner", "log_pi_exact"):
        m = cls == _cid(name)
        assert (br[m] >= P.BR_PI).all() and not small[m].any(), name
        assert set(br[m]) == {P.BR_PI, P.BR_PI + 1, P.BR_PI + 2}, name            # all three permutations
        assert set(sgn[m]) == {-1, 1}, name
    # the seams: neighbouring angles on one axis, one on each side
    for name, lo_side, hi_side in (("log_seam_taylor_acos", {P.BR_TAYLOR}, {P.BR_ACOS}),
                                   ("log_seam_acos_pi", {P.BR_ACOS}, {P.BR_PI, P.BR_PI + 1, P.BR_PI + 2})):
        idx = np.flatnonzero(cls == _cid(name))
        assert len(idx) == 2 * (per_angle + 1), name
        for a, b in zip(idx[0::2], idx[1::2]):
            assert br[a] in lo_side and br[b] in hi_side, (name, a)
            assert th[b] == np.nextafter(th[a], np.inf) and (T[a, 9:] == T[b, 9:]).all(), (name, a)
    # log_pi_exact: seven axes x (Wv zero, positive, negative); the ties R33 == R22 > R11, R22 == R11 and all three equal
    m = np.flatnonzero(cls == _cid("log_pi_exact"))
    assert len(m) == 22
    d = T[m][:, [0, 4, 8]]
    assert ((d[:, 2] == d[:, 1]) & (d[:, 1] > d[:, 0])).any() and ((d[:, 1] == d[:, 0]) & (d[:, 2] < d[:, 1])).any()
    assert ((d[:, 0] == d[:, 1]) & (d[:, 1] == d[:, 2])).any()
    Wv = np.array([[t[3] - t[1], t[2] - t[6], t[7] - t[5]][b - P.BR_PI] for t, b in zip(T[m], br[m])])
    for p in range(3):
        s = Wv[br[m] == P.BR_PI + p]
        assert (s == 0).any() and (s > 0).any() and (s < 0).any(), p
    # log_trace_out: a trace of 3 + ulp, and tr + 1 negative
    m = cls == _cid("log_trace_out")
    assert (tr[m] == 3.0 + 2 * P.EPS).sum() >= 6 and (tr[m] + 1.0 < 0).sum() >= 6 and ((tr[m] > 3.0) | (tr[m] + 1.0 < 0)).all()
    assert np.isfinite(P.oracle_log(orc, T[m])).all()
    # the exponential classes
    xi, ecls, eth = fx["exp_xi"], fx["exp_class"], fx["exp_theta"]
    first = np.array([P.exp_first_order(x[:3]) for x in xi])
    for name, thetas in P.EXP_CLASSES:
        m = ecls == _cid(name)
        assert m.sum() == len(thetas) * per_angle + 1, name
        assert (first[m] == (name == "exp_first_order")).all(), name
        assert (np.abs(xi[m, 3:]).max(axis=1) == 0).sum() == 1, name
        nrm = np.sqrt((xi[m, :3] ** 2).sum(axis=1))
        assert np.abs(nrm - eth[m]).max() <= 4 * P.EPS * max(thetas), name
    assert len(fx["probe_xi"]) == len(xi) + sum(len(dict(P.LOG_CLASSES)[c]) for c in P.INTERIOR) * per_angle


def test_composed_cases_sit_a_percent_from_every_threshold(orc, fx):
    """the branch of the error pose, decided on the oracle's doubles, is the one the 50-digit chain decided on its own error pose (stored
    in the fixture), and no predicate is within 1 % of its threshold"""
    cin, th = fx["cmp_in"], fx["cmp_theta"]
    L = orc.lib()
    assert len(cin) == P.N_COMPOSED_AXES * sum(1 for c in P.INTERIOR for t in dict(P.LOG_CLASSES)[c] if t not in P.NEAR_THRESHOLD)
    assert np.abs(cin[:, [9, 10, 11, 21, 22, 23]]).max() > 900
    xi_or = P.oracle_edge(orc, cin)
    seen = set()
    h, er = orc.Pose(), orc.Pose()
    for c, t, x, rhi, b50 in zip(cin, th, xi_or, fx["cmp_ref_hi"], fx["cmp_branch"]):
        A, B, M = P._opose(orc, c[:12]), P._opose(orc, c[12:24]), P._opose(orc, c[24:36])
        L.orc_pose_between(C.byref(A), C.byref(B), C.byref(h)); L.orc_pose_between(C.byref(M), C.byref(h), C.byref(er))
        R = np.array(er.R)
        br, sgn = P.log_branch(R)
        assert br == b50, t
        want = P.BR_TAYLOR if t < 1e-3 else P.BR_ACOS if t < 3.1 else P.BR_PI
        assert (br >= P.BR_PI) if want == P.BR_PI else br == want, t
        seen.add(min(br, P.BR_PI))
        tr = (R[0] + R[4]) + R[8]
        assert abs((tr + 1.0) / 1e-3 - 1) > 0.01 and abs((tr - 3.0) / -1e-6 - 1) > 0.01
        assert abs(np.sqrt((x[:3] ** 2).sum()) / 1e-10 - 1) > 0.01 and not P.log_small(x[:3])
        if br >= P.BR_PI:
            dg = R[[0, 4, 8]]
            assert min(abs(dg[0] - dg[1]), abs(dg[1] - dg[2]), abs(dg[0] - dg[2])) > 0.01
            s = np.array([R[7] - R[5], R[2] - R[6], R[3] - R[1]])
            assert np.abs(s).min() > 0.01 * np.abs(s).max()
        assert np.abs(x - rhi).max() < 1e-9
    assert seen == {P.BR_TAYLOR, P.BR_ACOS, P.BR_PI}


def test_oracle_against_the_reference_per_class(orc, fx):
    got = P.oracle_floors(orc, fx)
    print("\n%-22s %11s %11s %11s %11s %11s" % ("class", "F rot", "figure x16", "F trans", "figure x16", "F probe"))
    bad = []
    for name in P.CLASS_NAMES:
        c = _cid(name)
        if name == "composed": thetas = [3.0]
        elif name.startswith("exp"): thetas = fx["exp_theta"][fx["exp_class"] == c]
        else: thetas = fx["log_theta"][fx["log_class"] == c]
        fw, fv = P.floor_figure(name, thetas)
        print("%-22s %11.3g %11.3g %11.3g %11.3g %11.3g" % (name, got["floor_w"][c], 16 * fw, got["floor_v"][c], 16 * fv, got["floor_probe"][c]))
        if not (got["floor_w"][c] <= 16 * fw and got["floor_v"][c] <= 16 * fv): bad.append(name)
    assert not bad, bad
    for k in ("floor_w", "floor_v", "floor_probe"):                              # the floors the device test judges by are these
        assert (got[k] == fx[k]).all(), k
    assert np.isfinite(fx["log_ref_hi"]).all() and np.isfinite(fx["exp_ref_hi"]).all() and np.isfinite(fx["cmp_ref_hi"]).all()


def _records(fx):
    """every function of the header on the fixture's cases -> (records for pose_check, the oracle's outputs in pose_check's layout)"""
    T, xi, cin = fx["log_T"], fx["exp_xi"], fx["cmp_in"]
    n = len(T)
    recs = []

    def add(fid, *parts):
        r = np.zeros(40); r[0] = fid
        v = np.concatenate([np.asarray(p, np.float64).ravel() for p in parts]); r[1:1 + len(v)] = v
        recs.append(r)
    for t in T:
        add(P.F_SO3_LOG, t[:9]); add(P.F_POSE_LOG, t); add(P.F_INVERSE, t); add(P.F_ADJOINT, t); add(P.F_RPY, t)
    for i in range(n):
        add(P.F_BETWEEN, T[i], T[(i + 1) % n]); add(P.F_COMPOSE, T[i], T[(i + 7) % n]); add(P.F_RETRACT, T[i], xi[i % len(xi)])
    for x in list(xi) + list(fx["probe_xi"]):
        add(P.F_SO3_EXP, x[:3]); add(P.F_POSE_EXP, x); add(P.F_RODRIGUES, x)
    for c in cin:
        add(P.F_EDGE, c)
    return np.array(recs)


def _oracle_outputs(orc, recs):
    L = orc.lib()
    out = np.zeros((len(recs), 36))
    o36 = np.zeros(36); O = orc.Pose()
    pose = lambda a: P._opose(orc, a)
    for i, r in enumerate(recs):
        fid, a = int(r[0]), np.ascontiguousarray(r[1:])
        o36[:] = 0
        if fid == P.F_SO3_EXP: L.orc_so3_exp(orc.dp(a), orc.dp(o36)); out[i] = o36
        elif fid == P.F_SO3_LOG: L.orc_so3_log(orc.dp(a), orc.dp(o36)); out[i] = o36
        elif fid == P.F_POSE_EXP: L.orc_pose_exp(orc.dp(a), C.byref(O)); out[i, :12] = P._row12(O)
        elif fid == P.F_POSE_LOG: L.orc_pose_log(C.byref(pose(a)), orc.dp(o36)); out[i] = o36
        elif fid == P.F_BETWEEN: L.orc_pose_between(C.byref(pose(a)), C.byref(pose(a[12:])), C.byref(O)); out[i, :12] = P._row12(O)
        elif fid == P.F_INVERSE: L.orc_pose_inverse(C.byref(pose(a)), C.byref(O)); out[i, :12] = P._row12(O)
        elif fid == P.F_COMPOSE: L.orc_pose_compose(C.byref(pose(a)), C.byref(pose(a[12:])), C.byref(O)); out[i, :12] = P._row12(O)
        elif fid == P.F_ADJOINT: L.orc_pose_adjoint(C.byref(pose(a)), orc.dp(o36)); out[i] = o36
        elif fid == P.F_RETRACT: L.orc_pose_retract(C.byref(pose(a)), orc.dp(np.ascontiguousarray(a[12:18])), C.byref(O)); out[i, :12] = P._row12(O)
        elif fid == P.F_RPY: L.orc_pose_rpy(C.byref(pose(a)), orc.dp(o36)); out[i] = o36
        elif fid == P.F_RODRIGUES: L.orc_pose_from_rodrigues(orc.dp(a), C.byref(O)); out[i, :12] = P._row12(O)
        elif fid == P.F_EDGE: out[i, :6] = P.oracle_edge(orc, a[None, :36])[0]
    return out


def test_host_build_of_the_header_equals_the_oracle_bit_for_bit(orc, fx, tmp_path):
    host = os.path.join(ROOT, "diasss_amd", "host")
    subprocess.check_call(["make", "-C", host, "-s", "pose_check"])
    recs = _records(fx)
    fin, fout = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    recs.tofile(fin)
    run = subprocess.run([os.path.join(host, "pose_check"), fin, fout], capture_output=True, text=True, timeout=120)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "pose_check: ok, %d records" % len(recs) in run.stdout
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error:" not in run.stderr
    got = np.fromfile(fout).reshape(len(recs), 36)
    want = _oracle_outputs(orc, recs)
    names = ["so3_exp", "so3_log", "pose_exp", "pose_log", "pose_between", "pose_inverse", "pose_compose", "pose_adjoint", "pose_retract",
             "pose_rpy", "pose_from_rodrigues", "edge error"]
    bad = []
    for fid, name in enumerate(names):
        m = recs[:, 0] == fid
        same = (got[m].view(np.uint64) == want[m].view(np.uint64)) | ((got[m] == 0) & (want[m] == 0))      # (+0 and -0: the same number)
        print("%-20s %5d cases, %d differ" % (name, m.sum(), (~same.all(axis=1)).sum()))
        assert m.sum() > 0
        if not same.all(): bad.append(name)
    assert not bad, bad
    assert np.isfinite(got).all()


def test_gap_between_gtsam_formulas_and_the_true_maps(fx):
    """measured, and asserted only against the derived bound plus 16 x the class's floor figure"""
    print("\n%-22s %11s %11s %11s %11s" % ("class", "gap rot", "bound", "gap trans", "bound"))
    bad = []
    for kind, names in (("log", [c for c, _ in P.LOG_CLASSES]), ("exp", [c for c, _ in P.EXP_CLASSES])):
        cls, th, gap = fx[kind + "_class"], fx[kind + "_theta"], fx[kind + "_gap"]
        tn = np.sqrt((fx["log_T"][:, 9:] ** 2).sum(axis=1)) if kind == "log" else np.sqrt((fx["exp_xi"][:, 3:] ** 2).sum(axis=1))
        for name in names:
            m = np.flatnonzero(cls == _cid(name))
            fw, fv = P.floor_figure(name, th[m])
            b = np.array([P.gap_bound(name, th[i], tn[i]) for i in m]) + 16 * np.array([fw, fv])
            print("%-22s %11.3g %11.3g %11.3g %11.3g" % (name, gap[m, 0].max(), b[:, 0].max(), gap[m, 1].max(), b[:, 1].max()))
            if not (gap[m] <= b).all(): bad.append(name)
    assert not bad, bad

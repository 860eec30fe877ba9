"""CPU: what the device probe (diasss_amd/host/dev_probe.hip, run by tests/test_gpu_dev_probe.py) rests on, checked without a GPU.
  * the probe builds for gfx950 with no warning located in its own file, and its code-generation flags are the library's;
  * tests/golden/dev_probe.npz regenerates byte for byte (needs mpmath), every case is in the class it is named for, and the oracle's
    floors F = max |oracle - 50-digit reference| are the stored ones and at most 16 x the figure the conditioning gives
    (dev_probe_ref.*_floor_figure, derived in their comments) -- the project's pattern and margin (test_pose_algebra_cpu.py);
  * orc_sss_factor is held to the mpmath restatement of the reference project's SssPointFactor::evaluateError (plan_a), the p == T.t cases
    by their pattern of NaNs;
  * orc_sincos against mpmath on the probe's whole argument list: 4.5e-16 up to |x| = 4 pi + pi / 2, beyond that the bound the two-term
    reduction gives, derived in test_oracle_sincos_against_50_digits;
  * the case lists can show what they are for: the Cholesky blocks reach condition numbers of 1e12, the four bad-pivot paths are taken, and
    the f64 scan vectors give other bits in butterfly order than summed left to right."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import dev_probe_ref as D
from tests import pose_algebra_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "diasss_amd", "host")
CODEGEN = ["-O3", "-std=c++17", "--offload-arch=$(ARCH)", "-ffp-contract=off", "-fno-fast-math"]


@pytest.fixture(scope="module")
def fx():
    return P.load()


@pytest.fixture(scope="module")
def dx():
    return D.load()


def _make_var(path, name):
    with open(path) as fh:
        m = re.search(r"^%s\s*\??=\s*(.*)$" % name, fh.read(), re.M)
    assert m, (path, name)
    return m.group(1).split()


def test_probe_is_built_with_the_library_code_generation_flags():
    """every flag of the library's CXXFLAGS that can change a computed number (-O, -std, the architecture, -f...) is a flag of the probe and
    the other way round; what is left on either side is -fPIC and warnings"""
    lib = _make_var(os.path.join(ROOT, "diasss_amd", "csrc", "Makefile"), "CXXFLAGS")
    probe = _make_var(os.path.join(HOST, "Makefile"), "PROBE_CODEGEN")
    arch_lib = _make_var(os.path.join(ROOT, "diasss_amd", "csrc", "Makefile"), "ARCH")
    arch_probe = _make_var(os.path.join(HOST, "Makefile"), "ARCH")
    codegen = lambda flags: sorted(f for f in flags if not f.startswith("-W") and f != "-fPIC")
    assert codegen(lib) == codegen(probe) == sorted(CODEGEN)
    assert arch_lib == arch_probe == ["gfx950"]
    with open(os.path.join(HOST, "Makefile")) as fh:
        rule = re.search(r"^dev_probe:.*\n\t(.*)$", fh.read(), re.M).group(1)
    assert "$(PROBE_CODEGEN)" in rule and "sanitize" not in rule
    assert [f for f in rule.split() if f.startswith("-") and not f.startswith("-W")] == ["-o"]      # nothing else that could change the code


def test_probe_builds_for_gfx950_without_a_warning_of_its_own():
    run = subprocess.run(["make", "-C", HOST, "-B", "dev_probe"], capture_output=True, text=True, timeout=600)
    print(run.stdout[-2000:], run.stderr[-4000:])
    assert run.returncode == 0
    assert os.path.exists(os.path.join(HOST, "dev_probe"))
    own = [l for l in (run.stdout + run.stderr).splitlines() if re.match(r"^(\./)?(dev_probe\.hip|lm_rule_table\.h|\./lm_rule_table\.h):\d+:\d+: (warning|error)", l)]
    assert not own, own


def test_fixture_regenerates_byte_identically(orc):
    pytest.importorskip("mpmath")
    with open(D.FIXTURE, "rb") as fh:
        have = fh.read()
    assert len(have) < 200 * 1024
    assert P.to_bytes(D.generate(orc)) == have


def test_every_case_is_in_the_class_it_is_named_for(orc, fx, dx):
    # gimbal: every combination of signed zeros at |R20| == 1 and one ulp either side, and the rotation-like neighbours
    g = dx["gimbal_T"]
    assert (g == D.gimbal_cases()).all() and (np.signbit(g) == np.signbit(D.gimbal_cases())).all()
    kind = np.array([D.gimbal_kind(t) for t in g])
    for s in (1.0, -1.0):
        for k in (0, 1, 2):
            m = (kind == k) & (np.sign(g[:, 6]) == s) & (g[:, 7] == 0) & (g[:, 8] == 0)
            assert m.sum() == 16, (s, k)
            sig = {tuple(np.signbit(t[[7, 8, 3, 0]])) for t in g[m]}
            assert len(sig) == 16, (s, k)                                         # all signs of the four zeros
        m = (kind == 1) & (np.sign(g[:, 6]) == s) & (g[:, 7] != 0)
        assert m.sum() == 4
        h = np.sqrt(g[m, 7] ** 2 + g[m, 8] ** 2)
        assert np.abs(h / np.sqrt(1.0 - g[m, 6] ** 2) - 1).max() < 1e-6           # the R21, R22 a rotation one ulp inside would have
    assert (kind >= 0).all()
    assert np.nextafter(1.0, 0) == 1.0 - D.EPS / 2 and np.nextafter(1.0, 2) == 1.0 + D.EPS
    # retract: interior log classes x every exp class
    ti, xi = D.retract_index(fx)
    assert set(fx["log_class"][ti]) == {P.CLASS_ID[c] for c in P.INTERIOR}
    assert set(fx["exp_class"][xi]) == {P.CLASS_ID[c] for c in D.RETRACT_CLASS_NAMES}
    assert len(ti) == len(dx["retract_ref_hi"]) > 200
    first = np.array([P.exp_first_order(x[:3]) for x in fx["exp_xi"][xi]])
    assert (first == (fx["exp_class"][xi] == P.CLASS_ID["exp_first_order"])).all()
    # sss_factor
    sin, scls, srange = D.sss_cases()
    assert (sin == dx["sss_in"]).all() and (scls == dx["sss_class"]).all() and (srange == dx["sss_range"]).all()
    p, T = sin[:, :3], sin[:, 3:15]
    R = T[:, :9].reshape(-1, 3, 3)
    tilt = np.degrees(np.arccos(R[:, 2, 2]))
    assert tilt.min() > 1 and tilt.max() > 15                                     # tilted poses
    assert np.abs(T[:, 9:]).max() > 900                                           # coordinates of a kilometre
    m = scls == 0
    assert m.sum() == D.SSS_POSES * len(D.SSS_RANGES)
    for r in D.SSS_RANGES:
        assert (np.abs(srange[m] / r - 1) < 1e-9).sum() == D.SSS_POSES, r         # slant ranges 0.5 ... 150 m
    assert (np.abs(sin[m, 15] / srange[m] - 1) < 1e-9).all()                      # mx next to the range: nrm - mx cancels
    m = scls == 1
    assert m.sum() == 4 * D.SSS_POSES
    steps = np.abs(p[m] - T[m, 9:]) / P.ulp(T[m, 9:])
    assert set(steps.ravel()) <= {0.0, 2.0} and (steps.max(axis=1) == 2).all() and (steps.min(axis=1) == 2).any()
    m = scls == 2
    assert m.sum() == 4 and (p[m] == T[m, 9:]).all()
    # the non-finite pattern of p == T.t: the two rows divided by the norm, nothing else
    nan = np.isnan(dx["sss_ref_hi"])
    want = np.zeros(20, bool); want[2:5] = True; want[8:14] = True
    assert (nan[m] == want).all() and not nan[~m].any()


def test_oracle_floors_are_stored_and_bounded(orc, fx, dx):
    got = D.oracle_floors(orc, dx, fx)
    for k in ("floor_rpy", "floor_retract_w", "floor_retract_v", "floor_sss"):
        assert (got[k] == dx[k]).all(), k
    bad = []
    print("\n%-22s %11s %11s %11s %11s %11s %11s" % ("class", "F", "figure x16", "F", "figure x16", "F", "figure x16"))
    fig = D.rpy_floor_figure()
    for c, name in enumerate(D.RPY_CLASS_NAMES):
        print("rpy %-18s %11.3g %11.3g" % (name, dx["floor_rpy"][c], 16 * fig))
        if not dx["floor_rpy"][c] <= 16 * fig: bad.append("rpy " + name)
    ti, xi = D.retract_index(fx)
    for c, name in enumerate(D.RETRACT_CLASS_NAMES):
        th = fx["exp_theta"][fx["exp_class"] == P.CLASS_ID[name]]
        fw, fv = D.retract_floor_figure(name, th)
        print("retract %-14s %11.3g %11.3g %11.3g %11.3g" % (name, dx["floor_retract_w"][c], 16 * fw, dx["floor_retract_v"][c], 16 * fv))
        if not (dx["floor_retract_w"][c] <= 16 * fw and dx["floor_retract_v"][c] <= 16 * fv): bad.append("retract " + name)
    for c, name in enumerate(D.SSS_CLASS_NAMES):
        f = D.sss_floor_figure(name, dx["sss_range"][dx["sss_class"] == c].max())
        print("%-22s %11.3g %11.3g %11.3g %11.3g %11.3g %11.3g" % (name, dx["floor_sss"][c, 0], 16 * f[0], dx["floor_sss"][c, 1], 16 * f[1],
                                                                   dx["floor_sss"][c, 2], 16 * f[2]))
        if not (dx["floor_sss"][c] <= 16 * np.array(f)).all(): bad.append(name)
    assert not bad, bad


def test_oracle_sss_factor_against_the_restatement(orc, dx):
    """orc_sss_factor with Ts = identity against the 50-digit restatement, per class and part within 16 x the figure; where the reference
    is not a number (p == T.t) the oracle is not one either, and nowhere else"""
    o = D.oracle_sss(orc, dx["sss_in"])
    nan = np.isnan(dx["sss_ref_hi"])
    assert (np.isnan(o) == nan).all() and np.isfinite(o[~nan]).all()
    err = np.where(nan, 0.0, P.diff_to_ref(o, dx["sss_ref_hi"], dx["sss_ref_lo"]))
    for c, name in enumerate(D.SSS_CLASS_NAMES):
        m = dx["sss_class"] == c
        f = D.sss_floor_figure(name, dx["sss_range"][m].max())
        for part, fig in zip(D.SSS_PARTS, f):
            assert err[m][:, part].max() <= 16 * fig, (name, part)
    # the translation block is -(Rs^T R^T) as the reference writes it, the rotation block [p_m]x: signs and places, on one case by hand
    r = dx["sss_in"][3]
    R = r[3:12].reshape(3, 3); pm = R.T @ (r[:3] - r[12:15])
    H2 = o[3, 8:20].reshape(2, 6)
    assert np.allclose(H2[1, 3:], -R.T[0], rtol=0, atol=1e-15) and np.allclose(H2[1, :3], [0, -pm[2], pm[1]], rtol=0, atol=1e-12)
    assert np.allclose(H2[0, 3:], -(pm / np.linalg.norm(pm)) @ R.T, rtol=0, atol=1e-14)


def test_oracle_sincos_against_50_digits(orc):
    """|x| <= 4 pi + pi / 2: the project's own bar, 4.5e-16 (2 ulp of 1.0), now against mpmath and on the probe's list.
    Beyond: r = (x - k pio2_1) - k pio2_1t with k = rint(x * invpio2).  pio2_1 has 33 significant bits and |k| < 2^20 on the list, so
    k * pio2_1 is exact, and x - k * pio2_1, a multiple of 2^-52 below 1 in size, is exact too.  What is left is (a) pi / 2 - pio2_1 - pio2_1t,
    the rounding of the tail constant, |k| times, (b) the rounding of the product k * pio2_1t, half an ulp of it, and (c) the rounding of the
    last subtraction, which the bar for small arguments already contains.  (a) + (b) are measured below from the constants in 50 digits and
    are at most |k| ulp(pio2_1t); sin and cos move by at most the error of their argument.  So: |k| ulp(pio2_1t) + 2 ulp."""
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp
    x = D.sincos_args()
    assert len(x) == 3 * 72001 + 17 * 2 * 9 + 2 + 6 * 52
    o = D.oracle_sincos(orc, x)
    with mp.workdps(40):
        vals = [mp.cos_sin(mp.mpf(float(t)))[::-1] for t in x]                     # (sin, cos)
        ref = np.array([[float(v) for v in sc] for sc in vals])
        tail = abs(mp.pi / 2 - mp.mpf(D.PIO2_1) - mp.mpf(D.PIO2_1T))
        ulp_t = float(P.ulp(D.PIO2_1T))
        k = np.rint(x * D.INVPIO2)
        assert np.abs(k).max() < 2 ** 20 and np.abs(k).max() > 6e5
        m33 = mp.mpf(D.PIO2_1) * 2 ** 32
        assert m33 == int(m33) and int(m33) < 2 ** 33                              # pio2_1: 33 significant bits
        reduction = np.array([float(abs(mp.mpf(float(q))) * tail + abs(mp.mpf(float(q) * D.PIO2_1T) - mp.mpf(float(q)) * mp.mpf(D.PIO2_1T))) for q in np.unique(np.abs(k))])
        assert (reduction <= np.unique(np.abs(k)) * ulp_t).all()                   # (a) + (b) <= |k| ulp(pio2_1t)
        # the error against the 40-digit value itself, not against its rounding to double
        err = np.array([[float(abs(mp.mpf(float(a)) - v)) for a, v in zip(row, sc)] for row, sc in zip(o, vals)]).max(axis=1)
    near = np.abs(x) <= D.SINCOS_NEAR
    assert near.sum() > 3 * 72001 and (~near).sum() >= 5 * 48
    print("\n|x| <= 4 pi + pi / 2: %d arguments, largest error %.3g" % (near.sum(), err[near].max()))
    assert err[near].max() <= 4.5e-16
    bound = np.abs(k) * ulp_t + 4.5e-16
    for d in range(2, 7):                                                          # (the first decade lies below 4 pi + pi / 2)
        m = ~near & (np.abs(x) > 10.0 ** (d - 1)) & (np.abs(x) <= 10.0 ** d)
        print("1e%d < |x| <= 1e%d: %3d arguments, largest error %.3g, bound %.3g" % (d - 1, d, m.sum(), err[m].max(), bound[m].max()))
        assert m.sum() >= 40
    assert (err[~near] <= bound[~near]).all()
    assert np.abs(ref - o).max() <= 4.5e-16                                        # (and against the correctly rounded values)


def test_atan2_and_geo_lists_cover_what_they_name():
    yx = D.atan2_pairs()
    assert len(yx) == 511 * 511 + 20000 and yx.dtype == np.float32
    g = yx[:511 * 511]
    assert len(np.unique(g, axis=0)) == 511 * 511 and np.abs(g).max() == 255 and (g == 0).all(axis=1).sum() == 1
    m = yx[511 * 511:]
    assert np.abs(m).max() == D.IC_MAX and (m == m.astype(np.int64)).all()
    assert {(int(np.sign(a)), int(np.sign(b))) for a, b in m} == {(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)}
    rows = D.geo_cases()
    for M in (4, 6, 32):
        r = rows[rows[:, 6] == M]
        half = M // 2
        assert set(r[:, 7]) == {0, 1, half - 1, half, half + 1, M - 1}
        for yaw in (0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi):
            assert (r[:, 2] == yaw).sum() == len(set(r[:, 7]))
        assert (r[:, 8:8 + half] > 0).all() and (r[:, 8 + half:] == 0).all()


def test_cholesky_cases_reach_every_path():
    A, kind = D.chol_cases()
    cond = np.array([np.linalg.cond(a.reshape(6, 6)) for a in A[kind == 0]])
    print("\ncondition numbers of the scaled blocks: %.3g ... %.3g, %d of %d at 1e12 and above" % (cond.min(), cond.max(), (cond >= 1e12).sum(), len(cond)))
    assert cond.max() >= 1e12 and (cond >= 1e12).sum() >= len(cond) // 2
    L, ri, bad = D.chol6_recip_np(A)
    assert (bad[kind <= 1] == 0).all() and (bad[kind >= 2] == 1).all()
    Lm = L.reshape(-1, 6, 6)
    ok = kind == 0
    Lt = np.tril(Lm[ok])
    rel = np.abs(Lt @ Lt.transpose(0, 2, 1) - A[ok].reshape(-1, 6, 6)) / (np.abs(Lt) @ np.abs(Lt).transpose(0, 2, 1))
    assert rel.max() < 1e-14                                                       # the restatement is a Cholesky factorisation
    assert (Lm[kind == 1][0] == np.eye(6)).all() and (ri[kind == 1] == 1).all()
    z = Lm[kind == 2][0]
    assert z[2, 2] == 1.0 and z[0, 0] == 2.0 and z[1, 1] == 3.0                    # the zero pivot, replaced by 1, after two exact ones
    assert Lm[kind == 3][0][2, 2] == 1.0
    assert np.isnan(Lm[kind == 4][0][3, 1]) and Lm[kind == 4][0][3, 3] == 1.0      # NaN reaches the pivot of its row
    assert Lm[kind == 5][0][4, 4] == 1.0 and Lm[kind == 5][0][5, 5] == 2.0         # +inf is refused, the next pivot is untouched


def test_scan_vectors_can_tell_the_order():
    vecs = D.scan_vectors()
    assert [len(v) for c, v in vecs if c == 2] == D.SCAN_N
    diff = total = 0
    for code, v in vecs:
        x = D.pad256(v)
        if code == 0:
            assert (v == 0).any() and (v != 0).any() or len(v) < 4
            assert int(v.astype(np.int64).sum()) < 2 ** 31
        if code == 1 and len(v) >= 63:
            assert sum(int(t) for t in v) > 2 ** 63                                # the running sum passes 2^63
        if code == 2:
            w = x.reshape(-1, 64)
            seq = np.array([D.sum_in_order(r, np.float64(0)) for r in w])
            full = np.array([len(v) - 64 * i >= 64 for i in range(len(w))])
            b = D.wave_sum_np(v)
            diff += (b[full] != seq[full]).sum(); total += full.sum()
            assert np.abs(b - seq).max() <= 64 * D.EPS * np.abs(w).sum(axis=1).max()
        # the emulations agree with numpy where the arithmetic is exact
        if code != 2:
            pre, tot = D.carried_scan_np(v)
            cs = np.cumsum(v, dtype=v.dtype)
            assert (pre == cs - v).all() and tot == cs[-1]
            assert (D.wave_sum_np(v) == x.reshape(-1, 64).sum(axis=1, dtype=v.dtype)).all()
    print("\nf64: the butterfly and the left-to-right sum differ in %d of %d full wavefronts" % (diff, total))
    assert diff * 2 >= total

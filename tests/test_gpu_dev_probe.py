"""GPU: the kernels' shared __device__ helpers, each on its own, as the device computes them.  diasss_amd/host/dev_probe.hip includes the
headers as the kernels do and is built with the library's code-generation flags (tests/test_dev_probe_cpu.py compares the two Makefiles); the
module builds it, runs each of its two modes ONCE as a child process and judges what it wrote.  Cases and references: tests/dev_probe_ref.py,
tests/pose_algebra_ref.py and their fixtures; the oracle is computed here.  If a child exits non-zero every test fails with its output and
nothing is started again.

Bit for bit with the oracle, +0 and -0 being the same number -- everything made of + - * / and sqrt: pose_between, pose_inverse, pose_compose,
pose_adjoint, the Taylor omega of so3_log / pose_log and pose_log's small exit, the first-order exponentials (and a retract by one), sss_factor
with all of H1 and H2 (p == T.t: the same places are NaN), dsss_sincos on its whole list (|x| up to 1e6), dsss_geo_at, fast_atan2_dev on every
pair, factor_eval's Jacobian -Ad(h^-1) w made from the oracle's between, inverse and adjoint with one multiply, chol6_recip against a literal
numpy restatement of its loop (flags and substituted pivots included), the integer scans against numpy.cumsum, and the f64 wave and block
sums against a numpy emulation of the 32 -> 1 butterfly and the ((s0 + s1) + s2) + s3 order.

Where the device's libm enters (sin, acos, tan, atan2): so3_exp, pose_exp, pose_from_rodrigues, pose_retract, so3_log, pose_log, pose_rpy, the
edge chain -- the project's rule, unchanged (tests/test_gpu_pose_algebra.py): |q - r| <= 8 F + 4 ulp(r) per class for the 50-digit reference r
and the class's floor F = max |oracle - r| stored in the fixtures, rotation and translation parts apart.  The bit-equal share is printed.
factor_eval's residual goes through that chain too: it must equal the device's own chain (function id 11, judged by the rule) times w bit for
bit -- one multiply -- which is the oracle's edge error times w wherever the chain equals the oracle's.

chol6_rdiag (the device's rsqrt): the componentwise backward error |A - L L^T| <= gamma_11 |L| |L|^T in long double (dev_probe_ref.
rdiag_backward_error), and rsqrt itself within 2 ulp of 1 / sqrt(d) in long double on the pivots it was given, which is what gamma_11 assumes.

Measured on an MI355X (ROCm 7, gfx950), largest |q - r| / F per function over its classes and the bit-equal share, are in DESIGN.md,
"Device helpers on their own"."""
import os
import subprocess

import numpy as np
import pytest

from tests import dev_probe_ref as D
from tests import pose_algebra_ref as P
from tests.test_pose_algebra_cpu import _oracle_outputs, _records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "diasss_amd", "host")


def _child(args):
    run = subprocess.run(args, capture_output=True, text=True, timeout=120)
    return run.returncode, run.stdout + run.stderr


@pytest.fixture(scope="module")
def probe(orc, tmp_path_factory):
    """builds the probe, runs `dev_probe IN OUT` and `dev_probe --scan IN OUT` once each -> everything the tests read, or the failure"""
    fx, dx = P.load(), D.load()
    r = dict(fx=fx, dx=dx, failure=None)
    mk = subprocess.run(["make", "-C", HOST, "-s", "dev_probe"], capture_output=True, text=True, timeout=600)
    if mk.returncode != 0:
        r["failure"] = "make dev_probe failed:\n" + mk.stdout + mk.stderr
        return r
    exe = os.path.join(HOST, "dev_probe")
    tmp = tmp_path_factory.mktemp("dev_probe")

    pose = _records(fx)
    groups = [("pose", np.pad(pose, ((0, 0), (0, D.IN_W - pose.shape[1]))))]
    r["pose_recs"] = pose
    add = lambda name, rows: groups.append((name, np.array(rows)))
    add("gimbal", [D.rec(P.F_RPY, t) for t in dx["gimbal_T"]])
    add("sss", [D.rec(D.F_SSS, row) for row in dx["sss_in"]])
    r["sincos_x"] = D.sincos_args()
    add("sincos", D.packed(D.F_SINCOS, r["sincos_x"], D.SINCOS_PER_REC, 1))
    r["geo_rows"] = D.geo_cases()
    add("geo", [D.rec(D.F_GEO, row) for row in r["geo_rows"]])
    r["atan2_yx"] = D.atan2_pairs()
    add("atan2", D.packed(D.F_ATAN2, r["atan2_yx"], D.ATAN2_PER_REC, 2))
    r["factor_rows"] = D.factor_cases(fx)
    add("factor", [D.rec(D.F_FACTOR, row) for row in r["factor_rows"]])
    add("factor_chain", [D.rec(P.F_EDGE, row[:36]) for row in r["factor_rows"]])
    r["chol_A"], r["chol_kind"] = D.chol_cases()
    add("chol_recip", [D.rec(D.F_CHOL_RECIP, a) for a in r["chol_A"]])
    add("chol_rdiag", [D.rec(D.F_CHOL_RDIAG, a) for a in r["chol_A"]])
    add("lm", [D.rec(D.F_LM, [k, i]) for k in range(D.LM_KINDS) for i in range(D.LM_ROWS_ASKED)])
    allrecs = np.concatenate([g for _, g in groups])
    fin, fout = str(tmp / "records.bin"), str(tmp / "records.out")
    allrecs.tofile(fin)
    code, out = _child([exe, fin, fout])
    print(out)
    if code != 0 or "dev_probe: ok, %d records" % len(allrecs) not in out:
        r["failure"] = "dev_probe exited %d:\n%s" % (code, out)
        return r
    got = np.fromfile(fout).reshape(len(allrecs), D.OUT_W)
    at = 0
    for name, g in groups:
        r[name] = got[at:at + len(g)]; at += len(g)

    r["vecs"] = D.scan_vectors()
    fin, fout = str(tmp / "scan.bin"), str(tmp / "scan.out")
    D.scan_file(r["vecs"]).tofile(fin)
    code, out = _child([exe, "--scan", fin, fout])
    print(out)
    if code != 0 or "dev_probe: ok, %d sections" % len(r["vecs"]) not in out:
        r["failure"] = "dev_probe --scan exited %d:\n%s" % (code, out)
        return r
    r["scan"] = D.scan_parse(r["vecs"], np.fromfile(fout, np.int64))
    return r


@pytest.fixture
def prx(probe, orc):
    if probe["failure"]:
        pytest.fail(probe["failure"])
    probe["orc"] = orc
    return probe


def _same(got, want):
    """bit for bit, +0 and -0 being the same number and a NaN a NaN"""
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    return (got.view(np.uint64) == want.view(np.uint64)) | ((got == 0) & (want == 0)) | (np.isnan(got) & np.isnan(want))


def _report_same(name, got, want):
    ok = _same(got, want)
    rows = ok.reshape(len(ok), -1).all(axis=1)
    print("%-22s %6d cases, %d differ" % (name, len(rows), (~rows).sum()))
    return bool(rows.all())


def _rows(pr, fid):
    """(inputs, device outputs, oracle outputs) of the pose records of one function id"""
    m = pr["pose_recs"][:, 0] == fid
    if "pose_oracle" not in pr:
        pr["pose_oracle"] = _oracle_outputs(pr["orc"], pr["pose_recs"])
        assert (pr["pose"][:, 36:] == 0).all()                                     # the record's unused outputs stay zero
    return pr["pose_recs"][m, 1:], pr["pose"][m, :36], pr["pose_oracle"][m]


def _part_ulp(r):
    return P.ulp(np.abs(r).max(axis=1))


def _judge(what, q, hi, lo, cls, names, Fw, Fv, oracle, nrot):
    """the pass rule on rows of nrot rotation-part components followed by the translation part (possibly none); prints per class the
    largest |q - r| / F and the bit-equal share; -> the classes that miss"""
    err = P.diff_to_ref(q, hi, lo)
    bad = []
    for c in np.unique(cls):
        m = cls == c
        ew = err[m, :nrot].max(axis=1); tw = 8 * Fw[c] + 4 * _part_ulp(hi[m, :nrot])
        ok = (ew <= tw).all()
        with np.errstate(divide="ignore", invalid="ignore"):
            line = "%s %-22s max|q-r|/F rot %9.3g" % (what, names[c], np.nan_to_num(ew.max() / Fw[c], nan=0.0))
            if q.shape[1] > nrot:
                ev = err[m, nrot:].max(axis=1); tv = 8 * Fv[c] + 4 * _part_ulp(hi[m, nrot:])
                ok = ok and (ev <= tv).all()
                line += " trans %9.3g" % np.nan_to_num(ev.max() / Fv[c], nan=0.0)
        eq = _same(q[m], oracle[m]).all(axis=1).sum()
        print("%s   bit-equal to the oracle %3d of %3d" % (line, eq, m.sum()))
        if not ok: bad.append("%s %s" % (what, names[c]))
    return bad


# ------------------------------------------------------------------ + - * / and sqrt: bit for bit
def test_algebra_without_libm_is_the_oracle_bit_for_bit(prx):
    fx = prx["fx"]
    print()
    bad = []
    for fid in (P.F_BETWEEN, P.F_INVERSE, P.F_COMPOSE, P.F_ADJOINT):
        _, q, o = _rows(prx, fid)
        assert len(q) == len(fx["log_T"])
        if not _report_same(D.NAMES[fid], q[:, :36], o): bad.append(D.NAMES[fid])
    # the Taylor branch's omega, and pose_log's small exit (omega and the copied translation)
    taylor = fx["log_branch"] == P.BR_TAYLOR
    small = fx["log_class"] == P.CLASS_ID["log_small"]
    assert taylor.sum() > 100 and small.sum() > 40
    for fid in (P.F_SO3_LOG, P.F_POSE_LOG):
        _, q, o = _rows(prx, fid)
        if not _report_same(D.NAMES[fid] + " Taylor omega", q[taylor, :3], o[taylor, :3]): bad.append(D.NAMES[fid])
    _, q, o = _rows(prx, P.F_POSE_LOG)
    if not _report_same("pose_log small exit", q[small, :6], o[small, :6]): bad.append("pose_log small")
    # the first-order exponential: R = I + W, t = v
    n_exp = len(fx["exp_xi"])
    first = fx["exp_class"] == P.CLASS_ID["exp_first_order"]
    for fid in (P.F_SO3_EXP, P.F_POSE_EXP, P.F_RODRIGUES):
        _, q, o = _rows(prx, fid)
        if not _report_same(D.NAMES[fid] + " first order", q[:n_exp][first, :12], o[:n_exp][first, :12]): bad.append(D.NAMES[fid])
    a, q, o = _rows(prx, P.F_RETRACT)
    f1 = np.array([P.exp_first_order(x[12:15]) for x in a])
    assert f1.sum() > 40
    if not _report_same("pose_retract by a first-order step", q[f1, :12], o[f1, :12]): bad.append("retract")
    # the translation of pose_from_rodrigues is copied
    a, q, _ = _rows(prx, P.F_RODRIGUES)
    assert _same(q[:, 9:12], a[:, 3:6]).all()
    assert not bad, bad


def test_sss_factor_is_the_oracle_bit_for_bit(prx, orc):
    dx = prx["dx"]
    q = prx["sss"][:, :20]
    o = D.oracle_sss(orc, dx["sss_in"])
    print()
    for c, name in enumerate(D.SSS_CLASS_NAMES):
        m = dx["sss_class"] == c
        ok = [_report_same("%s %s" % (name, part), q[m][:, sl], o[m][:, sl]) for part, sl in zip(("e", "H1", "H2"), D.SSS_PARTS)]
        assert all(ok), name
    nan = np.isnan(dx["sss_ref_hi"])
    assert (np.isnan(q) == nan).all() and np.isfinite(q[~nan]).all()              # p == T.t: the rows divided by the norm, nothing else
    err = np.where(nan, 0.0, P.diff_to_ref(q, dx["sss_ref_hi"], dx["sss_ref_lo"]))
    for c in range(len(D.SSS_CLASS_NAMES)):                                        # and so within the oracle's floor of the 50-digit restatement
        m = dx["sss_class"] == c
        for k, sl in enumerate(D.SSS_PARTS):
            assert err[m][:, sl].max() <= dx["floor_sss"][c, k]
    assert (prx["sss"][:, 20:] == 0).all()


def test_sincos_is_the_oracle_bit_for_bit(prx, orc):
    x = prx["sincos_x"]
    q = D.unpacked(prx["sincos"], len(x), D.SINCOS_PER_REC, 2)
    o = D.oracle_sincos(orc, x)
    print()
    near = np.abs(x) <= D.SINCOS_NEAR
    ok = _report_same("dsss_sincos |x| <= 4.5 pi", q[near], o[near])
    ok = _report_same("dsss_sincos beyond", q[~near], o[~near]) and ok
    assert ok
    z = x == 0
    assert z.sum() == 3 + 1 and (q[z, 0] == 0).all() and (q[z, 1] == 1).all()


def test_fast_atan2_is_the_oracle_on_every_pair(prx, orc):
    yx = prx["atan2_yx"]
    q = D.unpacked(prx["atan2"], len(yx), D.ATAN2_PER_REC, 1)[:, 0]
    o = D.oracle_atan2(orc, yx).astype(np.float64)
    assert (q == q.astype(np.float32)).all()                                       # floats carried as doubles
    diff = np.flatnonzero(q != o)
    print("\nfast_atan2_dev: %d pairs, %d differ" % (len(yx), len(diff)), yx[diff[:5]], q[diff[:5]], o[diff[:5]])
    assert len(diff) == 0
    assert (q >= 0).all() and (q <= 360).all()


def test_geo_at_is_the_oracle_bit_for_bit(prx, orc):
    rows = prx["geo_rows"]
    print()
    assert _report_same("dsss_geo_at", prx["geo"][:, :2], D.oracle_geo(orc, rows))
    # port columns 0 and 1 share the last bin
    c0, c1 = rows[:, 7] == 0, rows[:, 7] == 1
    assert c0.sum() == c1.sum() > 0


def test_factor_eval_residual_and_jacobian(prx, orc):
    rows = prx["factor_rows"]
    q = prx["factor"]
    w = rows[:, 36:42]
    assert np.log10(w.max() / w.min()) > 11                                        # twelve decades
    print()
    chain = prx["factor_chain"][:, :6]
    assert _report_same("factor_eval r = chain w", q[:, :6], chain * w)
    assert _report_same("factor_eval Ji", q[:, 6:42], D.oracle_factor_jacobian(orc, rows))
    o = P.oracle_edge(orc, rows[:, :36])
    eq = _same(chain, o).all(axis=1)
    print("the device's chain equals the oracle's bit for bit in %d of %d cases" % (eq.sum(), len(eq)))
    assert _same(q[eq, :6], (o * w)[eq]).all()
    hi, lo = P.hilo(prx["fx"], "cmp_ref")
    cls = np.full(len(rows), P.CLASS_ID["composed"])
    assert not _judge("edge chain", chain, hi, lo, cls, P.CLASS_NAMES, prx["fx"]["floor_w"], prx["fx"]["floor_v"], o, 3)


def test_chol6_recip_is_its_restatement_bit_for_bit(prx):
    A, kind = prx["chol_A"], prx["chol_kind"]
    q = prx["chol_recip"]
    L, ri, bad = D.chol6_recip_np(A)
    print()
    ok = _report_same("chol6_recip A'", q[:, :36], L)
    ok = _report_same("chol6_recip ri", q[:, 36:42], ri) and ok
    assert ok
    assert (q[:, 42] == bad).all() and (q[kind >= 2, 42] == 1).all() and (q[kind <= 1, 42] == 0).all()
    up = np.triu_indices(6, 1)
    assert _same(q[:, :36].reshape(-1, 6, 6)[:, up[0], up[1]], A.reshape(-1, 6, 6)[:, up[0], up[1]]).all()      # the upper triangle is not touched


def test_chol6_rdiag_backward_error_and_rsqrt(prx):
    A, kind = prx["chol_A"], prx["chol_kind"]
    q = prx["chol_rdiag"]
    assert (q[kind >= 2, 36] == 1).all() and (q[kind <= 1, 36] == 0).all()
    good = kind <= 1
    L = q[good, :36]
    ratio = D.rdiag_backward_error(A[good], L)
    d = D.rdiag_pivots(A[good], L)
    r = L.reshape(-1, 6, 6)[:, np.arange(6), np.arange(6)]
    ld = np.longdouble
    want = ld(1) / np.sqrt(d.astype(ld))
    ulps = (np.abs(r.astype(ld) - want) / P.ulp(r).astype(ld)).astype(np.float64)
    print("\nchol6_rdiag: %d blocks, largest |A - L L^T| / (gamma_11 |L||L^T|) %.3g; rsqrt: %d pivots, largest error %.3f ulp, %d of them correctly rounded"
          % (good.sum(), ratio.max(), d.size, ulps.max(), (ulps <= 0.5).sum()))
    assert (d > 0).all()
    assert ratio.max() <= 1.0
    assert ulps.max() <= 2.0
    # the substituted pivots: rsqrt(1) = 1 on the diagonal where the pivot was 0, negative, NaN or infinite
    Lb = q[:, :36].reshape(-1, 6, 6)
    one = [Lb[kind == 2][0][2, 2], Lb[kind == 3][0][2, 2], Lb[kind == 4][0][3, 3], Lb[kind == 5][0][4, 4]]
    assert (np.abs(np.array(one) - 1.0) <= 2 * D.EPS).all(), one
    half = [Lb[kind == 2][0][0, 0], Lb[kind == 5][0][5, 5]]                        # exact pivots around them: rsqrt(4)
    assert (np.abs(np.array(half) - 0.5) <= D.EPS).all(), half


# ------------------------------------------------------------------ where the device's libm enters
def test_libm_functions_within_the_floors(prx):
    fx, dx = prx["fx"], prx["dx"]
    Fw, Fv = fx["floor_w"], fx["floor_v"]
    print()
    bad = []
    # the exponentials: the exp cases have references (exp_ref); R 9 entries, t 3
    n_exp = len(fx["exp_xi"])
    hi, lo = P.hilo(fx, "exp_ref")
    ecls = fx["exp_class"].astype(int)
    _, q, o = _rows(prx, P.F_POSE_EXP)
    bad += _judge("pose_exp", q[:n_exp, :12], hi, lo, ecls, P.CLASS_NAMES, Fw, Fv, o[:n_exp, :12], 9)
    _, q, o = _rows(prx, P.F_SO3_EXP)
    bad += _judge("so3_exp", q[:n_exp, :9], hi[:, :9], lo[:, :9], ecls, P.CLASS_NAMES, Fw, Fv, o[:n_exp, :9], 9)
    _, q, o = _rows(prx, P.F_RODRIGUES)
    bad += _judge("rodrigues", q[:n_exp, :9], hi[:, :9], lo[:, :9], ecls, P.CLASS_NAMES, Fw, Fv, o[:n_exp, :9], 9)
    for fid in (P.F_SO3_EXP, P.F_POSE_EXP, P.F_RODRIGUES):                         # the other tangents have no reference of their own: the share only
        _, q, o = _rows(prx, fid)
        print("%s on the interior classes' tangents: bit-equal to the oracle %d of %d" % (D.NAMES[fid], _same(q[n_exp:], o[n_exp:]).all(axis=1).sum(), len(q) - n_exp))
        assert np.isfinite(q).all()
    # the logarithms
    hi, lo = P.hilo(fx, "log_ref")
    lcls = fx["log_class"].astype(int)
    _, q, o = _rows(prx, P.F_POSE_LOG)
    bad += _judge("pose_log", q[:, :6], hi, lo, lcls, P.CLASS_NAMES, Fw, Fv, o[:, :6], 3)
    _, q, o = _rows(prx, P.F_SO3_LOG)
    bad += _judge("so3_log", q[:, :3], hi[:, :3], lo[:, :3], lcls, P.CLASS_NAMES, Fw, Fv, o[:, :3], 3)
    # the edge chain at kilometre coordinates
    hi, lo = P.hilo(fx, "cmp_ref")
    _, q, o = _rows(prx, P.F_EDGE)
    bad += _judge("edge chain", q[:, :6], hi, lo, np.full(len(q), P.CLASS_ID["composed"]), P.CLASS_NAMES, Fw, Fv, o[:, :6], 3)
    # retract: the interior log classes, by the class of the tangent
    ti, xi = D.retract_index(fx)
    _, q, o = _rows(prx, P.F_RETRACT)
    hi, lo = P.hilo(dx, "retract_ref")
    tcls = fx["exp_class"][xi].astype(int) - P.CLASS_ID[D.RETRACT_CLASS_NAMES[0]]
    bad += _judge("retract", q[ti, :12], hi, lo, tcls, D.RETRACT_CLASS_NAMES, dx["floor_retract_w"], dx["floor_retract_v"], o[ti, :12], 9)
    assert np.isfinite(q).all()
    assert not bad, bad


def test_rpy_on_every_rotation_and_at_gimbal_lock(prx, orc):
    fx, dx = prx["fx"], prx["dx"]
    _, q, o = _rows(prx, P.F_RPY)
    g = dx["gimbal_T"]
    qa = np.concatenate([q[:, :3], prx["gimbal"][:, :3]])
    oa = np.concatenate([o[:, :3], D.oracle_rpy(orc, g)])
    cls = np.concatenate([fx["log_class"].astype(int), np.full(len(g), D.RPY_GIMBAL)])
    hi, lo = P.hilo(dx, "rpy_ref")
    print()
    bad = _judge("rpy", qa, hi, lo, cls, D.RPY_CLASS_NAMES, dx["floor_rpy"], dx["floor_rpy"], oa, 3)
    d = np.abs(qa - oa) / P.ulp(oa)
    print("rpy: the device's atan2 differs from glibc's in %d of %d angles, by %.3g ulp at most" % ((qa != oa).sum(), qa.size, np.nan_to_num(d).max()))
    assert not bad, bad
    # at gimbal lock: finite, and roll and yaw within the bar of the reference's atan2 of the same signed zeros, angle by angle
    qg, n = prx["gimbal"][:, :3], len(fx["log_T"])
    assert np.isfinite(qg).all()
    err = P.diff_to_ref(qg, hi[n:], lo[n:])
    bar = 8 * dx["floor_rpy"][D.RPY_GIMBAL] + 4 * P.ulp(hi[n:])
    assert (err[:, [0, 2]] <= bar[:, [0, 2]]).all()
    zeros = (g[:, 7] == 0) & (g[:, 8] == 0)
    assert set(np.round(np.abs(hi[n:][zeros][:, [0, 2]]).ravel(), 6)) == {0.0, round(np.pi, 6)}       # atan2(+-0, +-0): 0 or pi
    assert (np.signbit(qg[zeros][:, [0, 2]]) == np.signbit(g[zeros][:, [7, 3]])).all()                 # the sign is the first argument's
    assert (np.abs(np.abs(qg[:, 1]) - np.pi / 2) <= 3e-8).all()


# ------------------------------------------------------------------ the collectives
def test_scans_are_cumsum_and_keep_their_f64_order(prx):
    for (code, v), s in zip(prx["vecs"], prx["scan"]):
        if code == 2: continue
        cs = np.cumsum(v, dtype=v.dtype)
        assert (s["prefix"] == cs - v).all() and s["total"] == cs[-1], (code, len(v))
        x = D.pad256(v)
        w = x.reshape(-1, 64)
        assert (s["incl"].reshape(-1, 64) == np.cumsum(w, axis=1, dtype=v.dtype)).all(), (code, len(v))
        assert (s["wsum"] == w.sum(axis=1, dtype=v.dtype)).all(), (code, len(v))
    # f64: the scans in the device's order of additions
    for (code, v), s in zip(prx["vecs"], prx["scan"]):
        if code != 2: continue
        pre, tot = D.carried_scan_np(v)
        assert _same(s["prefix"], pre).all() and _same(s["total"], tot).all(), len(v)
        assert _same(s["incl"], D.wave_scan_np(v)).all(), len(v)


def test_f64_wave_and_block_sums_keep_their_order(prx):
    n = 0
    for (code, v), s in zip(prx["vecs"], prx["scan"]):
        if code != 2: continue
        assert _same(s["wsum"], D.wave_sum_np(v)).all(), len(v)
        assert _same(s["bsum"], D.block_sum_np(v)).all(), len(v)
        n += len(s["wsum"])
    assert n > 200


# ------------------------------------------------------------------ the LM rule
def test_lm_table_on_the_device(prx):
    q = prx["lm"].reshape(D.LM_KINDS, D.LM_ROWS_ASKED, D.OUT_W)
    print()
    for kind, (name, least) in enumerate((("verdict", 16), ("lambda", 5), ("continue", 12))):
        rows = int(q[kind, 0, 0])
        assert (q[kind, :, 0] == rows).all() and least <= rows < D.LM_ROWS_ASKED, name
        assert (q[kind, :rows, 1] == 1).all() and (q[kind, rows:, 1:] == 0).all(), name
        got, want = q[kind, :rows, 2:5], q[kind, :rows, 5:8]
        if kind == 1:
            stated = want[:, 2] >= 0
            assert stated.sum() >= 4
            got = np.where(stated[:, None] | (np.arange(3) < 2), got, 0); want = np.where(stated[:, None] | (np.arange(3) < 2), want, 0)
        wrong = np.flatnonzero((got != want).any(axis=1))
        print("LM %-9s %2d rows, %d wrong %s" % (name, rows, len(wrong), wrong))
        assert len(wrong) == 0, (name, wrong, got[wrong], want[wrong])
        assert (want[:, :2] == 1).any() and (want[:, :2] == 0).any()

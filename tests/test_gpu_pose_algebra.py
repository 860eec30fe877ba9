"""GPU: the device's SO(3)/SE(3) algebra (diasss_amd/csrc/dsss_pose.h as the kernels compile it) against the 50-digit reference of
tests/pose_algebra_ref.py, at every branch of the logarithm, through the Between factor's chain at kilometre coordinates, and -- as far as
a value leaves the device -- of the exponential.  Reads tests/golden/pose_algebra.npz and the library; the classes are described in
tests/test_pose_algebra_cpu.py, which also holds the oracle to the same reference and the host build of the header to the oracle.

The probe is dsss_posegraph_edge_report: r6[e] = Log(rel^-1 Xa^-1 Xb) / sqrt(var) as factor_eval computes it, at poses the caller supplies.
With Xa = rel = identity and var = 1 both pose_between calls multiply by 1 and add 0, so r6[e] is the device's pose_log on exactly the
fixture's doubles.

Pass rule for a device value q, the reference r and the class's floor F (max |oracle - r| over the class, stored in the fixture):
    |q - r| <= 8 F + 4 ulp(r), rotation and translation parts apart (ulp of the part's largest component).
The yardstick is the oracle's own rounding error, never the device's numbers.  The device runs the same operations unfused and can differ
from the oracle only in sin, acos, tan (and sqrt, were it not correctly rounded); each enters through the condition number that makes F, so 8
admits a library function a few ulps worse than glibc's and still fails a wrong term by orders of magnitude.  The Taylor branch's omega uses
+ - * / alone and must equal the oracle bit for bit.

The exponential leaves the device only as ONE SCALAR: with two poses, dr6 = [0, xi], both supplied poses the identity and no closures,
sums3[0] = 0.5 sum_a (odo_a Log(Pose3(Rodrigues(xi[:3]), xi[3:])^-1)_a)^2 -- a functional of pg_init_kernel's so3_exp and the logarithm, not
the full map.  This module keeps the view through the library's own entry.  The functions that leave through no entry -- pose_exp's
translation, pose_adjoint, pose_rpy, pose_retract, and with them the device's atan2 -- are evaluated on the device one at a time by the
stand-alone probe diasss_amd/host/dev_probe.hip and held to the same references and the same rule in tests/test_gpu_dev_probe.py."""
import numpy as np
import pytest

from tests import pose_algebra_ref as P

pytestmark = pytest.mark.gpu

IDENT = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64)


@pytest.fixture(scope="module")
def ctx():
    from diasss_amd import capi
    c = capi.Context(max_frames=2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fx():
    return P.load()


def _edges(a, b, rel, var):
    from diasss_amd import capi
    e = np.zeros(len(b), capi.LCEDGE_DTYPE)
    e["a"], e["b"], e["rel"], e["var"] = a, b, rel, var
    return e


def _part_ulp(r):
    return P.ulp(np.abs(r).max(axis=1))


def _judge(what, q, hi, lo, cls, Fw, Fv, oracle):
    """the pass rule on xi-like rows (3 rotation + 3 translation components); prints per class max |q - r| / F and the bit-equal share"""
    err = P.diff_to_ref(q, hi, lo)
    bad = []
    for c in np.unique(cls):
        m = cls == c
        ew, ev = err[m, :3].max(axis=1), err[m, 3:].max(axis=1)
        tw, tv = 8 * Fw[c] + 4 * _part_ulp(hi[m, :3]), 8 * Fv[c] + 4 * _part_ulp(hi[m, 3:])
        eq = (q[m] == oracle[m]).all(axis=1).sum()
        with np.errstate(divide="ignore", invalid="ignore"):
            rw, rv = np.nan_to_num(ew.max() / Fw[c], nan=0.0), np.nan_to_num(ev.max() / Fv[c], nan=0.0)
        print("%s %-22s max|q-r|/F rot %9.3g trans %9.3g   (F %9.3g %9.3g)   bit-equal to the oracle %3d of %3d"
              % (what, P.CLASS_NAMES[c], rw, rv, Fw[c], Fv[c], eq, m.sum()))
        if not ((ew <= tw).all() and (ev <= tv).all()): bad.append(P.CLASS_NAMES[c])
    assert not bad, bad


def test_device_logarithm_at_every_branch(ctx, orc, fx):
    T, cls = fx["log_T"], fx["log_class"].astype(int)
    n = len(T)
    poses = np.concatenate([IDENT[None], T])
    dr = np.zeros((n + 1, 6))
    ident = np.tile(IDENT, (n, 1))
    chi2, r6, sums = ctx.posegraph_edge_report(dr, _edges(0, 1 + np.arange(n), ident, 1.0), poses)
    assert np.isfinite(r6).all()
    hi, lo = P.hilo(fx, "log_ref")
    o = P.oracle_log(orc, T)
    print()
    _judge("log", r6, hi, lo, cls, fx["floor_w"], fx["floor_v"], o)
    taylor = fx["log_branch"] == P.BR_TAYLOR
    assert taylor.sum() > 100
    assert (r6[taylor, :3] == o[taylor, :3]).all()                               # + - * / only: a difference is a contraction or a reordering
    # whitening over twelve decades of variance: r = xi * (1 / sqrt(var)), one rounding each, and chi2 summed in index order
    var = 10.0 ** np.random.default_rng(7).uniform(-6, 6, (n, 6))
    chi2v, r6v, _ = ctx.posegraph_edge_report(dr, _edges(0, 1 + np.arange(n), ident, var), poses)
    assert (r6v == r6 * (1.0 / np.sqrt(var))).all()
    for c, r in ((chi2, r6), (chi2v, r6v)):
        assert (c == (((((r[:, 0] ** 2 + r[:, 1] ** 2) + r[:, 2] ** 2) + r[:, 3] ** 2) + r[:, 4] ** 2) + r[:, 5] ** 2)).all()


def test_device_between_chain_at_kilometre_coordinates(ctx, orc, fx):
    cin = fx["cmp_in"]
    n = len(cin)
    poses = cin[:, :24].reshape(2 * n, 12)
    chi2, r6, sums = ctx.posegraph_edge_report(np.zeros((2 * n, 6)), _edges(2 * np.arange(n), 2 * np.arange(n) + 1, cin[:, 24:], 1.0), poses)
    hi, lo = P.hilo(fx, "cmp_ref")
    print()
    _judge("between", r6, hi, lo, np.full(n, P.CLASS_ID["composed"]), fx["floor_w"], fx["floor_v"], P.oracle_edge(orc, cin))


def test_device_exponential_through_its_scalar(ctx, orc, fx):
    xi, cls = fx["probe_xi"], fx["probe_class"].astype(int)
    hi, lo = P.hilo(fx, "probe_ref")
    F = fx["floor_probe"]
    none = _edges(np.zeros(0, int), np.zeros(0, int), np.zeros((0, 12)), np.zeros((0, 6)))
    two = np.tile(IDENT, (2, 1))
    q = np.array([ctx.posegraph_edge_report(np.stack([np.zeros(6), x]), none, two)[2][0] for x in xi])
    assert np.isfinite(q).all()
    o = P.oracle_probe(orc, xi)
    err = P.diff_to_ref(q, hi, lo)
    bad = []
    print()
    for c in np.unique(cls):
        m = cls == c
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.nan_to_num(err[m].max() / F[c], nan=0.0)
        print("exp %-22s max|q-r|/F %9.3g   (F %9.3g, largest value %9.3g)   bit-equal to the oracle %3d of %3d"
              % (P.CLASS_NAMES[c], ratio, F[c], hi[m].max(), (q[m] == o[m]).sum(), m.sum()))
        if not (err[m] <= 8 * F[c] + 4 * P.ulp(hi[m])).all(): bad.append(P.CLASS_NAMES[c])
    assert not bad, bad

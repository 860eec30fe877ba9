"""The dense loop closures with a yaw fan off the device: the numpy reference of tests/register_yaw_ref.py by hand, the host arithmetic of
libdsss.so (dsss_register_rotate_rows, dsss_register_yaw_peak, dsss_register_edge_yaw) against that reference, and the preconditions of
the GPU tests on the reference alone (tests/test_gpu_register_yaw.py): on a survey whose leg 1 has every segment turned by a whole
number of steps and moved by whole cells, the fan finds that angle and that shift in every segment, away from its borders, with
unambiguous anchor pings, and its edges pull the heading of leg 1 back under the oracle's pose-graph solve."""
import numpy as np
import pytest

from tests import mosaic_register_ref as R
from tests import register_edges_ref as E
from tests import register_yaw_ref as Y
from tests.pg_report_ref import residual_bound

E_ARG = -2
N, M = 640, 400
RADIUS, MIN_CELLS = 8, 256
CELL, SEG, SHIFT, FANS = Y.CELL, Y.SEG, Y.SHIFT, Y.FANS


# ---------------------------------------------------------------- the reference itself
def test_reference_rotation_by_hand(orc):
    rows = np.zeros((5, 6)); rows[:, 3] = np.arange(5.0); rows[:, 4] = 1.0; rows[:, 2] = 0.25; rows[:, 0] = 0.5; rows[:, 5] = -3.0
    assert Y.thetas(5, 0.25) == [-0.5, -0.25, 0.0, 0.25, 0.5] and Y.thetas(1, 0.3) == [0.0]
    q = Y.rotate_rows(orc, rows, 1, 5, np.pi / 2)                   # pivot: ping 3 at (3, 1); a quarter turn takes (dx, 0) to (0, dx)
    assert np.allclose(q[:, 3], 3.0, atol=1e-15) and np.allclose(q[:, 4], [-1.0, 0.0, 1.0, 2.0], atol=1e-15)
    assert (q[:, 2] == 0.25 + np.pi / 2).all() and (q[:, [0, 1, 5]] == rows[1:5][:, [0, 1, 5]]).all()
    assert q[2].tolist()[3:5] == [3.0, 1.0]                         # the pivot stays where it is, exactly
    # theta == 0 copies: coordinates for which cx + (x - cx) != x keep their bits
    odd = rows.copy(); odd[:, 3] = [0.1, 0.2, 1e9 + 0.3, 0.7, 1e-9]
    assert odd[2, 3] + (odd[0, 3] - odd[2, 3]) != odd[0, 3]
    assert Y.rotate_rows(orc, odd, 0, 5, 0.0).tobytes() == odd.tobytes() and Y.rotate_rows(orc, odd, 0, 5, -0.0).tobytes() == odd.tobytes()
    s, c = Y.sincos(orc, 0.3)
    assert abs(s - np.sin(0.3)) < 1e-15 and abs(c - np.cos(0.3)) < 1e-15


def _rows(n, seed, x0, y0, yaw):
    rng = np.random.default_rng(seed)
    s = 0.05 * (np.arange(n) + 0.5)
    rows = np.zeros((n, 6))
    rows[:, 0] = 0.02 * rng.standard_normal(n); rows[:, 1] = 0.02 * rng.standard_normal(n); rows[:, 2] = yaw + 0.01 * np.sin(s)
    rows[:, 3] = x0 + s * np.cos(yaw); rows[:, 4] = y0 + s * np.sin(yaw) + 0.3 * np.sin(s / 3.0); rows[:, 5] = 0.1 * rng.standard_normal(n)
    return rows


# ---------------------------------------------------------------- the library's host arithmetic
@pytest.mark.parametrize("theta", [0.0, -0.0, 0.01, -0.035, 1.0, -2.5, 7.0e-9])
def test_rotate_rows_bit_for_bit(orc, theta):
    from diasss_amd import capi
    rows = _rows(200, 4, 1234.5, -987.25, 2.1)
    for p0, p1 in ((0, 200), (37, 38), (40, 121), (199, 200)):
        dev = capi.register_rotate_rows(rows, p0, p1, theta)
        assert dev.tobytes() == Y.rotate_rows(orc, rows, p0, p1, theta).tobytes(), "theta %r, pings %d..%d" % (theta, p0, p1)
    if theta == 0.0:
        assert capi.register_rotate_rows(rows, 40, 121, theta).tobytes() == rows[40:121].tobytes()


def test_rotate_rows_argument_errors():
    from diasss_amd import capi
    rows = _rows(50, 5, 0.0, 0.0, 0.0)
    for args in ((None, 0, 10, 0.1), (rows, -1, 10, 0.1), (rows, 10, 10, 0.1), (rows, 11, 10, 0.1), (rows, 0, 51, 0.1), (rows, 0, 10, np.nan),
                 (rows, 0, 10, np.inf)):
        with pytest.raises(capi.DsssError) as ei:
            capi.register_rotate_rows(*args)
        assert ei.value.code == E_ARG
    L = capi.lib()
    assert L.dsss_register_rotate_rows(capi._ptr(rows), 50, 0, 10, 0.1, None) == E_ARG


def _recs(znccs):
    from diasss_amd import capi
    a = np.zeros(len(znccs), capi.REG_DTYPE)
    a["zncc"] = znccs
    return a


YAW_PEAK_CASES = {
    "single_angle": [0.7],
    "single_angle_unusable": [-2.0],
    "middle": [0.2, 0.5, 0.9, 0.6, 0.1],
    "skewed_parabola": [0.2, 0.5, 0.9, 0.8, 0.1],
    "first_angle": [0.9, 0.5, 0.3],
    "last_angle": [0.1, 0.5, 0.9],
    "tie_goes_to_the_middle": [0.9, 0.2, 0.9, 0.2, 0.9],
    "tie_at_one_distance_goes_down": [0.1, 0.9, 0.3, 0.9, 0.1],
    "tie_on_both_borders": [0.9, 0.2, 0.9],
    "all_equal": [0.5] * 7,
    "left_neighbour_unusable": [0.1, -2.0, 0.9, 0.6, 0.1],
    "right_neighbour_unusable": [0.1, 0.5, 0.9, -2.0, 0.1],
    "flat_top_has_no_parabola": [0.1, 0.9, 0.9, 0.9, 0.1],
    "valley": [0.1, 0.95, 0.9, 1.0, 0.1],                     # at the peak k = 3 the neighbours are 0.9 and 0.1: den < 0 still
    "none_usable": [-2.0] * 5,
    "only_a_border_usable": [-2.0, -2.0, 0.4],
    "seventeen": [0.01 * k for k in range(9)] + [0.085] + [0.01 * (7 - k) for k in range(7)],
}


@pytest.mark.parametrize("name", sorted(YAW_PEAK_CASES))
def test_yaw_peak_against_the_rule(name):
    from diasss_amd import capi
    z = YAW_PEAK_CASES[name]
    for step in (0.01, 0.37):
        ref = Y.yaw_peak(z, len(z), step)
        dev = capi.register_yaw_peak(_recs(z), step)
        assert dev[:2] == ref[:2] and np.float64(dev[2]).tobytes() == np.float64(ref[2]).tobytes() and np.float64(dev[3]).tobytes() == np.float64(ref[3]).tobytes(), (dev, ref)
    k, border, theta, hat = Y.yaw_peak(z, len(z), 0.01)
    expect = {"single_angle": (0, 0), "single_angle_unusable": (0, 0), "middle": (2, 0), "first_angle": (0, 1), "last_angle": (2, 1),
              "tie_goes_to_the_middle": (2, 0), "tie_at_one_distance_goes_down": (1, 0), "tie_on_both_borders": (0, 1), "all_equal": (3, 0),
              "none_usable": (2, 0), "only_a_border_usable": (2, 1), "left_neighbour_unusable": (2, 0), "seventeen": (9, 0)}
    if name in expect:
        assert (k, border) == expect[name]
    if name in ("first_angle", "last_angle", "left_neighbour_unusable", "right_neighbour_unusable", "flat_top_has_no_parabola", "none_usable", "single_angle", "all_equal"):
        assert hat == theta
    if name == "skewed_parabola":
        assert theta == 0.0 and 0.0 < hat < 0.005                   # towards the better neighbour, less than half a step
    if name == "middle":
        assert theta == 0.0 and hat == 0.5 * (0.5 - 0.6) / (0.5 - 2.0 * 0.9 + 0.6) * 0.01 + 0.0


def test_yaw_peak_random_tables():
    from diasss_amd import capi
    rng = np.random.default_rng(11)
    for _ in range(300):
        nyaw = int(rng.choice([1, 3, 5, 9, 17]))
        z = np.round(rng.uniform(-1, 1, nyaw), 1)                   # one decimal: ties happen
        z[rng.uniform(size=nyaw) < 0.25] = -2.0
        ref = Y.yaw_peak(z.tolist(), nyaw, 0.02)
        dev = capi.register_yaw_peak(_recs(z), 0.02)
        assert dev[:2] == ref[:2] and dev[2] == ref[2] and np.float64(dev[3]).tobytes() == np.float64(ref[3]).tobytes(), (z, dev, ref)


def test_yaw_peak_argument_errors():
    from diasss_amd import capi
    for z, step in (([0.1, 0.2], 0.01), ([0.1] * 19, 0.01), ([0.1] * 4, 0.01), ([0.1] * 3, 0.0), ([0.1] * 3, -0.01), ([0.1] * 3, np.nan), ([0.1] * 3, np.inf)):
        with pytest.raises(capi.DsssError) as ei:
            capi.register_yaw_peak(_recs(z), step)
        assert ei.value.code == E_ARG
    with pytest.raises(capi.DsssError):
        capi.register_yaw_peak(_recs([]), 0.01)
    y = capi.reg_yaw_params_default(); e = capi.reg_edge_yaw_params_default()
    assert (y.nyaw, y.step) == (1, Y.STEP) and (e.fan.nyaw, e.fan.step, e.sigma_yaw_steps) == (1, Y.STEP, Y.SIGMA_YAW_STEPS)
    assert (e.e.min_zncc, e.e.sigma_xy_cells, e.e.sigma_z, e.e.sigma_rot) == (E.MIN_ZNCC, E.SIGMA_XY_CELLS, E.SIGMA_Z, E.SIGMA_ROT)


# ---------------------------------------------------------------- dsss_register_edge_yaw on constructed rows
def _grid(cell=CELL):
    from diasss_amd import capi
    return capi.MosaicParams(-3.0, -2.0, cell, 400, 300, 0, 0)


def _row(p0, p1, k=3, nyaw=5, step=0.01, hat=0.0123, border=0, zncc=0.9, on_border=0, n=1000, sx=100000, sy=120000, off=(0.23, -0.11)):
    r = dict(dx=2, dy=-1, off_x=off[0], off_y=off[1], zncc=zncc, zncc0=0.2, n=n, n0=n, on_border=on_border)
    return dict(pair=0, seg=0, p0=p0, p1=p1, sx=sx, sy=sy, r=r, k=k, yaw_on_border=border, theta=float(k - (nyaw - 1) // 2) * step, theta_hat=hat, zncc_k0=0.5)


def _seg(row):
    from diasss_amd import capi
    s = np.zeros(1, capi.REGSEGYAW_DTYPE)
    for k in ("pair", "seg", "p0", "p1", "sx", "sy"):
        s["s"][k] = row[k]
    for k, v in row["r"].items():
        s["s"]["r"][k] = v
    for k in ("k", "yaw_on_border", "theta", "theta_hat", "zncc_k0"):
        s[k] = row[k]
    return s[0]


def _params(nyaw, step, sigma_yaw_steps=1.0, e=(0.5, 1.0, 10.0, 1.0)):
    from diasss_amd import capi
    return capi.RegEdgeYawParams(capi.RegEdgeParams(*e), capi.RegYawParams(nyaw, 0, step), sigma_yaw_steps)


def _same_edge(dev, ref, exact=False):
    assert int(dev["a"]) == ref["a"] and int(dev["b"]) == ref["b"]
    assert np.asarray(dev["var"]).tobytes() == np.asarray(ref["var"], np.float64).tobytes(), "var: %s, reference %s" % (dev["var"], ref["var"])
    d, r = np.asarray(dev["rel"]), ref["rel"]
    assert (np.abs(d - r) <= residual_bound(r, 1.0)).all(), "rel: %s, reference %s" % (d, r)


EDGE_CASES = {
    "forward": dict(row=_row(40, 120), base_a=0, base_b=200),
    "reversed": dict(row=_row(40, 120, k=1, hat=-0.0087), base_a=900, base_b=100),
    "middle_angle": dict(row=_row(40, 120, k=2, hat=0.0004), base_a=0, base_b=200),
    "on_the_border_of_the_fan": dict(row=_row(40, 120, k=4, hat=0.02, border=1), base_a=0, base_b=200),
    "on_the_border_of_the_square": dict(row=_row(40, 120, on_border=1), base_a=0, base_b=200),
    "below_the_threshold": dict(row=_row(40, 120, zncc=0.4999), base_a=0, base_b=200),
    "no_usable_angle": dict(row=_row(0, 200, k=2, hat=0.0, zncc=-2.0, n=17, sx=0, sy=0, off=(0.0, 0.0)), base_a=0, base_b=200),
    "one_ping": dict(row=_row(77, 78), base_a=0, base_b=200),
    "a_wide_turn": dict(row=_row(10, 190, k=7, nyaw=9, step=0.05, hat=0.21), base_a=0, base_b=200),     # the anchor ping moves with theta
}


@pytest.mark.parametrize("name", sorted(EDGE_CASES))
def test_register_edge_yaw_against_the_reference(orc, name):
    from diasss_amd import capi
    cs = EDGE_CASES[name]
    nyaw, step = (9, 0.05) if name == "a_wide_turn" else (5, 0.01)
    p = _grid()
    rows_a = _rows(200, 1, 2.0, 9.0, 0.02); rows_b = _rows(200, 2, 11.5, 14.0, np.pi - 0.03)
    ref = Y.edge_yaw(orc, cs["row"], p, rows_a, cs["base_a"], rows_b, cs["base_b"], nyaw, step, sigma_yaw_steps=1.5)
    dev = capi.register_edge_yaw(_seg(cs["row"]), p, rows_a, cs["base_a"], rows_b, cs["base_b"], _params(nyaw, step, 1.5))
    assert (dev is None) == (ref is None)
    assert (ref is None) == (name in ("on_the_border_of_the_fan", "on_the_border_of_the_square", "below_the_threshold", "no_usable_angle"))
    if ref is None:
        return
    assert ref["lead"] > 1e-6, "the constructed case has an ambiguous anchor ping (lead %g)" % ref["lead"]
    assert cs["row"]["p0"] <= ref["j"] < cs["row"]["p1"]
    _same_edge(dev, ref)
    assert ref["var"][2] == (1.5 * step) ** 2 and ref["var"][0] == ref["var"][1] == 1.0
    # the heading of the measurement is the row's own turned by theta_hat: against the edge of the unrotated row it differs by that angle
    flat = dict(cs["row"], theta=0.0, theta_hat=0.0)
    plain = Y.edge_yaw(orc, flat, p, rows_a, cs["base_a"], rows_b, cs["base_b"], nyaw, step)
    if plain["j"] == ref["j"]:
        turn = np.arctan2(ref["rel"][3], ref["rel"][0]) - np.arctan2(plain["rel"][3], plain["rel"][0])
        turn = (turn + np.pi) % (2 * np.pi) - np.pi
        want = cs["row"]["theta_hat"] * (-1.0 if name == "reversed" else 1.0)
        assert abs(turn - want) < 2e-3, (turn, want)               # (not exact: roll and pitch of the two pings tilt the axis a little)
    if name == "a_wide_turn":
        assert plain["j"] != ref["j"]


def test_one_angle_is_the_existing_edge_bit_for_bit(orc):
    from diasss_amd import capi
    p = _grid()
    rows_a = _rows(200, 1, 2.0, 9.0, 0.02); rows_b = _rows(200, 2, 11.5, 14.0, np.pi - 0.03)
    for base_a, base_b in ((0, 200), (900, 100)):
        row = _row(40, 120, k=0, nyaw=1, hat=0.0)
        assert row["theta"] == 0.0
        old = capi.register_edge(_seg(row)["s"], p, rows_a, base_a, rows_b, base_b, capi.RegEdgeParams(0.5, 2.0, 3.0, 0.25))
        new = capi.register_edge_yaw(_seg(row), p, rows_a, base_a, rows_b, base_b, _params(1, 0.01, 7.0, e=(0.5, 2.0, 3.0, 0.25)))
        assert old is not None and new.tobytes() == old.tobytes()
        assert capi.register_edge_yaw(_seg(row), p, rows_a, base_a, rows_b, base_b).tobytes() == capi.register_edge(_seg(row)["s"], p, rows_a, base_a, rows_b, base_b).tobytes()
        ref_old = E.edge(orc, row, p, rows_a, base_a, rows_b, base_b)
        ref_new = Y.edge_yaw(orc, row, p, rows_a, base_a, rows_b, base_b, 1, 0.01)
        assert ref_new["rel"].tobytes() == ref_old["rel"].tobytes() and ref_new["var"].tobytes() == ref_old["var"].tobytes() and (ref_new["a"], ref_new["b"]) == (ref_old["a"], ref_old["b"])


def test_register_edge_yaw_argument_errors():
    from diasss_amd import capi
    p = _grid()
    rows = _rows(100, 3, 0.0, 0.0, 0.0)
    good = _row(10, 60)
    assert capi.register_edge_yaw(_seg(good), p, rows, 0, rows, 100, _params(5, 0.01)) is not None

    def code(seg=good, grid=p, ra=rows, rb=rows, ep=_params(5, 0.01)):
        with pytest.raises(capi.DsssError) as ei:
            capi.register_edge_yaw(None if seg is None else _seg(seg), grid, ra, 0, rb, 100, ep)
        return ei.value.code

    assert code(seg=None) == E_ARG and code(grid=None) == E_ARG and code(ra=None) == E_ARG and code(rb=None) == E_ARG
    for nyaw, step in ((0, 0.01), (2, 0.01), (19, 0.01), (-3, 0.01), (5, 0.0), (5, -0.01), (5, np.nan), (5, np.inf)):
        assert code(ep=_params(nyaw, step)) == E_ARG
    for bad in (0.0, -1.0, np.inf, np.nan):
        assert code(ep=_params(5, 0.01, bad)) == E_ARG
        for k in range(1, 4):
            v = [0.5, 1.0, 10.0, 1.0]; v[k] = bad
            assert code(ep=_params(5, 0.01, e=v)) == E_ARG
    assert code(seg=dict(good, theta=np.nan)) == E_ARG and code(seg=dict(good, theta_hat=np.inf)) == E_ARG
    assert code(seg=_row(60, 60)) == E_ARG and code(seg=_row(10, 101)) == E_ARG and code(seg=_row(10, 60, n=0)) == E_ARG
    assert code(seg=_row(10, 60, zncc=0.1), ep=_params(5, 0.01, 0.0)) == E_ARG        # the parameters are checked before the row is judged
    L = capi.lib()
    s = capi.RegSegYaw.from_buffer_copy(_seg(good).tobytes()); ep = _params(5, 0.01)
    import ctypes as C
    assert L.dsss_register_edge_yaw(C.byref(s), C.byref(p), capi._ptr(rows), 100, 0, capi._ptr(rows), 100, 100, C.byref(ep), None) == E_ARG      # no edge


# ---------------------------------------------------------------- preconditions of the GPU tests, on the reference alone
@pytest.fixture(scope="module")
def legs(orc):
    """the two legs of synth.Survey(2, 640, 400, seed=7) under their true poses"""
    from diasss_amd.synth import Survey
    sv = Survey(2, N, M, seed=7)
    fr = []
    for f in range(2):
        raw = sv.frame(f).numpy().copy()
        pose, alt, gr = sv.inputs(f)
        fr.append(dict(gr=gr, norm=orc.normalize(raw), mask=orc.mask(raw), true=np.ascontiguousarray(sv.poses_true[f])))
    return fr


def _survey(orc, fr, nyaw, step, m):
    from diasss_amd import capi
    rows = [fr[0]["true"], Y.rotated_survey(orc, fr[1]["true"], SEG, m, step, SHIFT, CELL)]
    g = [orc.geo_img(np.ascontiguousarray(r), L["gr"], M) for r, L in zip(rows, fr)]
    gx = np.concatenate([a[0].ravel() for a in g]); gy = np.concatenate([a[1].ravel() for a in g])
    p = capi.mosaic_grid((gx.min(), gx.max(), gy.min(), gy.max()), CELL); p.use_mask = 0
    la = R.mean_layer(g[0][0], g[0][1], fr[0]["norm"], fr[0]["mask"], p, 0)
    return rows, p, la, g[1]


def _wrap(a):
    return (a + np.pi) % (2 * np.pi) - np.pi


@pytest.mark.parametrize("name", sorted(FANS))
def test_preconditions_of_the_gpu_tests(orc, legs, name):
    """Seen with this reference on the CPU, fan one_step_up (5 angles 0.01 rad apart, segments turned by -0.01): 8 segments, every one
    with k - mid = 1 and the peak at (2, -1); ZNCC 0.969 to 0.990 against 0.903 to 0.932 without rotation; theta_hat 0.0097 to 0.0108;
    anchor leads 2.4e-4 and more.  Mean |yaw - true| of leg 1 after the oracle's solve: 0.01000 with the translation-only edges (they
    leave the heading alone), 0.00987 with the fan's edges at the default sigma of one step (the odometry's yaw sigma is 1.7e-5 rad per
    ping, so eight edges of sigma 0.01 move little), 0.00170 at a sigma of 0.05 steps."""
    nyaw, step, m = FANS[name]
    mid = (nyaw - 1) // 2
    rows, p, la, gb = _survey(orc, legs, nyaw, step, m)
    fan = Y.register_segments_yaw(orc, la, rows[1], legs[1]["gr"], M, legs[1]["norm"], legs[1]["mask"], p, SEG, RADIUS, MIN_CELLS, nyaw, step)
    assert len(fan) == 8
    usable = [s for s in fan if s["r"]["zncc"] > -2.0]
    print("k %s, peaks %s" % ([s["k"] for s in fan], [(s["r"]["dx"], s["r"]["dy"]) for s in fan]))
    print("zncc %s, unrotated %s" % (" ".join("%.3f" % s["r"]["zncc"] for s in fan), " ".join("%.3f" % s["zncc_k0"] for s in fan)))
    print("theta_hat %s" % " ".join("%.5f" % s["theta_hat"] for s in fan))
    assert len(usable) == 8
    assert all(s["k"] - mid == m and (s["r"]["dx"], s["r"]["dy"]) == SHIFT for s in usable)              # 1. the angle and the shift, exactly
    assert all(s["r"]["zncc"] > s["zncc_k0"] > -2.0 for s in usable)                                      # 2. better than without rotation
    es, src = Y.edges_yaw(orc, fan, p, rows[0], 0, rows[1], N, nyaw, step)
    assert src == list(range(8))
    assert all(fan[k]["yaw_on_border"] == 0 and fan[k]["r"]["on_border"] == 0 for k in src)               # 3. no accepted row on a border
    assert all(abs(s["theta_hat"] - m * step) < 0.5 * step for s in usable)
    leads = [e["lead"] for e in es]
    print("anchor leads %s" % " ".join("%.3g" % v for v in leads))
    knife = [e for e in es if not e["lead"] > 1e-6]
    assert len(knife) < 0.1 * len(fan) and len(knife) == 0
    assert all(0 <= e["a"] < N <= e["b"] < 2 * N for e in es)
    # one angle: the existing reference, sums and records and centroids
    one = Y.register_segments_yaw(orc, la, rows[1], legs[1]["gr"], M, legs[1]["norm"], legs[1]["mask"], p, SEG, RADIUS, MIN_CELLS, 1, step)
    old = E.register_segments(la, gb[0], gb[1], legs[1]["norm"], legs[1]["mask"], p, SEG, RADIUS, MIN_CELLS)
    for a, b in zip(one, old):
        assert (a["sums"][0] == b["sums"]).all() and a["r"] == b["r"] and (a["sx"], a["sy"], a["p0"], a["p1"]) == (b["sx"], b["sy"], b["p0"], b["p1"])
        assert (a["k"], a["yaw_on_border"], a["theta"], a["theta_hat"], a["zncc_k0"]) == (0, 0, 0.0, 0.0, b["r"]["zncc"])
        assert (a["sums"][0] == fan[a["seg"]]["sums"][mid]).all()                                          # and the fan's unrotated angle
    e_one, _ = Y.edges_yaw(orc, one, p, rows[0], 0, rows[1], N, 1, step); e_old, _ = E.edges(orc, old, p, rows[0], 0, rows[1], N)
    assert len(e_one) == len(e_old) > 0 and all(a["rel"].tobytes() == b["rel"].tobytes() and a["var"].tobytes() == b["var"].tobytes() for a, b in zip(e_one, e_old))
    # end to end: the heading of leg 1 after the oracle's solve, with the fan's edges and with the translation-only edges of the same rows
    plain, _ = E.edges(orc, fan, p, rows[0], 0, rows[1], N)
    dr = np.concatenate(rows); true = np.concatenate([legs[0]["true"], legs[1]["true"]])
    err = {}
    for what, ed in (("translation", plain), ("fan", es), ("fan_0.05", Y.edges_yaw(orc, fan, p, rows[0], 0, rows[1], N, nyaw, step, sigma_yaw_steps=0.05)[0])):
        poses, stats = orc.pg_solve(dr, E.lc_edges(orc, ed))
        err[what] = float(np.abs(_wrap(E.rows_of_poses12(poses)[N:, 2] - true[N:, 2])).mean())
    print("mean |yaw - true| of leg 1: before %.5f, %s" % (abs(m) * step, ", ".join("%s %.5f" % kv for kv in err.items())))
    assert err["fan"] < err["translation"] and err["fan_0.05"] < err["fan"]

"""The dense loop closures off the device: the numpy reference of tests/register_edges_ref.py by hand, dsss_register_edge (pure host
arithmetic of libdsss.so) against that reference on constructed rows, and the preconditions of the GPU tests on the reference alone
(tests/test_gpu_register_segments.py): the drifted two-leg survey registers in every segment, the anchor pings are unambiguous, and
the edges pull the drifted leg back under the oracle's pose-graph solve."""
import ctypes as C
import numpy as np
import pytest

from tests import mosaic_register_ref as R
from tests import register_edges_ref as E
from tests.pg_report_ref import residual_bound

E_ARG = -2
N, M = 640, 400
CELL, RADIUS, MIN_CELLS, SEG = 0.1, 8, 256, 80


# ---------------------------------------------------------------- the reference itself
def test_reference_centroid_by_hand():
    va = np.ones((3, 3), bool); va[0, 0] = False
    vb = np.ones((3, 3), bool); vb[2, 2] = False
    # zero shift: every cell but (0, 0) and (2, 2): ix 1 2 | 0 1 2 | 0 1, iy 0 0 | 1 1 1 | 2 2
    assert E.centroid_sums(va, vb, 0, 0) == (7, 7, 7)
    # (dx, dy) = (1, 0): a cells with ix <= 1 whose right neighbour is valid in b: (1,0) (0,1) (1,1) (0,2); (1,2) -> b(2,2) is invalid
    assert E.centroid_sums(va, vb, 1, 0) == (4, 2, 4)
    # (dx, dy) = (-1, 1): a cells ix >= 1, iy <= 1 -> b (ix - 1, iy + 1): all four valid
    assert E.centroid_sums(va, vb, -1, 1) == (4, 6, 2)
    assert E.centroid_sums(va, vb, 3, 0) == (0, 0, 0)
    # the same cells as the shift sums count
    ma = np.arange(1, 10).reshape(3, 3)
    s = R.shift_sums(ma, va, ma, vb, 1)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            assert E.centroid_sums(va, vb, dx, dy)[0] == s[dy + 1, dx + 1, 0]
    assert (E.shift_sums(ma, va, ma, vb, 1) == s).all()
    assert E.segments(10, 4) == [(0, 4), (4, 8), (8, 10)] and E.segments(8, 4) == [(0, 4), (4, 8)] and E.segments(3, 7) == [(0, 3)]


def _track(n, x0=0.0, step=1.0, yaw=0.0, y=0.0):
    """a straight track along the heading: ping i at x0 + i step along (cos yaw, sin yaw)"""
    s = x0 + step * np.arange(n)
    rows = np.zeros((n, 6)); rows[:, 2] = yaw; rows[:, 3] = s * np.cos(yaw); rows[:, 4] = y + s * np.sin(yaw)
    return rows


def test_reference_anchor_on_a_straight_track():
    rows = _track(10)                                               # pings at x = 0 .. 9, heading +x: scan lines are x = const
    assert E.anchor(rows, 0, 10, 3.2, 55.0) == (3, pytest.approx(0.6))          # 0.2 from ping 3, 0.8 from ping 4; y does not matter
    assert E.anchor(rows, 0, 10, 3.5, 0.0)[0] == 3                  # a tie between 3 and 4 goes to the lower index
    assert E.anchor(rows, 5, 10, 3.2, 0.0)[0] == 5                  # the range of a segment
    assert E.anchor(rows, 0, 10, -7.0, 0.0)[0] == 0 and E.anchor(rows, 0, 10, 70.0, 0.0)[0] == 9
    back = _track(10, yaw=np.pi)                                    # heading -x: ping i at x = -i
    assert E.anchor(back, 0, 10, -6.9, 1.0)[0] == 7
    same = np.zeros((4, 6))                                         # four pings in one place: all distances equal
    assert E.anchor(same, 1, 4, 2.0, 0.0) == (1, np.inf)
    up = _track(10, yaw=np.pi / 2)                                  # heading +y: scan lines are y = const
    assert E.anchor(up, 0, 10, 123.0, 4.4)[0] == 4


# ---------------------------------------------------------------- dsss_register_edge on constructed rows
def _grid(cell=CELL):
    from diasss_amd import capi
    return capi.MosaicParams(-3.0, -2.0, cell, 400, 300, 0, 0)


def _row(p0, p1, zncc=0.9, on_border=0, n=1000, sx=100000, sy=120000, off=(0.23, -0.11), pair=0, seg=0, dx=2, dy=-1):
    return dict(pair=pair, seg=seg, p0=p0, p1=p1, sx=sx, sy=sy,
                r=dict(dx=dx, dy=dy, off_x=off[0], off_y=off[1], zncc=zncc, zncc0=0.2, n=n, n0=n, on_border=on_border))


def _seg(row):
    from diasss_amd import capi
    s = np.zeros(1, capi.REGSEG_DTYPE)
    for k in ("pair", "seg", "p0", "p1", "sx", "sy"):
        s[k] = row[k]
    for k, v in row["r"].items():
        s["r"][k] = v
    return s[0]


def _rows(n, seed, x0, y0, yaw):
    """a track with roll, pitch, heave and a wiggle, so that every entry of the relative pose is exercised"""
    rng = np.random.default_rng(seed)
    s = 0.05 * (np.arange(n) + 0.5)
    rows = np.zeros((n, 6))
    rows[:, 0] = 0.02 * rng.standard_normal(n); rows[:, 1] = 0.02 * rng.standard_normal(n); rows[:, 2] = yaw + 0.01 * np.sin(s)
    rows[:, 3] = x0 + s * np.cos(yaw); rows[:, 4] = y0 + s * np.sin(yaw) + 0.3 * np.sin(s / 3.0); rows[:, 5] = 0.1 * rng.standard_normal(n)
    return rows


def _same_edge(dev, ref):
    assert int(dev["a"]) == ref["a"] and int(dev["b"]) == ref["b"]
    for name in ("rel", "var"):
        d, r = np.asarray(dev[name]), ref[name]
        assert (np.abs(d - r) <= residual_bound(r, 1.0)).all(), "%s: %s, reference %s" % (name, d, r)


CASES = {
    "forward": dict(row=_row(40, 120), base_a=0, base_b=200),
    "reversed": dict(row=_row(40, 120), base_a=900, base_b=100),            # ga > gb: the edge runs from b's ping to a's
    "at_the_threshold": dict(row=_row(0, 200, zncc=0.5), base_a=0, base_b=200),
    "on_the_border": dict(row=_row(0, 200, on_border=1, dx=8), base_a=0, base_b=200),
    "no_usable_shift": dict(row=_row(0, 200, zncc=-2.0, n=17, sx=0, sy=0, off=(0.0, 0.0), dx=0, dy=0), base_a=0, base_b=200),
    "below_the_threshold": dict(row=_row(0, 200, zncc=0.4999), base_a=0, base_b=200),
    "one_ping": dict(row=_row(77, 78), base_a=0, base_b=200),
    "first_segment_short_frame": dict(row=_row(0, 3, sx=30000, sy=20000), base_a=5, base_b=205),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_register_edge_against_the_reference(orc, name):
    from diasss_amd import capi
    cs = CASES[name]
    p = _grid()
    rows_a = _rows(200, 1, 2.0, 9.0, 0.02); rows_b = _rows(200, 2, 11.5, 14.0, np.pi - 0.03)
    ref = E.edge(orc, cs["row"], p, rows_a, cs["base_a"], rows_b, cs["base_b"])
    dev = capi.register_edge(_seg(cs["row"]), p, rows_a, cs["base_a"], rows_b, cs["base_b"])
    assert (dev is None) == (ref is None)
    assert (ref is None) == (name in ("on_the_border", "no_usable_shift", "below_the_threshold"))
    if ref is None:
        return
    assert ref["lead"] > 1e-6, "the constructed case has an ambiguous anchor ping (lead %g)" % ref["lead"]
    assert cs["row"]["p0"] <= ref["j"] < cs["row"]["p1"]
    if name == "reversed":
        assert ref["a"] == cs["base_b"] + ref["j"] and ref["b"] == cs["base_a"] + ref["i"]
    else:
        assert ref["a"] == cs["base_a"] + ref["i"] and ref["b"] == cs["base_b"] + ref["j"]
    _same_edge(dev, ref)


def test_register_edge_parameters_and_ties(orc):
    from diasss_amd import capi
    p = _grid(0.5)
    rows_a = _track(50, step=0.05); rows_b = _track(50, x0=0.3, step=0.05, yaw=np.pi, y=4.0)
    # the overlap centre at x = -3 + (4 + 0.5) 0.5 = -0.75 lies before every ping of a: ping 0; b (heading -x, ping i at x = -0.3 - 0.05 i) passes it at ping 9
    row = _row(0, 50, n=4, sx=16, sy=16, off=(0.0, 0.0))
    assert E.centre(row, p) == (-0.75, 0.25)
    ep = capi.RegEdgeParams(0.9, 2.0, 3.0, 0.25)
    ref = E.edge(orc, row, p, rows_a, 0, rows_b, 50, min_zncc=0.9, sigma_xy_cells=2.0, sigma_z=3.0, sigma_rot=0.25)
    dev = capi.register_edge(_seg(row), p, rows_a, 0, rows_b, 50, ep)
    _same_edge(dev, ref)
    assert ref["var"].tolist() == [0.0625] * 3 + [1.0, 1.0, 9.0] and (ref["i"], ref["j"]) == (0, 9)
    assert capi.register_edge(_seg(_row(0, 50, zncc=0.89, n=4, sx=16, sy=16)), p, rows_a, 0, rows_b, 50, ep) is None
    # pings in one place: every distance is equal, the lowest index of the range wins on both sides
    still = np.zeros((6, 6)); still[:, 5] = np.arange(6)
    dev = capi.register_edge(_seg(_row(2, 5, n=4, sx=16, sy=16, off=(0.0, 0.0))), p, still, 10, still, 20)
    assert (int(dev["a"]), int(dev["b"])) == (10, 22) and abs(dev["rel"][11] - 2.0) < 1e-15
    d = capi.reg_edge_params_default()
    assert (d.min_zncc, d.sigma_xy_cells, d.sigma_z, d.sigma_rot) == (E.MIN_ZNCC, E.SIGMA_XY_CELLS, E.SIGMA_Z, E.SIGMA_ROT) == (0.5, 1.0, 10.0, 1.0)


def test_register_edge_argument_errors():
    from diasss_amd import capi
    p = _grid()
    rows = _rows(100, 3, 0.0, 0.0, 0.0)
    good = _row(10, 60)
    assert capi.register_edge(_seg(good), p, rows, 0, rows, 100) is not None

    def code(seg=good, grid=p, ra=rows, rb=rows, ep=None):
        with pytest.raises(capi.DsssError) as ei:
            capi.register_edge(None if seg is None else _seg(seg), grid, ra, 0, rb, 100, ep)
        return ei.value.code

    assert code(seg=None) == E_ARG and code(grid=None) == E_ARG and code(ra=None) == E_ARG and code(rb=None) == E_ARG
    L = capi.lib()
    s = capi.RegSeg.from_buffer_copy(_seg(good).tobytes())
    assert L.dsss_register_edge(C.byref(s), C.byref(p), capi._ptr(rows), 100, 0, capi._ptr(rows), 100, 100, None, None) == E_ARG      # no edge
    assert code(seg=_row(10, 60, n=0)) == E_ARG and code(seg=_row(10, 60, n=-3)) == E_ARG       # an accepted peak without cells
    assert capi.register_edge(_seg(_row(10, 60, n=0, zncc=0.1)), p, rows, 0, rows, 100) is None   # ... a rejected one is just rejected
    assert code(seg=_row(60, 60)) == E_ARG and code(seg=_row(61, 60)) == E_ARG and code(seg=_row(-1, 60)) == E_ARG
    assert code(seg=_row(10, 101)) == E_ARG                                                      # past the frame's pings
    assert code(ra=np.zeros((0, 6))) == E_ARG and code(rb=np.zeros((0, 6))) == E_ARG
    for cell in (0.0, -0.1, np.inf, np.nan):
        assert code(grid=capi.MosaicParams(0.0, 0.0, cell, 10, 10, 0, 0)) == E_ARG
    for k in range(1, 4):
        for bad in (0.0, -1.0, np.inf, np.nan):
            v = [0.5, 1.0, 10.0, 1.0]; v[k] = bad
            assert code(ep=capi.RegEdgeParams(*v)) == E_ARG
    assert code(seg=_row(10, 60, zncc=0.1), ep=capi.RegEdgeParams(0.5, 0.0, 10.0, 1.0)) == E_ARG   # the parameters are checked before the row is judged


# ---------------------------------------------------------------- preconditions of the GPU tests, on the reference alone
@pytest.fixture(scope="module")
def survey(orc):
    """the two legs of synth.Survey(2, 640, 400, seed=7) with their dead-reckoning rows, leg 1 drifted (E.drift); the reference's
    segment rows of pair (0, 1) at cell 0.1, radius 8, 256 cells, no mask, 80 pings"""
    from diasss_amd import capi
    from diasss_amd.synth import Survey
    sv = Survey(2, N, M, seed=7)
    fr = []
    for f in range(2):
        raw = sv.frame(f).numpy().copy()
        pose, alt, gr = sv.inputs(f)
        fr.append(dict(gr=gr, norm=orc.normalize(raw), mask=orc.mask(raw), dr=np.ascontiguousarray(pose), true=np.ascontiguousarray(sv.poses_true[f])))
    rows = [fr[0]["dr"], E.drift(fr[1]["dr"])]
    g = [orc.geo_img(r, L["gr"], M) for r, L in zip(rows, fr)]
    gx = np.concatenate([a[0].ravel() for a in g]); gy = np.concatenate([a[1].ravel() for a in g])
    p = capi.mosaic_grid((gx.min(), gx.max(), gy.min(), gy.max()), CELL); p.use_mask = 0
    return dict(fr=fr, rows=rows, p=p)


def _register(orc, sv, rows):
    fr, p = sv["fr"], sv["p"]
    ga = orc.geo_img(np.ascontiguousarray(rows[0]), fr[0]["gr"], M); gb = orc.geo_img(np.ascontiguousarray(rows[1]), fr[1]["gr"], M)
    la = R.mean_layer(ga[0], ga[1], fr[0]["norm"], fr[0]["mask"], p, 0)
    return E.register_segments(la, gb[0], gb[1], fr[1]["norm"], fr[1]["mask"], p, SEG, RADIUS, MIN_CELLS)


def test_preconditions_of_the_gpu_tests(orc, survey):
    """Seen with this reference on the CPU: 8 segments with ZNCC 0.895 to 0.976; median |offset| 0.343 m before the solve and 0.015 m
    after it; median ZNCC at zero shift 0.209 before and 0.976 after."""
    rows, p = survey["rows"], survey["p"]
    before = _register(orc, survey, rows)
    assert len(before) == 8
    z = [s["r"]["zncc"] for s in before]
    print("zncc %s" % " ".join("%.3f" % v for v in z))
    assert all(E.accepted(s["r"]) for s in before) and min(z) >= 0.85
    es, src = E.edges(orc, before, p, rows[0], 0, rows[1], N)
    assert src == list(range(8))
    leads = [e["lead"] for e in es]
    print("anchor leads %s" % " ".join("%.3g" % v for v in leads))
    assert min(leads) > 1e-6
    assert all(0 <= e["a"] < N <= e["b"] < 2 * N for e in es)
    poses, stats = orc.pg_solve(np.concatenate(rows), E.lc_edges(orc, es))
    solved = E.rows_of_poses12(poses)
    after = _register(orc, survey, [solved[:N], solved[N:]])
    off0 = np.median([np.hypot(s["r"]["off_x"], s["r"]["off_y"]) for s in before])
    off1 = np.median([np.hypot(s["r"]["off_x"], s["r"]["off_y"]) for s in after])
    z0 = np.median([s["r"]["zncc0"] for s in before]); z1 = np.median([s["r"]["zncc0"] for s in after])
    print("median |offset| %.3f -> %.3f m, median zncc0 %.3f -> %.3f, %d LM iterations" % (off0, off1, z0, z1, int(stats[0])))
    assert off0 >= 0.2 and off1 <= 0.05 and z1 - z0 >= 0.5

"""The overlap registration off the device: the numpy reference against hand-computed values, and dsss_mosaic_register_peak (pure host
arithmetic of libdsss.so: score, peak, tie and sub-cell rules) against the reference's rule on constructed tables, bit for bit."""
import numpy as np
import pytest

from tests import mosaic_register_ref as R

E_ARG = -2
CELL = 0.1


# ---------------------------------------------------------------- the reference itself
def test_reference_sums_by_hand():
    ma = np.arange(1, 10).reshape(3, 3); mb = ma[::-1, ::-1].copy()
    va = np.ones((3, 3), bool); va[0, 0] = False
    vb = np.ones((3, 3), bool); vb[2, 2] = False
    s = R.shift_sums(ma, va, mb, vb, 1)
    assert s.shape == (3, 3, 6)
    assert s[1, 1].tolist() == [7, 35, 35, 147, 203, 203]          # (dx, dy) = (0, 0): every cell but the two invalid corners
    assert s[1, 2].tolist() == [4, 18, 18, 68, 94, 94]             # (1, 0): a 2 4 5 7 over b 7 5 4 2
    assert s[2, 0].tolist() == [4, 16, 16, 54, 74, 74]             # (-1, 1): a 2 3 5 6 over b 6 5 3 2
    z, ok = R.score(s[1, 1], 1)
    assert ok and z == (7 * 147 - 35 * 35) / np.sqrt(float(7 * 203 - 35 * 35) ** 2)
    assert R.score(s[1, 1], 8) == (-2.0, False)


def test_reference_recovers_a_moved_texture():
    rng = np.random.default_rng(3)
    big = rng.integers(0, 256, (80, 80))
    ma = big[8:72, 8:72].copy()
    mb = big[11:75, 6:70].copy()                                    # mb[y - 3, x + 2] = ma[y, x]: b is a moved by (dx, dy) = (2, -3)
    assert (mb[0:61, 2:64] == ma[3:64, 0:62]).all()
    va = rng.random((64, 64)) > 0.1; vb = rng.random((64, 64)) > 0.1
    va[20:30, 20:40] = False; vb[40:50, 5:25] = False               # holes
    s = R.shift_sums(ma, va, mb, vb, 4)
    p = R.peak(s, 4, 256, CELL)
    assert (p["dx"], p["dy"]) == (2, -3) and p["zncc"] == 1.0 and p["on_border"] == 0 and p["n"] > 2000
    z = R.scores(s, 4, 256)
    others = [z[j][i][0] for j in range(9) for i in range(9) if (i - 4, j - 4) != (2, -3)]
    assert max(others) < 0.2
    # |z-|, |z+| < 0.2 around a peak of 1: |p| <= 0.5 * 0.4 / 1.6
    assert abs(p["off_x"] - 2 * CELL) <= 0.125 * CELL and abs(p["off_y"] + 3 * CELL) <= 0.125 * CELL


# ---------------------------------------------------------------- dsss_mosaic_register_peak on constructed tables
def _entry(q, seed=1, n=400, reps=1):
    """six sums of n cells whose b agrees with a on a fraction q of them (q = 1: zncc 1), repeated reps times"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, n); b = np.where(rng.random(n) < q, a, rng.integers(0, 256, n))
    return [reps * int(v) for v in (n, a.sum(), b.sum(), (a * b).sum(), (a * a).sum(), (b * b).sum())]


def _table(radius, entries):
    S = 2 * radius + 1
    t = np.zeros((S, S, 6), np.uint64)
    for (dx, dy), e in entries.items():
        t[dy + radius, dx + radius] = e
    return t


def _check(t, radius, min_cells, **expect):
    from diasss_amd import capi
    dev = capi.mosaic_register_peak(t, radius, min_cells, CELL)
    ref = R.peak(t.astype(object), radius, min_cells, CELL)
    assert R.same_result(dev, ref), "library %s, reference %s" % ({k: getattr(dev, k) for k in R.FIELDS}, ref)
    for k, v in expect.items():
        assert ref[k] == v, "%s = %r, expected %r" % (k, ref[k], v)
    return ref


def test_peak_tie_at_different_distances():
    e = _entry(0.8)
    _check(_table(2, {(2, 0): e, (-1, 0): e, (0, 0): _entry(0.5), (1, 1): _entry(0.3)}), 2, 256, dx=-1, dy=0)
    _check(_table(2, {(0, 2): e, (1, -1): e, (-2, -2): e}), 2, 256, dx=1, dy=-1)


def test_peak_tie_at_equal_distance():
    e = _entry(0.8)
    _check(_table(2, {(1, 0): e, (-1, 0): e, (0, 1): e, (0, -1): e}), 2, 256, dx=0, dy=-1)       # the smallest dy
    _check(_table(2, {(1, 0): e, (-1, 0): e}), 2, 256, dx=-1, dy=0)                              # the same dy: the smallest dx
    _check(_table(2, {(1, 1): e, (-1, 1): e, (1, -1): e}), 2, 256, dx=1, dy=-1)


def test_peak_min_cells():
    t = _table(1, {(1, 0): _entry(0.9), (0, 0): _entry(0.5, n=399)})
    _check(t, 1, 400, dx=1, dy=0, n=400, n0=399, zncc0=-2.0)
    r = _check(t, 1, 399, dx=1, dy=0)
    assert r["zncc0"] > -1.0
    _check(t, 1, 401, dx=0, dy=0, zncc=-2.0, n=399)


def test_peak_constant_layer_and_no_usable_shift():
    const = [400, 400 * 7, 51000, 7 * 51000, 400 * 49, 6600000]     # a = 7 everywhere: da = 0
    _check(_table(1, {(0, 0): const, (1, 1): _entry(0.2)}), 1, 256, dx=1, dy=1, zncc0=-2.0)
    constb = [400, 51000, 400 * 7, 7 * 51000, 6600000, 400 * 49]    # b constant: db = 0
    _check(_table(1, {(0, 0): const, (-1, 0): constb}), 1, 256, dx=0, dy=0, zncc=-2.0, off_x=0.0, off_y=0.0, on_border=0, n=400)
    _check(_table(2, {}), 2, 1, dx=0, dy=0, zncc=-2.0, zncc0=-2.0, n=0, n0=0)


def test_peak_on_border_and_sub_cell():
    _check(_table(2, {(1, 1): _entry(0.6, 2), (2, 0): _entry(0.5, 3), (2, 2): _entry(0.4, 4), (0, 0): _entry(0.1, 5), (2, 1): _entry(0.9)}), 2, 256, dx=2, dy=1, on_border=1, off_x=2 * CELL, off_y=1 * CELL)
    # inside: both parabolas apply, and the higher neighbour pulls the offset towards it
    t = _table(2, {(0, 0): _entry(0.9), (1, 0): _entry(0.7, 2), (-1, 0): _entry(0.4, 3), (0, 1): _entry(0.5, 4), (0, -1): _entry(0.5, 5)})
    r = _check(t, 2, 256, dx=0, dy=0, on_border=0)
    assert 0.0 < r["off_x"] < 0.5 * CELL and abs(r["off_y"]) < 0.1 * CELL and r["off_y"] != 0.0
    # a neighbour that is not usable: no sub-cell part on that axis, the other axis keeps its own
    t2 = t.copy(); t2[1, 2] = _entry(0.5, 5, n=200)                 # (dx, dy) = (0, -1) below min_cells
    r2 = _check(t2, 2, 256, dx=0, dy=0, off_y=0.0)
    assert r2["off_x"] == r["off_x"]
    # a flat top: the denominator is 0
    e = _entry(0.9)
    _check(_table(2, {(0, 0): e, (1, 0): e, (-1, 0): e, (0, 1): _entry(0.5, 4), (0, -1): _entry(0.5, 5)}), 2, 256, dx=0, dy=0, off_x=0.0)
    # a plateau: den = 0 on both axes, and the tie goes to the centre
    _check(_table(1, {(i, j): e for i in (-1, 0, 1) for j in (-1, 0, 1)}), 1, 256, dx=0, dy=0, on_border=0, off_x=0.0, off_y=0.0)


def test_peak_radius_zero():
    _check(_table(0, {(0, 0): _entry(0.7)}), 0, 256, dx=0, dy=0, on_border=1, off_x=0.0, off_y=0.0, n=400, n0=400)
    _check(_table(0, {}), 0, 256, zncc=-2.0, on_border=0)


def test_peak_sums_beyond_64_bits():
    reps = 1 << 20
    e = {(0, 0): _entry(0.9, 1, 256, reps), (1, 0): _entry(0.7, 2, 256, reps), (-1, 0): _entry(0.6, 3, 256, reps),
         (0, 1): _entry(0.8, 4, 256, reps), (0, -1): _entry(0.3, 5, 256, reps), (1, 1): _entry(1.0, 6, 256, reps - 1)}
    n, Sab = e[(0, 0)][0], e[(0, 0)][3]
    assert n == 1 << 28 and n * Sab > 1 << 63
    r = _check(_table(1, {k: v for k, v in e.items() if k != (1, 1)}), 1, 256, dx=0, dy=0, n=1 << 28)
    assert 0.0 < r["zncc"] < 1.0 and r["off_x"] != 0.0 and r["off_y"] != 0.0
    _check(_table(1, e), 1, 256, dx=1, dy=1, zncc=1.0, on_border=1)
    # the rounding of the one conversion: the score of 200 entries of large sums, each as a radius-0 table of its own
    rng = np.random.default_rng(8)
    for _ in range(200):
        _check(_table(0, {(0, 0): _entry(rng.random(), int(rng.integers(1 << 30)), 256, int(rng.integers(1 << 19, 1 << 20)))}), 0, 1, on_border=1)


def test_peak_argument_errors():
    from diasss_amd import capi
    t = _table(1, {(0, 0): _entry(0.7)})
    for args in ((None, 1, 256, CELL), (t, -1, 256, CELL), (np.zeros(6, np.uint64), 17, 256, CELL), (t, 1, 0, CELL), (t, 1, 256, 0.0), (t, 1, 256, -1.0),
                 (t, 1, 256, float("nan")), (t, 1, 256, float("inf"))):
        with pytest.raises(capi.DsssError) as ei:
            capi.mosaic_register_peak(*args)
        assert ei.value.code == E_ARG
    with pytest.raises(ValueError):
        capi.mosaic_register_peak(t, 2, 256, CELL)                  # 9 x 6 sums are not a radius-2 table
    assert capi.mosaic_register_peak(t, 1, 256, CELL).n == 400
    r = capi.reg_params_default()
    assert (r.radius, r.min_cells) == (8, 256)

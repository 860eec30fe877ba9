"""The footprint rendering off the device: dsss_mosaic_footprint_steps (pure host arithmetic of libdsss.so, the one body the kernels
run) against tests/mosaic_footprint_ref.steps and against values worked out by hand, its argument errors and the defaults, and the
preconditions of the GPU cases on the reference alone."""
import math

import numpy as np
import pytest

from tests import mosaic_footprint_cases as K
from tests import mosaic_footprint_ref as FR

E_ARG = -2
NAN, INF = float("nan"), float("inf")


def up(x):
    return math.nextafter(x, math.inf)


# cell 0.0625 = 2^-4, so every quotient below is exact and the expected count follows by hand.  (max_steps, max_gap), sx, sy, n
CELL = 0.0625
STEP_TABLE = [
    ((4, 1.0), 0.0, 0.0, 1),                              # a zero step: t = 0 < 1
    ((4, 1.0), -0.0, 0.0, 1),
    ((4, 1.0), 1e-300, 0.0, 1),                           # t = ceil(1.6e-299) = 1
    ((4, 1.0), 0.0625, 0.0, 1),                           # exactly one cell: t = 1
    ((4, 1.0), up(0.0625), 0.0, 2),                       # one ulp above: the quotient is 1 + 2^-52, t = 2
    ((4, 1.0), 0.125, 0.0, 2), ((4, 1.0), up(0.125), 0.0, 3),
    ((4, 1.0), 0.25, 0.0, 4),                             # exactly max_steps cells: t = 4
    ((4, 1.0), up(0.25), 0.0, 4),                         # one ulp above: t = 5, cut to max_steps
    ((8, 1.0), 0.25, 0.0, 4), ((8, 1.0), up(0.25), 0.0, 5),
    ((8, 1.0), 0.5, 0.0, 8), ((8, 1.0), up(0.5), 0.0, 8),
    ((1, 1.0), 0.3, 0.0, 1),                              # max_steps 1: point samples
    ((4, 1.0), 1.0, 0.0, 4),                              # exactly max_gap: bridged (t = 16, cut)
    ((4, 1.0), up(1.0), 0.0, 1),                          # one ulp above max_gap: a jump, not bridged
    ((4, 1.0), 0.0, 1.0, 4), ((4, 1.0), 0.0, -up(1.0), 1),
    ((8, 0.2), 0.2, 0.0, 4), ((8, 0.2), up(0.2), 0.0, 1),
    ((4, 1.0), NAN, 0.0, 1), ((4, 1.0), 0.0, NAN, 1), ((4, 1.0), INF, 0.0, 1), ((4, 1.0), 0.0, -INF, 1), ((4, 1.0), NAN, INF, 1),
    ((4, 1.0), 0.1, 0.2, 4), ((4, 1.0), 0.2, 0.1, 4),     # the larger component, on either axis: ceil(3.2)
    ((4, 1.0), 0.13, 0.01, 3), ((4, 1.0), 0.01, 0.13, 3),  # ceil(2.08)
    ((4, 1.0), -0.13, 0.01, 3), ((4, 1.0), 0.01, -0.13, 3), ((4, 1.0), -0.13, -0.2, 4),
    ((4, 1.0), 0.07, -0.06, 2),                           # per axis, not the length: 0.092 m long, 1.12 cells on the larger axis
]


def test_steps_table():
    from diasss_amd import capi
    for params, sx, sy, n in STEP_TABLE:
        assert int(FR.steps(params, CELL, sx, sy)) == n, "reference: %r" % ((params, sx, sy),)
        assert capi.mosaic_footprint_steps(params, CELL, sx, sy) == n, "library: %r" % ((params, sx, sy),)


def test_steps_match_reference_on_random_steps():
    from diasss_amd import capi
    rng = np.random.default_rng(17)
    sx = rng.standard_normal(4000) * 0.2; sy = rng.standard_normal(4000) * 0.2
    sx[::97] = np.nan; sy[5::89] = np.inf; sx[7::31] *= 8.0
    for params, cell in (((4, 1.0), 0.05), ((8, 1.0), 0.02), ((3, 0.3), 0.1)):
        ref = FR.steps(params, cell, sx, sy)
        lib = np.array([capi.mosaic_footprint_steps(capi.FootprintParams(params[0], 0, params[1]), cell, a, b) for a, b in zip(sx, sy)])
        assert (lib == ref).all()
        assert set(np.unique(ref).tolist()) == set(range(1, params[0] + 1))


def test_steps_argument_errors_and_defaults():
    from diasss_amd import capi
    L = capi.lib()
    n = capi.C.c_int32(77)
    d = capi.footprint_params_default()
    assert (d.max_steps, d.max_gap, d.pad_) == (4, 1.0, 0) and FR.DEFAULTS == (4, 1.0)

    def rc(fp=(4, 1.0), cell=0.05, out=capi.C.byref(n)):
        p = capi.FootprintParams(fp[0], 0, fp[1]) if fp is not None else None
        return L.dsss_mosaic_footprint_steps(capi.C.byref(p) if p is not None else None, cell, 0.1, 0.0, out)
    assert rc() == 0 and n.value == 2
    assert rc(fp=None) == E_ARG and rc(out=None) == E_ARG
    assert rc(cell=0.0) == E_ARG and rc(cell=-0.05) == E_ARG and rc(cell=NAN) == E_ARG and rc(cell=INF) == E_ARG
    assert rc(fp=(0, 1.0)) == E_ARG and rc(fp=(9, 1.0)) == E_ARG and rc(fp=(-1, 1.0)) == E_ARG and rc(fp=(1, 1.0)) == 0 and rc(fp=(8, 1.0)) == 0
    assert rc(fp=(4, 0.0)) == E_ARG and rc(fp=(4, -1.0)) == E_ARG and rc(fp=(4, NAN)) == E_ARG and rc(fp=(4, INF)) == E_ARG
    with pytest.raises(capi.DsssError) as e:
        capi.mosaic_footprint_steps((9, 1.0), 0.05, 0.1, 0.0)
    assert e.value.code == E_ARG
    L.dsss_footprint_params_default(None)                                        # a NULL pointer is ignored


# ---------------------------------------------------------------- the preconditions of the GPU cases, on the reference alone
def _counts(orc, case, cell=0.05, params=(4, K.MAX_GAP)):
    fr = K.frames(orc, case)[0]
    Ax, Ay, Bx, By, na, nc = FR.step_counts(fr["gx"], fr["gy"], cell, params)
    return fr, Ax, Ay, Bx, By, na, nc


def test_precondition_step_counts(orc):
    """on T1 and T2 together, at cell 0.05 with the defaults: every along count and every across count 1..4 occurs at least 1 000
    times; at least 1 000 steps are cut by the cap, 100 refused by max_gap, 100 not finite; at least 50 wavefronts (64 consecutive
    columns of a ping) hold three or more distinct na.  Measured with the oracle's geo: T1 na 54 711 / 50 710 / 48 937 / 101 642,
    nc 255 836 / 164 / 0 / 0 (0.05 m bins on 0.05 m cells: the across counts come from T2); T2 na 48 735 / 46 440 / 42 053 / 118 772,
    nc 1 200 / 223 151 / 19 502 / 12 147; over both cases and both steps 148 319 cut by the cap, 800 refused by max_gap, 5 600 not
    finite; 387 wavefronts with three or more na on T2, none on T1."""
    na_all = np.zeros(5, np.int64); nc_all = np.zeros(5, np.int64)
    cut = gap = nonfinite = waves = 0
    for case in ("T1", "T2"):
        fr, Ax, Ay, Bx, By, na, nc = _counts(orc, case)
        a = np.bincount(na.ravel(), minlength=5); c = np.bincount(nc.ravel(), minlength=5)
        print("%s: na %s, nc %s" % (case, a[1:].tolist(), c[1:].tolist()))
        na_all += a; nc_all += c
        for sx, sy in ((Ax, Ay), (Bx, By)):
            with np.errstate(invalid="ignore"):
                fin = np.isfinite(sx) & np.isfinite(sy)
                l = np.maximum(np.abs(sx), np.abs(sy))
                cut += int((fin & (l <= K.MAX_GAP) & (np.ceil(l / 0.05) > 4)).sum())
                gap += int((fin & (l > K.MAX_GAP)).sum())
            nonfinite += int((~fin).sum())
        N, M = na.shape
        for c0 in range(0, M, 64):
            w = na[:, c0:c0 + 64]
            waves += int(sum(len(np.unique(r)) >= 3 for r in w))
    print("cut by the cap %d, refused by max_gap %d, not finite %d, wavefronts with three na %d" % (cut, gap, nonfinite, waves))
    assert (na_all[1:] >= 1000).all() and (nc_all[1:] >= 1000).all()
    assert cut >= 1000 and gap >= 100 and nonfinite >= 100 and waves >= 50


def test_precondition_holes(orc):
    """T0, no mask, defaults.  Cell 0.05: the point reference has enclosed single-cell holes (1 750 of 62 297 empty cells) and the
    footprint reference has none, and no more empty cells (60 543).  Cell 0.02: the footprint's enclosed single-cell holes are at most
    1 % of the point render's (800 of 549 503; the empty cells go from 2 698 722 of 3 292 110 to 375 343)."""
    for cell in K.T0_CELLS:
        pe, ph = FR.holes(K.render_ref(orc, "T0", cell, 0, None)[1])
        fe, fh = FR.holes(K.render_ref(orc, "T0", cell, 0, FR.DEFAULTS)[1])
        print("cell %g: point render %d empty, %d single-cell holes; footprint render %d empty, %d single-cell holes" % (cell, pe, ph, fe, fh))
        assert ph > 0 and fe <= pe
        if cell == 0.05:
            assert ph == 1750 and pe == 62297 and fh == 0
        else:
            assert fh * 100 <= ph


def test_precondition_counts_grow(orc):
    """cnt of the footprint reference >= cnt of the point reference in every cell, and sub-sample (0, 0) is the sample"""
    for case in ("T0", "T2"):
        a = K.render_ref(orc, case, 0.05, 1, None); b = K.render_ref(orc, case, 0.05, 1, FR.DEFAULTS)
        assert (b[1] >= a[1]).all() and b[3] > a[3]


@pytest.mark.parametrize("case", ["T0", "T1"])
def test_one_step_is_the_points(orc, case):
    for fr in K.frames(orc, case):
        lay, na, nc = FR.expand(fr["gx"], fr["gy"], 0.05, (1, K.MAX_GAP))
        lay = list(lay)
        assert (na == 1).all() and (nc == 1).all() and len(lay) == 1
        i, j, X, Y, live = lay[0]
        assert (i, j) == (0, 0) and live.all() and X.tobytes() == fr["gx"].tobytes() and Y.tobytes() == fr["gy"].tobytes()

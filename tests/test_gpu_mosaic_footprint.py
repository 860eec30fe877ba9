"""GPU parity of the footprint rendering (dsss_mosaic_render_footprint, dsss_mosaic_composite_footprint), exact on every layer and on
the cell counts.

Nothing expected comes from the code under test: geo coordinates are the oracle's geo_img, grey levels the oracle's normalised image,
the mask the oracle's filter mask; steps, sub-samples, sums, winners and fill come from tests/mosaic_footprint_ref.py, the gain
corrections from tests/mosaic_gain_ref.py and tests/mosaic_gain_bands_ref.py.  The cases are those of tests/mosaic_footprint_cases.py
(tests/test_mosaic_footprint_cpu.py proves their preconditions on the reference alone).  Frames 0 and 1 are the two legs, 2 is leg 0
set with the slant-corrected ground ranges of T2, 3 is leg 0 set and never extracted.  The rule that a listed frame has an even M of at
least 4 cannot be reached here: the extraction accepts no such frame, and a frame that is not extracted is DSSS_E_STATE first."""
import numpy as np
import pytest

from tests import mosaic_composite_ref as CR
from tests import mosaic_footprint_cases as K
from tests import mosaic_footprint_ref as FR
from tests import mosaic_gain_bands_ref as B
from tests import mosaic_gain_ref as G

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -2, -4
FRAME = {"T1": 0, "T2": 2}
BANDS = (8.0, 1.0, 2)                              # the legs' altitudes are 9 + sin(s / 7): both bands hold pings


@pytest.fixture(scope="module")
def ctx(orc):
    from diasss_amd import capi
    L = K.legs(orc)
    c = capi.Context(max_frames=4)
    for i, (l, gr) in enumerate(((L[0], L[0]["gr"]), (L[1], L[1]["gr"]), (L[0], K.t2_gr(orc)), (L[0], L[0]["gr"]))):
        c.frame_set(i, l["raw"], l["N"], l["M"], l["pose"], l["alt"], gr)
    c.extract_many([0, 1, 2])
    assert c.mosaic_gain_get() is None
    yield c
    c.close()


@pytest.fixture
def clean(ctx):
    """the context without a gain table, before and after the test"""
    ctx.mosaic_gain_set(None)
    yield ctx
    ctx.mosaic_gain_set(None)


def _dev_params(p, **kw):
    from diasss_amd import capi
    q = capi.MosaicParams(p.x0, p.y0, p.cell, p.W, p.H, p.use_mask, 0)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def _traj(orc, case):
    """the arguments that put a case's frame under its trajectory"""
    return {} if case == "T0" else dict(rpy6=K.t1_rows(orc), ping_off=np.zeros(1, np.int32))


def _ids(case):
    return [0, 1] if case == "T0" else [FRAME[case]]


def _check_render(dev, ref, what):
    for name, d, r in zip(("sum", "cnt", "img"), dev, ref[:3]):
        assert d.shape == r.shape, "%s %s: shape" % (what, name)
        bad = d.astype(np.int64) != r
        assert not bad.any(), "%s %s differs in %d cells, first at %s: device %s, reference %s" % (
            what, name, int(bad.sum()), np.argwhere(bad)[0].tolist(), d[bad][:4].tolist(), r[bad][:4].tolist())
    assert dev[0].dtype == np.uint32 and dev[1].dtype == np.uint32 and dev[2].dtype == np.uint8


def _check_comp(dev, info, ref, what):
    lay, counts = ref
    for name in CR.LAYERS:
        d = dev[name]
        assert d.shape == lay[name].shape, "%s %s: shape" % (what, name)
        bad = d.astype(np.int64) != lay[name]
        assert not bad.any(), "%s %s differs in %d cells, first at %s: device %s, reference %s" % (
            what, name, int(bad.sum()), np.argwhere(bad)[0].tolist(), d[bad][:4].tolist(), lay[name][bad][:4].tolist())
    assert (info.direct, info.filled, info.empty) == counts, "%s: counts %s, reference %s" % (what, (info.direct, info.filled, info.empty), counts)


def _comp_bytes(dev, info):
    return b"".join(dev[n].tobytes() for n in CR.LAYERS) + bytes(info)


def _code(fn, *a, **kw):
    from diasss_amd import capi
    with pytest.raises(capi.DsssError) as e:
        fn(*a, **kw)
    return e.value.code


# ---------------------------------------------------------------- 1. the footprint render
@pytest.mark.parametrize("use_mask", [0, 1])
@pytest.mark.parametrize("cell", K.T0_CELLS)
def test_render_t0(clean, orc, cell, use_mask):
    """both legs under their own poses with the defaults (NULL parameters); at cell 0.02 every count 1..4 occurs along and across"""
    p = K.full_grid(orc, "T0", cell, use_mask)
    ref = K.render_ref(orc, "T0", cell, use_mask, FR.DEFAULTS)
    dev = clean.mosaic_render_footprint([0, 1], _dev_params(p))
    _check_render(dev, ref, "T0 cell %g mask %d" % (cell, use_mask))
    assert ref[3] > K.render_ref(orc, "T0", cell, use_mask, None)[3]


@pytest.mark.parametrize("max_steps", K.T_STEPS)
@pytest.mark.parametrize("cell", K.T_CELLS)
@pytest.mark.parametrize("case", ["T1", "T2"])
def test_render_t1_t2(clean, orc, case, cell, max_steps):
    p = K.full_grid(orc, case, cell, 1)
    ref = K.render_ref(orc, case, cell, 1, (max_steps, K.MAX_GAP))
    dev = clean.mosaic_render_footprint(_ids(case), _dev_params(p), footprint=(max_steps, K.MAX_GAP), **_traj(orc, case))
    _check_render(dev, ref, "%s cell %g max_steps %d" % (case, cell, max_steps))


def test_render_on_a_grid_that_cuts_the_coverage(clean, orc):
    """half the extent in x and y out of the middle of T2's grid: parents off the grid have sub-samples on it and the reverse"""
    full = K.full_grid(orc, "T2", 0.05, 0)
    q = _dev_params(full, x0=full.x0 + (full.W // 4) * full.cell, y0=full.y0 + (full.H // 4) * full.cell, W=full.W // 2, H=full.H // 2)
    fr = K.frames(orc, "T2")
    ref = FR.render(fr, q, 0, (4, K.MAX_GAP))
    point = FR.render(fr, q, 0, (1, K.MAX_GAP))
    assert ref[3] > point[3] > 1000
    dev = clean.mosaic_render_footprint([2], q, footprint=(4, K.MAX_GAP), **_traj(orc, "T2"))
    _check_render(dev, ref, "clipped grid")


def test_counts_never_fall(clean, orc):
    """cnt of the footprint render >= cnt of the point render in every cell, on T2"""
    p = _dev_params(K.full_grid(orc, "T2", 0.05, 1))
    point = clean.mosaic_render([2], p, **_traj(orc, "T2"))
    foot = clean.mosaic_render_footprint([2], p, **_traj(orc, "T2"))
    assert (foot[1] >= point[1]).all() and int(foot[1].sum(dtype=np.int64)) > int(point[1].sum(dtype=np.int64))


# ---------------------------------------------------------------- 2. the footprint composite
@pytest.mark.parametrize("mode", CR.MODES)
def test_composite_t0(clean, orc, mode):
    p = K.full_grid(orc, "T0", 0.05, 0)
    for R in (0, 2):
        ref = K.composite_ref(orc, "T0", 0.05, 0, mode, R, FR.DEFAULTS)
        dev, info = clean.mosaic_composite_footprint([0, 1], _dev_params(p), mode=mode, fill_radius=R)
        _check_comp(dev, info, ref, "T0 mode %d R %d" % (mode, R))


@pytest.mark.parametrize("case", ["T1", "T2"])
def test_composite_t1_t2(clean, orc, case):
    p = K.full_grid(orc, case, 0.05, 1)
    filled = []
    for R in (0, 1, 4):
        ref = K.composite_ref(orc, case, 0.05, 1, CR.NEAR, R, FR.DEFAULTS)
        dev, info = clean.mosaic_composite_footprint(_ids(case), _dev_params(p), mode=CR.NEAR, fill_radius=R, footprint=FR.DEFAULTS, **_traj(orc, case))
        _check_comp(dev, info, ref, "%s R %d" % (case, R))
        filled.append(ref[1][1])
    assert filled[0] == 0 < filled[1] < filled[2]


def test_composite_under_gain_tables(clean, orc):
    """T1 under a column table, then under a two-band table: a sub-sample carries its parent's corrected value, column and band"""
    l = K.legs(orc)[0]
    M = l["M"]
    fr = K.frames(orc, "T1")[0]
    p = K.full_grid(orc, "T1", 0.05, 1)
    rng = np.random.default_rng(11)
    col = rng.integers(150, 400, M).astype(np.uint16); col[::7] = 0; col[3::11] = 65535
    two = rng.integers(100, 500, (2, M)).astype(np.uint16)
    bands_of = B.bands_of(BANDS, l["alt"])
    assert min((bands_of == 0).sum(), (bands_of == 1).sum()) > 100
    plain = K.composite_ref(orc, "T1", 0.05, 1, CR.NEAR, 1, FR.DEFAULTS)
    for tab, bands, val in ((col, None, G.apply(l["norm"], col)), (two, BANDS, B.apply_banded(l["norm"], l["alt"], two, BANDS))):
        ref = FR.composite([dict(fr, val=val)], p, 1, CR.NEAR, 1, FR.DEFAULTS)
        rref = FR.render([dict(fr, val=val)], p, 1, FR.DEFAULTS)
        clean.mosaic_gain_set(tab, bands=bands)
        dev, info = clean.mosaic_composite_footprint([0], _dev_params(p), fill_radius=1, **_traj(orc, "T1"))
        _check_comp(dev, info, ref, "under a table of %d bands" % (1 if bands is None else bands[2]))
        _check_render(clean.mosaic_render_footprint([0], _dev_params(p), **_traj(orc, "T1")), rref, "render under the table")
        held = ref[0]["fill"] < 255                                                # (most of the grid lies outside the swath)
        assert (ref[0]["img"] != plain[0]["img"])[held].mean() > 0.5 and (ref[0]["src_col"] == plain[0]["src_col"]).all()
    clean.mosaic_gain_set(None)


# ---------------------------------------------------------------- 3. one step is the point entries
def test_one_step_equals_the_point_entries(clean, orc):
    """max_steps 1: both entries give the bytes of dsss_mosaic_render / dsss_mosaic_composite of the same call, on T1 with its NaN rows,
    without and under a gain table"""
    M = K.legs(orc)[0]["M"]
    tab = np.random.default_rng(4).integers(100, 700, M).astype(np.uint16)
    for cell in K.T_CELLS:
        p = _dev_params(K.full_grid(orc, "T1", cell, 1))
        for t in (None, tab):
            clean.mosaic_gain_set(t)
            a = clean.mosaic_render([0], p, **_traj(orc, "T1"))
            b = clean.mosaic_render_footprint([0], p, footprint=(1, 0.5), **_traj(orc, "T1"))
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
            for mode, R in ((CR.NEAR, 0), (CR.MID, 2)):
                a = clean.mosaic_composite([0], p, mode=mode, fill_radius=R, **_traj(orc, "T1"))
                b = clean.mosaic_composite_footprint([0], p, mode=mode, fill_radius=R, footprint=(1, 0.5), **_traj(orc, "T1"))
                assert _comp_bytes(*a) == _comp_bytes(*b)
    q = _dev_params(K.full_grid(orc, "T0", 0.05, 0))
    clean.mosaic_gain_set(None)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(clean.mosaic_render([0, 1], q), clean.mosaic_render_footprint([0, 1], q, footprint=(1, 1.0))))


# ---------------------------------------------------------------- 4. order, repetition, NULL outputs
def test_order_repeat_and_null_outputs(clean, orc):
    from diasss_amd import capi
    p = _dev_params(K.full_grid(orc, "T0", 0.05, 1))
    got_r, got_c = [], []
    for ids in ([0, 1], [1, 0], [0, 1]):
        got_r.append(b"".join(a.tobytes() for a in clean.mosaic_render_footprint(ids, p)))
        got_c.append(_comp_bytes(*clean.mosaic_composite_footprint(ids, p, mode=CR.MID, fill_radius=2)))
    assert got_r[0] == got_r[1] == got_r[2] and got_c[0] == got_c[1] == got_c[2]
    _check_render(clean.mosaic_render_footprint([1, 0], p), K.render_ref(orc, "T0", 0.05, 1, FR.DEFAULTS), "ids reversed")
    # under a packed trajectory in either order of ids
    L = K.legs(orc)
    rpy = np.ascontiguousarray(np.concatenate([L[1]["pose"], L[0]["pose"]])); off = np.array([len(L[1]["pose"]), 0], np.int32)
    a = clean.mosaic_render_footprint([0, 1], p, rpy6=rpy, ping_off=off)
    b = clean.mosaic_render_footprint([1, 0], p, rpy6=rpy, ping_off=off[::-1].copy())
    assert b"".join(x.tobytes() for x in a) == b"".join(x.tobytes() for x in b) == got_r[0]
    # all outputs NULL: accepted, nothing comes down
    assert clean.mosaic_render_footprint([0, 1], p, download=False) is None
    assert clean.mosaic_composite_footprint([0, 1], p, want=()) == ({}, None)
    ids = np.array([0, 1], np.int32)
    assert clean.L.dsss_mosaic_render_footprint(clean.h, capi._ptr(ids), 2, None, None, capi.C.byref(p), None, None, None, None) == 0
    assert clean.L.dsss_mosaic_composite_footprint(clean.h, capi._ptr(ids), 2, None, None, capi.C.byref(p), None, None, None, None, None, None, None, None) == 0
    dev, info = clean.mosaic_composite_footprint([0, 1], p, want=("info",))
    assert dev == {} and (info.direct, info.filled, info.empty) == K.composite_ref(orc, "T0", 0.05, 1, CR.NEAR, 0, FR.DEFAULTS)[1]


# ---------------------------------------------------------------- 5. errors
def test_errors_leave_the_context_usable(clean, orc):
    nan, inf = float("nan"), float("inf")
    p = _dev_params(K.full_grid(orc, "T1", 0.1, 1))
    kw = _traj(orc, "T1")
    rref = K.render_ref(orc, "T1", 0.1, 1, (4, K.MAX_GAP))
    cref = K.composite_ref(orc, "T1", 0.1, 1, CR.NEAR, 0, FR.DEFAULTS)

    def still_right():
        _check_render(clean.mosaic_render_footprint([0], p, **kw), rref, "after an error")
        dev, info = clean.mosaic_composite_footprint([0], p, **kw)
        _check_comp(dev, info, cref, "after an error")

    still_right()
    for f in (clean.mosaic_render_footprint, clean.mosaic_composite_footprint):
        calls = [
            (E_ARG, lambda: f([0], p, footprint=(0, 1.0), **kw)),
            (E_ARG, lambda: f([0], p, footprint=(9, 1.0), **kw)),
            (E_ARG, lambda: f([0], p, footprint=(-3, 1.0), **kw)),
            (E_ARG, lambda: f([0], p, footprint=(4, 0.0), **kw)),
            (E_ARG, lambda: f([0], p, footprint=(4, -1.0), **kw)),
            (E_ARG, lambda: f([0], p, footprint=(4, nan), **kw)),
            (E_ARG, lambda: f([0], p, footprint=(4, inf), **kw)),
            (E_STATE, lambda: f([0, 3], p)),                                       # set, never extracted
            (E_STATE, lambda: f([3], p, footprint=(0, 1.0))),                      # the point entry's rules come first
            (E_ARG, lambda: f([0], p, rpy6=kw["rpy6"])),                           # a trajectory without ping_off
            (E_ARG, lambda: f([0, 0], p)),
            (E_ARG, lambda: f([0, 4], p)),
            (E_ARG, lambda: f([], p)),
            (E_ARG, lambda: f([0], _dev_params(p, cell=0.0), **kw)),
            (E_ARG, lambda: f([0], _dev_params(p, W=0), **kw)),
            (E_ARG, lambda: f([0], _dev_params(p, W=1 << 15, H=(1 << 13) + 1), **kw)),
        ]
        for code, call in calls:
            assert _code(call) == code
        still_right()
    assert _code(clean.mosaic_composite_footprint, [0], p, mode=4, **kw) == E_ARG
    assert _code(clean.mosaic_composite_footprint, [0], p, fill_radius=5, **kw) == E_ARG
    # a gain table of another M than a listed frame's: refused, and the table stays
    tab = np.full(K.legs(orc)[0]["M"], 256, np.uint16)
    clean.mosaic_gain_set(tab)
    assert _code(clean.mosaic_render_footprint, [0, 1], p) == E_ARG
    assert _code(clean.mosaic_composite_footprint, [0, 1], p) == E_ARG
    assert clean.mosaic_gain_get().tolist() == tab.tolist()
    still_right()                                                                  # (a table of 256s corrects nothing)
    clean.mosaic_gain_set(None)
    still_right()

"""GPU parity of the per-ping disagreement profile (include/dsss_profile.h): byte equality everywhere, never a tolerance.

Nothing expected comes from the code under test: geo coordinates, grey levels and masks are the oracle's, the records, residual layers
and sums are tests/mosaic_profile_ref.profile, gain corrections tests/mosaic_gain_ref.py and tests/mosaic_gain_bands_ref.py; the cases are
those of tests/mosaic_profile_cases.py (tests/test_mosaic_profile_cpu.py proves their preconditions on the reference alone), the canvas
scripts those of tests/mosaic_canvas_cases.py.  Frames 0 and 1 are the two legs, 2 is leg 0 set with the slant-corrected ground ranges
of T2, 3 is leg 0 set and never extracted.  No device fault is provoked and a broken canvas is not probed."""
import collections
import ctypes as C

import numpy as np
import pytest

from tests import mosaic_canvas_cases as K
from tests import mosaic_profile_cases as P
from tests import mosaic_profile_ref as PR
from tests import test_gpu_mosaic_canvas as TC

pytestmark = pytest.mark.gpu

E_ARG, E_STATE, E_CAPACITY = -2, -4, -5
# the table of driven entries (tests/test_mosaic_profile_cpu.py holds it to the header): test_every_driven_entry_is_called counts the calls
DRIVEN = ("dsss_profile_params_default", "dsss_profile_summary", "dsss_profile_mosaic", "dsss_profile_canvas")


@pytest.fixture(autouse=True)
def _nothing_after_a_hang():
    if TC._HUNG:
        pytest.skip("%s did not come back: nothing more is started on the GPU" % TC._HUNG[0])


@pytest.fixture(scope="module")
def ctx(orc):
    from diasss_amd import capi
    c = capi.Context(max_frames=4)
    TC._load(c, orc)
    assert c.mosaic_gain_get() is None
    yield c
    c.close()


@pytest.fixture
def clean(ctx):
    """the context without a gain table, before and after the test"""
    ctx.mosaic_gain_set(None)
    yield ctx
    ctx.mosaic_gain_set(None)


def _traj(orc, ids, rows):
    r = [K.rows_of(orc, i, rows[i]) for i in ids]
    return dict(rpy6=np.concatenate(r), ping_off=np.cumsum([0] + [len(x) for x in r[:-1]]).astype(np.int32))


def _run(c, orc, name, want=("stats", "diff", "info"), ids=None, prof="case", min_count=None):
    """dsss_profile_mosaic on a case (with its gain table installed), optionally with other ids, prof or min_count"""
    case = P.CASES[name]
    c.mosaic_gain_set(P.gain_table(orc, case["gain"]), bands=P.BANDS if case["gain"] == "two" else None)
    ids = case["ids"] if ids is None else ids
    return c.profile_mosaic(ids, TC._dev_params(P.grid(orc, case)), prof=case["prof"] if prof == "case" else prof,
                            min_count=case["min_count"] if min_count is None else min_count, want=want, **_traj(orc, ids, case["rows"]))


def _info(info):
    return {k: getattr(info, k) for k in PR.INFO_FIELDS}


def _check(dev, ref, what):
    stats, diff, info = dev
    assert stats.dtype.itemsize == 40 and stats.shape == ref[0].shape, "%s: %s records, the reference has %s" % (what, stats.shape, ref[0].shape)
    if stats.tobytes() != ref[0].tobytes():
        for f in PR.REC.names:
            bad = np.argwhere(stats[f] != ref[0][f])
            assert not len(bad), "%s: %s differs in %d places, first at ping, side %s: device %s, reference %s" % (
                what, f, len(bad), bad[0].tolist(), stats[f][tuple(bad[0])], ref[0][f][tuple(bad[0])])
    assert len(diff) == len(ref[1])
    for k, (d, r) in enumerate(zip(diff, ref[1])):
        assert d.dtype == np.int16 and d.shape == r.shape
        bad = np.argwhere(d != r)
        assert not len(bad), "%s: residual layer %d differs in %d samples, first at %s: device %d, reference %d" % (
            what, k, len(bad), bad[0].tolist(), d[tuple(bad[0])], r[tuple(bad[0])])
    assert _info(info) == ref[2], what                                             # rms with ==


def _bytes(dev):
    stats, diff, info = dev
    return stats.tobytes() + b"".join(d.tobytes() for d in diff) + bytes(info)


# ---------------------------------------------------------------- equality with the reference
@pytest.mark.parametrize("name", sorted(P.CASES))
def test_equals_the_reference(clean, orc, name):
    _check(_run(clean, orc, name), P.reference(orc, name), name)


# ---------------------------------------------------------------- output combinations
def test_each_output_alone_and_none(clean, orc):
    full = _run(clean, orc, "three")
    _check(full, P.reference(orc, "three"), "three")
    s, d, i = _run(clean, orc, "three", want=("stats",))
    assert d is None and i is None and s.tobytes() == full[0].tobytes()
    s, d, i = _run(clean, orc, "three", want=("diff",))
    assert s is None and i is None and all(a.tobytes() == b.tobytes() for a, b in zip(d, full[1])) and len(d) == 3
    s, d, i = _run(clean, orc, "three", want=("info",))
    assert s is None and d is None and bytes(i) == bytes(full[2])
    assert _run(clean, orc, "three", want=()) == (None, None, None)              # all three NULL: DSSS_OK
    _check(_run(clean, orc, "three"), P.reference(orc, "three"), "three after the partial calls")


# ---------------------------------------------------------------- determinism
def test_two_runs_and_another_order_of_ids(clean, orc):
    a, b = _run(clean, orc, "own_um1"), _run(clean, orc, "own_um1")
    assert _bytes(a) == _bytes(b)
    three = _run(clean, orc, "three")
    spans = P.pings_of(orc, P.CASES["three"])                                      # of ids [0, 1, 2]
    order = [2, 0, 1]
    other = _run(clean, orc, "three", ids=order)
    o = 0
    for k, i in enumerate(order):
        p0, N = spans[i]
        assert other[0][o:o + N].tobytes() == three[0][p0:p0 + N].tobytes(), "frame %d" % i
        assert other[1][k].tobytes() == three[1][i].tobytes(), "frame %d" % i
        o += N
    assert _info(other[2]) == _info(three[2])


# ---------------------------------------------------------------- the mosaic is untouched
def test_render_and_gain_table_are_untouched(clean, orc):
    case = P.CASES["gain_col"]
    tab = P.gain_table(orc, "col")
    clean.mosaic_gain_set(tab)
    p = TC._dev_params(P.grid(orc, case))
    kw = _traj(orc, case["ids"], case["rows"])
    before = b"".join(a.tobytes() for a in clean.mosaic_render(case["ids"], p, **kw))
    _check(_run(clean, orc, "gain_col"), P.reference(orc, "gain_col"), "gain_col")
    assert clean.mosaic_gain_get().tobytes() == tab.tobytes()
    assert b"".join(a.tobytes() for a in clean.mosaic_render(case["ids"], p, **kw)) == before


# ---------------------------------------------------------------- canvas
CANVAS_SCRIPTS = {"add": (K.ADD_AT_ONCE, 0), "move_t1": (K.MOVE_T1, 0), "mixed": (K.MIXED_B, 1), "shift": (K.move_script(0.01), 0)}


@pytest.mark.parametrize("move", TC.MOVES)
@pytest.mark.parametrize("script", sorted(CANVAS_SCRIPTS))
def test_canvas_profile_is_the_fresh_profile(clean, orc, script, move):
    steps, um = CANVAS_SCRIPTS[script]
    p = K.grid(orc, um)
    state = K.final_state(steps)
    S = sorted(state)
    cv = TC._canvas(clean, p, "point", move)
    try:
        TC._play(cv, orc, steps)
        before = (TC._bytes(cv), cv.frames(), cv.dirty(reset=False))
        lists = [S, S[::-1]] + ([S[1:]] if len(S) > 1 else [])                     # all, reversed, a strict subset
        for ids in lists:
            dev = cv.profile(ids)
            fresh = clean.profile_mosaic(S, TC._dev_params(p), prof=[S.index(i) for i in ids], **_traj(orc, S, state))
            assert _bytes(dev) == _bytes(fresh), "%s %s" % (script, ids)
            _check(dev, P.state_reference(orc, state, ids, um), "%s %s" % (script, ids))
        dev = cv.profile(S, min_count=3)
        _check(dev, P.state_reference(orc, state, S, um, 3), "%s min_count 3" % script)
        assert (TC._bytes(cv), cv.frames(), cv.dirty(reset=False)) == before
        TC._check_rows(cv, orc, state)
    finally:
        cv.close()


# ---------------------------------------------------------------- refusals
def test_refusals_of_the_fresh_entry(clean, orc):
    from diasss_amd import capi
    case = P.CASES["own_um1"]
    p = TC._dev_params(P.grid(orc, case))
    kw = _traj(orc, [0, 1], case["rows"])
    ref = P.reference(orc, "own_um1")
    own = np.concatenate([K.rows_of(orc, 0, "own")] * 2)
    huge = capi.MosaicParams(0.0, 0.0, 0.1, 1 << 15, (1 << 13) + 1, 1, 0)          # W H over 2^28
    calls = [
        (E_ARG, lambda: clean.profile_mosaic([0, 1], p, prof=[-1], **kw)),
        (E_ARG, lambda: clean.profile_mosaic([0, 1], p, prof=[2], **kw)),
        (E_ARG, lambda: clean.profile_mosaic([0, 1], p, prof=[1, 1], **kw)),
        (E_ARG, lambda: clean.profile_mosaic([0, 1], p, prof=[], **kw)),            # nprof 0
        (E_ARG, lambda: clean.profile_mosaic([0, 1], p, min_count=0, **kw)),
        (E_ARG, lambda: clean.profile_mosaic([0, 1], p, min_count=(1 << 24) + 1, **kw)),
        (E_ARG, lambda: clean.profile_mosaic([0, 0], p, rpy6=own, ping_off=np.array([0, 640], np.int32))),
        (E_STATE, lambda: clean.profile_mosaic([0, 3], p, rpy6=own, ping_off=np.array([0, 640], np.int32))),      # set, never extracted
        (E_ARG, lambda: clean.profile_mosaic([0, 1], huge, **kw)),
        (E_ARG, lambda: clean.profile_mosaic([0, 1], p, rpy6=kw["rpy6"])),          # a trajectory without ping_off
        (E_STATE, lambda: clean.profile_mosaic([0, 3], p, prof=[5], min_count=0, rpy6=own, ping_off=np.array([0, 640], np.int32))),   # the render's rules come first
    ]
    for k, (code, call) in enumerate(calls):
        assert TC._code(call) == code, "refusal %d" % k
        _check(_run(clean, orc, "own_um1"), ref, "after refusal %d" % k)
    assert clean.profile_mosaic([0, 1], p, min_count=1 << 24, **kw)[2].n == 0       # the largest min_count is legal and compares nothing
    L = clean.L
    assert L.dsss_profile_mosaic(None, None, 0, None, None, None, None, 0, None, None, None, None) == E_ARG


def test_refusals_of_the_canvas_entry(clean, orc):
    l = K.legs(orc)[0]
    p = K.grid(orc, 1)
    state = {0: "own", 1: "own"}
    fp = TC._canvas(clean, p, "fp4", 0)
    cv = TC._canvas(clean, p, "point", 0)
    try:
        TC._put(fp, orc, state); TC._put(cv, orc, state)
        ref = P.state_reference(orc, state, [0, 1], 1)
        before = TC._bytes(cv)
        calls = [
            (E_ARG, lambda: fp.profile([0])),                                       # a footprint canvas
            (E_ARG, lambda: cv.profile([2])),                                       # not on the canvas
            (E_ARG, lambda: cv.profile([0, 2])),
            (E_ARG, lambda: cv.profile([1, 1])),
            (E_ARG, lambda: cv.profile([])),
            (E_ARG, lambda: cv.profile([0], min_count=0)),
            (E_ARG, lambda: cv.profile([0], min_count=(1 << 24) + 1)),
        ]
        for k, (code, call) in enumerate(calls):
            assert TC._code(call) == code, "refusal %d" % k
            _check(cv.profile([0, 1]), ref, "after refusal %d" % k)
        assert clean.L.dsss_profile_canvas(None, None, 0, None, None, None, None) == E_ARG
        # a frame set again since its put: its images are no longer those that were added
        clean.frame_set(0, l["raw"], l["N"], l["M"], l["pose"], l["alt"], l["gr"])
        assert TC._code(cv.profile, [0]) == E_STATE and TC._code(cv.profile, [1, 0]) == E_STATE
        _check(cv.profile([1]), P.state_reference(orc, state, [1], 1), "the frame that is not stale")
        clean.extract(0)                                                           # the same images again, but the canvas cannot know
        assert TC._code(cv.profile, [0]) == E_STATE
        cv.clear(); TC._put(cv, orc, state)
        _check(cv.profile([0, 1]), ref, "after clear")
        # the gain table changed since the put
        clean.mosaic_gain_set(P.gain_table(orc, "col"))
        assert TC._code(cv.profile, [0]) == E_STATE
        clean.mosaic_gain_set(None)
        assert TC._code(cv.profile, [0]) == E_STATE
        cv.clear(); TC._put(cv, orc, state)
        _check(cv.profile([0, 1]), ref, "after the table went and the canvas was cleared")
        assert TC._bytes(cv) == before
    finally:
        fp.close(); cv.close()


# ---------------------------------------------------------------- sample limit
@pytest.fixture(scope="module")
def big(orc):
    """leg 0 as frame 0 and a frame of 4200 x 4000 (the sample-limit test's shape of tests/test_gpu_mosaic.py) as frame 1"""
    from diasss_amd import capi
    from tests import helpers as H
    N, M = 4200, 4000
    assert N * M > 1 << 24
    l = K.legs(orc)[0]
    pose, alt, gr = H.track(N, M, 0, seed=3)
    raw = np.random.default_rng(11).random((N, M)) * 200.0 + 1.0
    c = capi.Context(max_frames=2)
    c.frame_set(0, l["raw"], l["N"], l["M"], l["pose"], l["alt"], l["gr"])
    c.frame_set(1, raw, N, M, pose, alt, gr)
    c.extract(0); c.extract(1)
    yield c
    c.close()


def test_sample_limit(big, orc):
    from diasss_amd import capi
    l = K.legs(orc)[0]
    one = capi.MosaicParams(-5000.0, -5000.0, 10000.0, 1, 1, 0, 0)
    assert TC._code(big.mosaic_render, [1], one) == E_CAPACITY
    assert TC._code(big.profile_mosaic, [1], one) == E_CAPACITY
    assert TC._code(big.profile_mosaic, [0, 1], one, prof=[0], want=("info",)) == E_CAPACITY
    stats, diff, info = big.profile_mosaic([0], one)                               # the next call works: every sample in the one cell, none compared
    assert int(stats["binned"].astype(np.int64).sum()) == l["N"] * l["M"] == info.binned and info.n == 0 and (diff[0] == PR.NONE).all()


# ---------------------------------------------------------------- the table of driven entries
def test_every_driven_entry_is_called(clean, orc):
    from diasss_amd import capi
    counts = collections.Counter()

    class Counting:
        def __init__(self, L):
            self._L = L

        def __getattr__(self, name):
            fn = getattr(self._L, name)
            if name.startswith("dsss_profile_") and name in DRIVEN:
                def call(*a):
                    counts[name] += 1
                    return fn(*a)
                return call
            return fn

    plain, real = clean.L, capi._LIB
    clean.L = Counting(plain); capi._LIB = Counting(real)
    try:
        capi.profile_params_default()
        stats = _run(clean, orc, "alone")[0]
        capi.profile_summary(stats)
        cv = TC._canvas(clean, K.grid(orc, 0), "point", 0)
        TC._put(cv, orc, {0: "own"}); cv.profile([0]); cv.close()
    finally:
        clean.L = plain; capi._LIB = real
    assert sorted(counts) == sorted(DRIVEN), "never called: %s" % sorted(set(DRIVEN) - set(counts))

"""GPU parity of the mosaic canvas (include/dsss_canvas.h): byte equality everywhere.

The contract every case is held to is the header's invariant: after every call that returns DSSS_OK, and after every refused call, the
canvas reads (sum, cnt, img) what a fresh render of its frames under their stored rows reads.  Nothing expected comes from the code
under test: geo coordinates are the oracle's geo_img, grey levels and mask the oracle's, the sums tests/mosaic_footprint_ref.render, gain
corrections tests/mosaic_gain_ref.py and tests/mosaic_gain_bands_ref.py; scripts, rows and windows are those of
tests/mosaic_canvas_cases.py (tests/test_mosaic_canvas_cpu.py proves their preconditions on the reference alone).  Frames 0 and 1 are the
two legs, 2 is leg 0 set with the slant-corrected ground ranges of T2, 3 is leg 0 set and never extracted.  The footprint rule (an even
M of at least 4) cannot be reached: the extraction accepts no such frame, and a frame that is not extracted is DSSS_E_STATE first."""
import ctypes as C
import threading
import time

import numpy as np
import pytest

from tests import mosaic_canvas_cases as K
from tests import mosaic_gain_bands_ref as B
from tests import mosaic_gain_ref as G

pytestmark = pytest.mark.gpu

E_ARG, E_STATE, E_CAPACITY = -2, -4, -5
MOVES = (0, 1)                                     # DSSS_CANVAS_MOVE_AUTO, DSSS_CANVAS_MOVE_SPLIT
BANDS = (8.0, 1.0, 2)                              # the legs' altitudes are 9 + sin(s / 7): both bands hold pings
CONFIGS = [(kind, move, um) for kind in K.KINDS for move in MOVES for um in (0, 1)]
MODES = [(kind, move) for kind in K.KINDS for move in MOVES]
# the table of driven entries (tests/test_mosaic_canvas_cpu.py holds it to the header): test_every_driven_entry_is_called counts the calls
DRIVEN = ("dsss_canvas_params_default", "dsss_canvas_create", "dsss_canvas_destroy", "dsss_canvas_put", "dsss_canvas_remove", "dsss_canvas_clear",
          "dsss_canvas_read", "dsss_canvas_dirty", "dsss_canvas_frames", "dsss_canvas_rows", "dsss_canvas_frame_window")
_HUNG = []                                         # threads that did not come back: nothing more is started on the GPU


@pytest.fixture(autouse=True)
def _nothing_after_a_hang():
    if _HUNG:
        pytest.skip("%s did not come back: nothing more is started on the GPU" % _HUNG[0])


def _load(c, orc, extract=(0, 1, 2)):
    from tests import mosaic_footprint_cases as FK
    L = K.legs(orc)
    for i, (l, gr) in enumerate(((L[0], L[0]["gr"]), (L[1], L[1]["gr"]), (L[0], FK.t2_gr(orc)), (L[0], L[0]["gr"]))):
        if i < c.max_frames:
            c.frame_set(i, l["raw"], l["N"], l["M"], l["pose"], l["alt"], gr)
    c.extract_many([i for i in extract if i < c.max_frames])


@pytest.fixture(scope="module")
def ctx(orc):
    from diasss_amd import capi
    c = capi.Context(max_frames=4)
    _load(c, orc)
    assert c.mosaic_gain_get() is None
    yield c
    c.close()


@pytest.fixture
def clean(ctx):
    """the context without a gain table, before and after the test"""
    ctx.mosaic_gain_set(None)
    yield ctx
    ctx.mosaic_gain_set(None)


def _dev_params(p):
    from diasss_amd import capi
    return capi.MosaicParams(p.x0, p.y0, p.cell, p.W, p.H, p.use_mask, 0)


def _canvas(c, p, kind, move):
    return c.canvas(_dev_params(p), footprint=K.KINDS[kind], move=move)


def _N(orc, fid):
    return K.legs(orc)[1 if fid == 1 else 0]["N"]


def _put(cv, orc, frames):
    """one put step {id: rows name}: the poses the frames were set with go as NULL, everything else as a packed trajectory"""
    ids = list(frames)
    if all(n == "own" for n in frames.values()):
        return cv.put(ids)
    rows = [K.rows_of(orc, i, frames[i]) for i in ids]
    off = np.cumsum([0] + [len(r) for r in rows[:-1]]).astype(np.int32)
    return cv.put(ids, rpy6=np.concatenate(rows), ping_off=off)


def _play(cv, orc, script):
    info = None
    for step in script:
        if step[0] == "put":
            info = _put(cv, orc, step[1])
        elif step[0] == "remove":
            cv.remove(step[1])
        else:
            cv.clear()
    return info


def _bytes(cv):
    return b"".join(a.tobytes() for a in cv.read())


def _check(cv, ref, what):
    dev = cv.read()
    for name, d, r in zip(("sum", "cnt", "img"), dev, ref[:3]):
        assert d.shape == r.shape, "%s %s: shape" % (what, name)
        bad = d.astype(np.int64) != r
        assert not bad.any(), "%s %s differs in %d cells, first at %s: device %s, reference %s" % (
            what, name, int(bad.sum()), np.argwhere(bad)[0].tolist(), d[bad][:4].tolist(), r[bad][:4].tolist())
    assert dev[0].dtype == np.uint32 and dev[1].dtype == np.uint32 and dev[2].dtype == np.uint8


def _check_rows(cv, orc, state):
    assert cv.frames() == sorted(state)
    for i, name in state.items():
        assert cv.rows(i, _N(orc, i)).tobytes() == K.rows_of(orc, i, name).tobytes(), "rows of frame %d" % i


def _fresh(c, p, kind, state, orc):
    """the bytes of the fresh render entry for a state"""
    ids = sorted(state)
    rows = [K.rows_of(orc, i, state[i]) for i in ids]
    off = np.cumsum([0] + [len(r) for r in rows[:-1]]).astype(np.int32)
    kw = dict(rpy6=np.concatenate(rows), ping_off=off)
    out = c.mosaic_render(ids, _dev_params(p), **kw) if K.KINDS[kind] is None else c.mosaic_render_footprint(ids, _dev_params(p), footprint=K.KINDS[kind], **kw)
    return b"".join(a.tobytes() for a in out)


def _code(fn, *a, **kw):
    from diasss_amd import capi
    with pytest.raises(capi.DsssError) as e:
        fn(*a, **kw)
    return e.value.code


def _pings(orc, kind, move, added=(), moved=()):
    """the workgroups a put launches: one per ping of an added frame; of a moved one, one (fused) or two (split)"""
    fused = K.KINDS[kind] is None and move == 0
    return sum(_N(orc, i) for i in added) + sum(_N(orc, i) * (1 if fused else 2) for i in moved)


# ---------------------------------------------------------------- add
@pytest.mark.parametrize("kind,move,um", CONFIGS)
def test_add(clean, orc, kind, move, um):
    p = K.grid(orc, um)
    ref = K.reference(orc, {0: "own", 1: "own"}, p, um, kind)
    a, b = _canvas(clean, p, kind, move), _canvas(clean, p, kind, move)
    try:
        assert a.frames() == [] and not any(x.any() for x in a.read()) and a.dirty(reset=False) is None
        info = _play(a, orc, K.ADD_AT_ONCE)
        assert (info.added, info.moved, info.skipped, info.pings) == (2, 0, 0, _pings(orc, kind, move, added=(0, 1)))
        _play(b, orc, K.ADD_IN_TURN)
        _check(a, ref, "put [0, 1]")
        assert _bytes(a) == _bytes(b) == _fresh(clean, p, kind, {0: "own", 1: "own"}, orc)
        _check_rows(a, orc, {0: "own", 1: "own"}); _check_rows(b, orc, {0: "own", 1: "own"})
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------- move
@pytest.mark.parametrize("kind,move,um", CONFIGS)
def test_move_to_t1_and_back(clean, orc, kind, move, um):
    p = K.grid(orc, um)
    cv = _canvas(clean, p, kind, move)
    try:
        _play(cv, orc, K.MOVE_T1[:1])
        before = _bytes(cv)
        _check(cv, K.reference(orc, {0: "own"}, p, um, kind), "own")
        info = _play(cv, orc, K.MOVE_T1[1:])
        assert (info.added, info.moved, info.skipped, info.pings) == (0, 1, 0, _pings(orc, kind, move, moved=(0,)))
        _check(cv, K.reference(orc, {0: "t1"}, p, um, kind), "moved to t1")
        _check_rows(cv, orc, {0: "t1"})
        assert _bytes(cv) == _fresh(clean, p, kind, {0: "t1"}, orc) != before
        _play(cv, orc, K.MOVE_T1_BACK[2:])
        assert _bytes(cv) == before
        _check_rows(cv, orc, {0: "own"})
    finally:
        cv.close()


@pytest.mark.parametrize("d", K.SHIFTS)
@pytest.mark.parametrize("kind,move,um", CONFIGS)
def test_move_by_a_shift(clean, orc, kind, move, um, d):
    p = K.grid(orc, um)
    cv = _canvas(clean, p, kind, move)
    try:
        script = K.move_script(d)
        info = _play(cv, orc, script)
        assert (info.added, info.moved, info.skipped) == (0, 1, 0)
        state = K.final_state(script)
        _check(cv, K.reference(orc, state, p, um, kind), "shift %g" % d)
        _check_rows(cv, orc, state)
    finally:
        cv.close()


# ---------------------------------------------------------------- remove
@pytest.mark.parametrize("kind,move,um", CONFIGS)
def test_remove(clean, orc, kind, move, um):
    p = K.grid(orc, um)
    cv = _canvas(clean, p, kind, move)
    try:
        _play(cv, orc, K.REMOVE_0)
        _check(cv, K.reference(orc, {1: "own"}, p, um, kind), "leg 1 alone")
        _check_rows(cv, orc, {1: "own"})
        _play(cv, orc, K.REMOVE_ALL[len(K.REMOVE_0):])
        assert cv.frames() == [] and not any(x.any() for x in cv.read())
    finally:
        cv.close()


# ---------------------------------------------------------------- skip
@pytest.mark.parametrize("kind,move,um", CONFIGS)
def test_skip_and_one_flipped_bit(clean, orc, kind, move, um):
    p = K.grid(orc, um)
    cv = _canvas(clean, p, kind, move)
    try:
        _put(cv, orc, {0: "t1", 1: "own"})
        before = _bytes(cv)
        cv.dirty()
        info = _put(cv, orc, {0: "t1"})
        assert (info.added, info.moved, info.skipped, info.pings, info.win[2]) == (0, 0, 1, 0, 0)
        info = cv.put([1], rpy6=K.rows_of(orc, 1, "own"), ping_off=np.zeros(1, np.int32))      # the bytes the frame was set with, handed in
        assert (info.added, info.moved, info.skipped, info.pings, info.win[2]) == (0, 0, 1, 0, 0)
        assert _bytes(cv) == before and cv.dirty() is None
        # a NaN payload: one mantissa bit of a row that is NaN
        rows = K.rows_of(orc, 0, "t1").copy()
        assert np.isnan(rows[501, 3])
        rows.view(np.uint64)[501, 3] ^= np.uint64(1)
        assert np.isnan(rows[501, 3]) and rows.tobytes() != K.rows_of(orc, 0, "t1").tobytes()
        info = cv.put([0], rpy6=rows, ping_off=np.zeros(1, np.int32))
        assert (info.added, info.moved, info.skipped, info.pings) == (0, 1, 0, _pings(orc, kind, move, moved=(0,)))
        assert _bytes(cv) == before and cv.rows(0, _N(orc, 0)).tobytes() == rows.tobytes()
        # a signed zero in a component the geometry does not read
        own = K.rows_of(orc, 1, "own").copy()
        col = [k for k in (0, 1, 5) if own[7, k] == 0.0 and not np.signbit(own[7, k])]
        assert col, own[7]
        own[7, col[0]] = -0.0
        info = cv.put([1], rpy6=own, ping_off=np.zeros(1, np.int32))
        assert (info.added, info.moved, info.skipped) == (0, 1, 0)
        assert _bytes(cv) == before and cv.rows(1, _N(orc, 1)).tobytes() == own.tobytes()
    finally:
        cv.close()


# ---------------------------------------------------------------- mixed call
@pytest.mark.parametrize("kind,move,um", CONFIGS)
def test_mixed_call_and_another_order(clean, orc, kind, move, um):
    p = K.grid(orc, um)
    a, b = _canvas(clean, p, kind, move), _canvas(clean, p, kind, move)
    try:
        info = _play(a, orc, K.MIXED_A)
        assert (info.added, info.moved, info.skipped, info.pings) == (1, 1, 1, _pings(orc, kind, move, added=(1,), moved=(0,)))
        _play(b, orc, K.MIXED_B)
        state = K.final_state(K.MIXED_A)
        _check(a, K.reference(orc, state, p, um, kind), "mixed call")
        assert _bytes(a) == _bytes(b)
        _check_rows(a, orc, state); _check_rows(b, orc, state)
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------- gain
@pytest.mark.parametrize("kind,move", MODES)
def test_under_gain_tables(clean, orc, kind, move):
    l = K.legs(orc)[0]
    M = l["M"]
    p = K.grid(orc, 1)
    rng = np.random.default_rng(11)
    col = rng.integers(150, 400, M).astype(np.uint16); col[::7] = 0; col[3::11] = 65535
    two = rng.integers(100, 500, (2, M)).astype(np.uint16)
    plain = K.reference(orc, {0: "d0.01"}, p, 1, kind)
    cv = _canvas(clean, p, kind, move)
    try:
        for tag, tab, bands, val in (("col", col, None, G.apply(l["norm"], col)), ("two", two, BANDS, B.apply_banded(l["norm"], l["alt"], two, BANDS))):
            clean.mosaic_gain_set(tab, bands=bands)
            cv.clear()
            _play(cv, orc, [("put", {0: "own"}), ("put", {0: "d0.01"})])
            ref = K.reference(orc, {0: "d0.01"}, p, 1, kind, vals={0: val}, tag=tag)
            assert (ref[0] != plain[0]).any()
            _check(cv, ref, "under the %s table" % tag)
        # the table changes under a canvas that holds a frame: put and remove are refused, the bytes stay, clear recovers
        before = _bytes(cv)
        clean.mosaic_gain_set(col)
        assert _code(_put, cv, orc, {0: "own"}) == E_STATE and _code(_put, cv, orc, {2: "t1"}) == E_STATE and _code(cv.remove, [0]) == E_STATE
        assert _bytes(cv) == before and cv.frames() == [0]
        cv.clear()
        _put(cv, orc, {0: "d0.01"})
        _check(cv, K.reference(orc, {0: "d0.01"}, p, 1, kind, vals={0: G.apply(l["norm"], col)}, tag="col"), "after clear")
        # a table of another M than a listed frame's: DSSS_E_ARG before the staleness is looked at
        assert _code(_put, cv, orc, {1: "own"}) == E_ARG
        clean.mosaic_gain_set(None)
        assert _code(_put, cv, orc, {1: "own"}) == E_STATE
    finally:
        cv.close()


# ---------------------------------------------------------------- stale frame
@pytest.mark.parametrize("kind,move", MODES)
def test_stale_frame(clean, orc, kind, move):
    l = K.legs(orc)[0]
    p = K.grid(orc, 1)
    cv = _canvas(clean, p, kind, move)
    try:
        _put(cv, orc, {0: "own", 1: "own"})
        before = _bytes(cv)
        clean.frame_set(0, l["raw"], l["N"], l["M"], l["pose"], l["alt"], l["gr"])      # set again: its images are gone
        assert _code(_put, cv, orc, {0: "d0.01"}) == E_STATE and _code(cv.remove, [0]) == E_STATE
        clean.extract(0)                                                           # extracted again: the same images, but the canvas cannot know
        assert _code(_put, cv, orc, {0: "d0.01"}) == E_STATE and _code(_put, cv, orc, {0: "own"}) == E_STATE and _code(cv.remove, [0, 1]) == E_STATE
        assert _bytes(cv) == before and cv.frames() == [0, 1]
        cv.remove([1])                                                             # the other frame is not stale
        cv.clear()
        assert cv.frames() == [] and cv.dirty() == (0, 0, p.W, p.H)
        _put(cv, orc, {0: "d0.01"})
        _check(cv, K.reference(orc, {0: "d0.01"}, p, 1, kind), "after clear")
    finally:
        cv.close()


# ---------------------------------------------------------------- windows
@pytest.mark.parametrize("kind,move", MODES)
def test_windows(clean, orc, kind, move):
    """T2 on its grown grid without the mask: sub-samples of the footprint canvases fall outside the frame's point window"""
    p = K.t2_grid(orc, 0)
    cv = _canvas(clean, p, kind, move)
    try:
        w_t1, w_d = K.frame_window(orc, 2, "t1", p, kind), K.frame_window(orc, 2, "d0.3", p, kind)
        assert cv.frame_window(2, K.rows_of(orc, 2, "t1")) == w_t1 and cv.frame_window(2, K.rows_of(orc, 2, "d0.3")) == w_d
        assert w_t1[2] < p.W and w_t1[3] < p.H
        empty = [a.copy() for a in cv.read()]
        info = _put(cv, orc, {2: "t1"})
        assert tuple(info.win) == w_t1 == cv.frame_window(2) == cv.dirty(reset=False)
        full = cv.read()
        _check(cv, K.reference(orc, {2: "t1"}, p, 0, kind), "T2")
        assert K.outside(sum((a != b) for a, b in zip(full, empty)), w_t1).sum() == 0 and (full[1] != empty[1]).any()
        assert cv.dirty() == w_t1 and cv.dirty() is None                          # the reset works
        info = _put(cv, orc, {2: "d0.3"})
        both = K.union(w_t1, w_d)
        assert tuple(info.win) == both == cv.dirty(reset=False) and cv.frame_window(2) == w_d
        moved = cv.read()
        _check(cv, K.reference(orc, {2: "d0.3"}, p, 0, kind), "T2 moved")
        assert K.outside(sum((a != b) for a, b in zip(moved, full)), both).sum() == 0
        for win in (both, w_d, (both[0] + 3, both[1] + 5, 17, 1), (0, 0, 1, 1), (p.W - 2, p.H - 3, 2, 3)):
            part = cv.read(win)
            for a, b in zip(part, moved):
                assert a.shape == (win[3], win[2]) and a.tobytes() == np.ascontiguousarray(b[win[1]:win[1] + win[3], win[0]:win[0] + win[2]]).tobytes()
        s, c, i = cv.read(both, want=("cnt",))
        assert s is None and i is None and c.tobytes() == cv.read(both)[1].tobytes()
        cv.remove([2])
        assert cv.dirty() == both and not any(x.any() for x in cv.read())
    finally:
        cv.close()


# ---------------------------------------------------------------- capacity
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


@pytest.mark.parametrize("kind,move", [("point", 0), ("point", 1), ("fp4", 0)])
def test_capacity_undoes_the_call(big, orc, kind, move):
    from diasss_amd import capi
    l = K.legs(orc)[0]
    one = capi.MosaicParams(-5000.0, -5000.0, 10000.0, 1, 1, 0, 0)
    cv = big.canvas(one, footprint=K.KINDS[kind], move=move)
    try:
        cv.put([0])
        before = cv.read()
        # every sample of leg 0 lies in the one cell, once: a step of centimetres on a cell of 10 km has one sub-sample
        assert int(before[1][0, 0]) == l["N"] * l["M"] and int(before[0][0, 0]) == int(l["norm"].sum(dtype=np.int64))
        assert _code(cv.put, [1]) == E_CAPACITY
        assert _bytes(cv) == b"".join(a.tobytes() for a in before) and cv.frames() == [0]
        assert _code(cv.put, [0, 1], rpy6=np.concatenate([K.rows_of(orc, 0, "d0.3"), np.zeros((4200, 6))]), ping_off=np.array([0, l["N"]], np.int32)) == E_CAPACITY
        assert _bytes(cv) == b"".join(a.tobytes() for a in before) and cv.frames() == [0]
        assert cv.rows(0, l["N"]).tobytes() == K.rows_of(orc, 0, "own").tobytes()
        cv.remove([0])
        assert not any(x.any() for x in cv.read())
    finally:
        cv.close()


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("kind,move", MODES)
def test_refusals_leave_the_bytes(clean, orc, kind, move):
    from diasss_amd import capi
    p = K.grid(orc, 1)
    dp = _dev_params(p)
    cv = _canvas(clean, p, kind, move)
    try:
        _put(cv, orc, {0: "own"})
        before = _bytes(cv)
        t1 = K.rows_of(orc, 0, "t1")
        zero = np.zeros(1, np.int32)
        calls = [
            (E_ARG, lambda: cv.put([])),
            (E_ARG, lambda: cv.put([0, 4])),
            (E_ARG, lambda: cv.put([-1])),
            (E_ARG, lambda: cv.put([1, 1])),
            (E_ARG, lambda: cv.put([0], rpy6=t1)),                                  # a trajectory without ping_off
            (E_ARG, lambda: cv.put([0], rpy6=t1, ping_off=np.array([-1], np.int32))),
            (E_STATE, lambda: cv.put([1, 3])),                                      # set, never extracted: nothing of the call happens
            (E_STATE, lambda: cv.put([3, 0], rpy6=np.concatenate([t1, t1]), ping_off=np.array([0, len(t1)], np.int32))),
            (E_ARG, lambda: cv.remove([])),
            (E_ARG, lambda: cv.remove([1])),                                        # not on the canvas
            (E_ARG, lambda: cv.remove([0, 1])),                                     # all or nothing
            (E_ARG, lambda: cv.remove([0, 0])),
            (E_ARG, lambda: cv.remove([9])),
            (E_ARG, lambda: cv.read((-1, 0, 4, 4))),
            (E_ARG, lambda: cv.read((0, 0, p.W + 1, 1))),
            (E_ARG, lambda: cv.read((p.W - 1, p.H - 1, 2, 1))),
            (E_ARG, lambda: cv.read((0, 0, 0, 4))),
            (E_ARG, lambda: cv.read((0, 5, 4, p.H - 4))),
            (E_ARG, lambda: cv.rows(1, 8)),
            (E_ARG, lambda: cv.frame_window(1)),                                    # not on the canvas and no rows
            (E_ARG, lambda: cv.frame_window(4, t1)),
        ]
        for k, (code, call) in enumerate(calls):
            assert _code(call) == code, "refusal %d" % k
            assert _bytes(cv) == before and cv.frames() == [0], "refusal %d" % k
        assert cv.rows(0, _N(orc, 0)).tobytes() == K.rows_of(orc, 0, "own").tobytes()
        # room for fewer ids than there are frames: the count comes back with DSSS_E_CAPACITY
        n = C.c_int(-1)
        one = np.zeros(1, np.int32)
        _put(cv, orc, {1: "own"})
        assert cv.L.dsss_canvas_frames(cv.h, capi._ptr(one), 1, C.byref(n)) == E_CAPACITY and n.value == 2
        assert cv.L.dsss_canvas_frames(cv.h, capi._ptr(one), 1, None) == E_ARG
        # NULL handles and outputs
        L = clean.L
        assert L.dsss_canvas_put(None, capi._ptr(zero), 1, None, None, None) == E_ARG and L.dsss_canvas_remove(None, capi._ptr(zero), 1) == E_ARG
        assert L.dsss_canvas_clear(None) == E_ARG and L.dsss_canvas_destroy(None) == E_ARG and L.dsss_canvas_read(None, None, None, None, None) == E_ARG
        assert L.dsss_canvas_dirty(cv.h, None, 0) == E_ARG and L.dsss_canvas_rows(cv.h, 0, None) == E_ARG and L.dsss_canvas_frame_window(cv.h, 0, None, None) == E_ARG
        assert L.dsss_canvas_read(cv.h, None, None, None, None) == 0               # no output: accepted
        assert L.dsss_canvas_put(cv.h, capi._ptr(zero), 1, None, None, None) == 0   # no info: accepted (a skip)
        # creation
        h = C.c_void_p()
        assert L.dsss_canvas_create(None, C.byref(dp), None, C.byref(h)) == E_ARG and L.dsss_canvas_create(clean.h, C.byref(dp), None, None) == E_ARG
        assert L.dsss_canvas_create(clean.h, None, None, C.byref(h)) == E_ARG
        assert _code(clean.canvas, dp, move=2) == E_ARG and _code(clean.canvas, dp, move=-1) == E_ARG
        for fp in ((0, 1.0), (9, 1.0), (4, 0.0), (4, float("nan")), (4, float("inf"))):
            assert _code(clean.canvas, dp, footprint=fp) == E_ARG
        for bad in (capi.MosaicParams(0.0, 0.0, 0.0, 4, 4, 1, 0), capi.MosaicParams(0.0, 0.0, 0.1, 0, 4, 1, 0), capi.MosaicParams(0.0, 0.0, 0.1, 1 << 15, (1 << 13) + 1, 1, 0)):
            assert _code(clean.canvas, bad) == E_ARG
        assert L.dsss_canvas_create(clean.h, C.byref(dp), None, C.byref(h)) == 0   # NULL parameters: a point canvas
        assert L.dsss_canvas_put(h, capi._ptr(zero), 1, None, None, None) == 0
        out = [np.empty((p.H, p.W), t) for t in (np.uint32, np.uint32, np.uint8)]
        assert L.dsss_canvas_read(h, None, *[capi._ptr(a) for a in out]) == 0 and L.dsss_canvas_destroy(h) == 0
        assert b"".join(a.tobytes() for a in out) == _fresh(clean, p, "point", {0: "own"}, orc)
        _check(cv, K.reference(orc, {0: "own", 1: "own"}, p, 1, kind), "after the refusals")
    finally:
        cv.close()


# ---------------------------------------------------------------- independence
@pytest.mark.parametrize("move", MOVES)
def test_two_canvases_on_one_context(clean, orc, move):
    p, q = K.grid(orc, 1), K.grid(orc, 0)
    a, b = _canvas(clean, p, "point", move), _canvas(clean, q, "fp4", move)
    try:
        _put(a, orc, {0: "own"}); _put(b, orc, {1: "own", 0: "t1"})
        clean.mosaic_render_footprint([0, 1], _dev_params(q))                      # another mosaic entry between the calls: it reuses the scratch
        _put(a, orc, {0: "d0.01", 1: "own"}); b.remove([0])
        clean.mosaic_consistency([0, 1], _dev_params(p))
        _put(b, orc, {0: "d0.3"}); a.remove([1])
        _check(a, K.reference(orc, {0: "d0.01"}, p, 1, "point"), "the point canvas")
        _check(b, K.reference(orc, {0: "d0.3", 1: "own"}, q, 0, "fp4"), "the footprint canvas")
        a.clear()
        assert a.frames() == [] and b.frames() == [0, 1]
        _check(b, K.reference(orc, {0: "d0.3", 1: "own"}, q, 0, "fp4"), "the footprint canvas after the other was cleared")
    finally:
        a.close(); b.close()
    # a context closes the canvases that are left
    from diasss_amd import capi
    c = capi.Context(max_frames=1)
    left = c.canvas(_dev_params(p))
    c.close()
    assert left.h is None
    left.close()


# ---------------------------------------------------------------- behind a busy stream and in flight
SCRIPT = K.MIXED_B + [("remove", [2]), ("put", {0: "t1", 1: "own"}), ("remove", [1]), ("clear",), ("put", {1: "own", 0: "d0.003"})]
SPIN_MS = 2.0


class _Held:
    """a canvas's library handle that queues a bounded spin on the context's stream before every dsss_canvas_* call"""

    def __init__(self, L, h, cycles, busy):
        import torch
        self._L, self._cycles, self._busy, self._torch = L, cycles, busy, torch
        self._stream = torch.cuda.ExternalStream(L.dsss_stream(h))

    def __getattr__(self, name):
        fn = getattr(self._L, name)
        if not name.startswith("dsss_canvas_"):
            return fn
        torch = self._torch

        def call(*args):
            with torch.cuda.stream(self._stream):
                torch.cuda._sleep(self._cycles)
            ev = torch.cuda.Event()
            ev.record(self._stream)
            self._busy.append(not ev.query())
            return fn(*args)
        return call


def _script_bytes(c, orc, kind, move, cycles=None, busy=None):
    p = K.grid(orc, 1)
    cv = _canvas(c, p, kind, move)
    try:
        if cycles is not None:
            cv.L = _Held(c.L, c.h, cycles, busy)
        out = []
        for step in SCRIPT:
            _play(cv, orc, [step])
            out.append(_bytes(cv) + np.array(cv.frames(), np.int32).tobytes())
        return out
    finally:
        cv.L = c.L
        cv.close()


@pytest.fixture(scope="module")
def spin_cycles():
    import torch
    from diasss_amd import capi
    c = capi.Context(max_frames=1)
    try:
        st = torch.cuda.ExternalStream(c.L.dsss_stream(c.h))

        def ms(cycles):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(st):
                e0.record(st); torch.cuda._sleep(cycles); e1.record(st)
            e1.synchronize()
            return e0.elapsed_time(e1)
        probe = 1_000_000
        ms(probe)
        per_cycle = min(ms(probe) for _ in range(3)) / probe
        cycles = max(1, min(int(SPIN_MS / per_cycle), 50 * probe))
    finally:
        c.close()
    return cycles


@pytest.mark.parametrize("kind,move", MODES)
def test_behind_a_busy_stream(clean, orc, spin_cycles, kind, move):
    idle = _script_bytes(clean, orc, kind, move)
    p = K.grid(orc, 1)
    assert idle[-1][:-8] == b"".join(r.astype(t).tobytes() for r, t in zip(K.reference(orc, K.final_state(SCRIPT), p, 1, kind)[:3], (np.uint32, np.uint32, np.uint8)))
    busy = []
    held = _script_bytes(clean, orc, kind, move, spin_cycles, busy)
    assert len(busy) >= 2 * len(SCRIPT) and all(busy), "calls entered with the spin in front of them already over: %d of %d" % (busy.count(False), len(busy))
    assert held == idle


@pytest.mark.parametrize("kind,move", [("point", 0), ("fp4", 1)])
def test_two_contexts_in_flight(clean, orc, kind, move):
    from diasss_amd import capi
    idle = _script_bytes(clean, orc, kind, move)
    K.rows_of(orc, 0, "t1"); K.legs(orc)                                           # the caches are filled before the threads read them
    barrier = threading.Barrier(2)
    got, failed = [None, None], [None, None]

    def work(k):
        try:
            c = capi.Context(max_frames=3)
            try:
                _load(c, orc)
                barrier.wait(timeout=60)
                got[k] = [_script_bytes(c, orc, kind, move) for _ in range(2)]
            finally:
                c.close()
        except BaseException as ex:                                                # carried to the test and raised there
            failed[k] = ex

    threads = [threading.Thread(target=work, args=(k,), name="canvas-in-flight-%d" % k, daemon=True) for k in range(2)]
    t0 = time.perf_counter()
    for t in threads:
        t.start()
    for t in threads:
        t.join(max(0.0, 60.0 - (time.perf_counter() - t0)))
    for t in threads:
        if t.is_alive():
            _HUNG.append(t.name)
    assert not _HUNG, "threads that did not come back: %s" % _HUNG
    for ex in failed:
        if ex is not None:
            raise ex
    for k in range(2):
        assert got[k] == [idle, idle], "thread %d differs from the idle context's bytes" % k


# ---------------------------------------------------------------- the table of driven entries
def test_every_driven_entry_is_called(clean, orc):
    """one short life of a canvas through a counting handle: every entry of DRIVEN is reached from this file's helpers"""
    import collections
    from diasss_amd import capi
    counts = collections.Counter()

    class Counting:
        def __init__(self, L):
            self._L = L

        def __getattr__(self, name):
            fn = getattr(self._L, name)
            if name.startswith("dsss_canvas_"):
                def call(*a):
                    counts[name] += 1
                    return fn(*a)
                return call
            return fn

    plain = clean.L
    real = capi._LIB
    clean.L = Counting(plain); capi._LIB = Counting(real)
    try:
        p = K.grid(orc, 1)
        cv = _canvas(clean, p, "point", 0)
        _play(cv, orc, K.MIXED_A + [("remove", [2]), ("clear",)])
        cv.read(); cv.dirty(); cv.frames(); _put(cv, orc, {0: "own"}); cv.rows(0, _N(orc, 0)); cv.frame_window(0)
        cv.close()
    finally:
        clean.L = plain; capi._LIB = real
    assert sorted(counts) == sorted(DRIVEN), "never called: %s" % sorted(set(DRIVEN) - set(counts))

"""Peaks on the device: mosaic_peak_kernel through dsss_mosaic_register_peaks on the case table of tests/register_peaks_ref.py (every
record equal to the reference byte for byte, from host and from device memory), the argument rules, and the four registration
entries on their device path (no sums asked for) against their host path (sums asked for, or DSSS_REG_PEAKS=host) and against the
numpy references, as bytes, with what dsss_mosaic_register_info says each call did.

tests/test_register_peaks_cpu.py proves the preconditions: the host entry equals the reference on the same table, and the table reaches
every branch of the rule.  Frames, grid and helpers are those of tests/test_gpu_register_segments.py; the fan's and the pyramid's
special rows come from the constructions of tests/test_gpu_register_yaw.py and tests/test_gpu_register_pyr.py."""
import ctypes as C
import os
import numpy as np
import pytest

from tests import mosaic_register_ref as R
from tests import register_edges_ref as E
from tests import register_peaks_ref as P
from tests import register_pyr_ref as PY
from tests import register_yaw_ref as Y
import tests.test_gpu_register_pyr as TP
import tests.test_gpu_register_segments as TS
import tests.test_gpu_register_yaw as TY

pytestmark = pytest.mark.gpu

E_ARG, E_CAPACITY = -2, -5
N = TS.N
RADIUS, MIN_CELLS, CELL = 8, 256, 0.1
NYAW, STEP, LEVELS, REFINE = 5, 0.01, 3, 3
REC = P.REC_BYTES


@pytest.fixture(scope="module")
def data(orc):
    """the frames of tests/test_gpu_register_segments.py"""
    from diasss_amd.synth import Survey
    from tests import helpers as H
    sv = Survey(2, N, TS.M, seed=7)
    fr = []
    for f in range(2):
        raw = sv.frame(f).numpy().copy()
        pose, alt, gr = sv.inputs(f)
        fr.append(dict(N=N, M=TS.M, raw=raw, pose=np.ascontiguousarray(pose), alt=alt, gr=gr, true=np.ascontiguousarray(sv.poses_true[f]),
                       norm=orc.normalize(raw), mask=orc.mask(raw)))
    pose, alt, gr = H.track(TS.N2, TS.M2, 1, seed=9)
    raw = np.random.default_rng(1).rayleigh(1.0, (TS.N2, TS.M2)) * 100.0
    fr.append(dict(N=TS.N2, M=TS.M2, raw=raw, pose=pose, alt=alt, gr=gr, true=np.ascontiguousarray(pose), norm=orc.normalize(raw), mask=orc.mask(raw)))
    return fr


@pytest.fixture(scope="module")
def ctx(data):
    from diasss_amd import capi
    c = capi.Context(max_frames=4)
    for i, L in enumerate(data):
        c.frame_set(i, L["raw"], L["N"], L["M"], L["pose"], L["alt"], L["gr"])
    c.extract_many([0, 1, 2])
    yield c
    c.close()


def _info(ctx):
    i = ctx.mosaic_register_info()
    return (int(i.tables_device), int(i.tables_host), int(i.bytes_down), int(i.syncs))


class _host_peaks:
    """DSSS_REG_PEAKS=host around a call: the switch is read once per call"""
    def __enter__(self):
        os.environ["DSSS_REG_PEAKS"] = "host"

    def __exit__(self, *a):
        del os.environ["DSSS_REG_PEAKS"]


# ---------------------------------------------------------------- 1. the case table
@pytest.mark.parametrize("radius", P.RADII)
def test_case_table_from_host_and_device_memory(ctx, radius):
    import torch
    from diasss_amd import capi
    names, sums, ref, traces, blob = P.case_table(radius)
    nt = len(names)
    out = np.zeros(nt, capi.REG_DTYPE)
    ctx.mosaic_register_peaks(sums, radius, P.MIN_CELLS, P.CELL, out=out)
    got = out.tobytes()
    for k, name in enumerate(names):
        assert got[k * REC:(k + 1) * REC] == blob[k * REC:(k + 1) * REC], "radius %d, table %r: device %s, reference %s" % (radius, name, out[k], ref[k])
    assert _info(ctx) == (nt, 0, 64 * nt, 1)
    # the records do not depend on what the output array held before
    dirty = np.frombuffer(np.random.default_rng(radius).bytes(nt * REC), capi.REG_DTYPE).copy()
    ctx.mosaic_register_peaks(sums, radius, P.MIN_CELLS, P.CELL, out=dirty)
    assert dirty.tobytes() == blob
    # from device memory: the same bytes
    dsums = torch.from_numpy(sums.astype(np.int64)).cuda()
    dev = ctx.mosaic_register_peaks(dsums, radius, P.MIN_CELLS, P.CELL, ntables=nt)
    assert dev.tobytes() == blob and _info(ctx) == (nt, 0, 64 * nt, 1)
    # 1 table, and 5: a partial last workgroup; the array behind them stays as it was
    for n in (1, 5):
        out = np.frombuffer(b"\xa5" * (8 * REC), capi.REG_DTYPE).copy()
        ctx.mosaic_register_peaks(sums[:n], radius, P.MIN_CELLS, P.CELL, out=out)
        assert out.tobytes() == blob[:n * REC] + b"\xa5" * ((8 - n) * REC)
        assert ctx.mosaic_register_peaks(dsums, radius, P.MIN_CELLS, P.CELL, ntables=n).tobytes() == blob[:n * REC]
    # another min_cells and cell reach the kernel: the host entry's records under them
    few = ctx.mosaic_register_peaks(sums, radius, 1, 0.37)
    for k in range(nt):
        rec = capi.mosaic_register_peak(sums[k], radius, 1, 0.37)
        assert few[k].tobytes() == C.string_at(C.addressof(rec), REC), (radius, names[k])


def test_no_tables_and_ten_thousand(ctx):
    from diasss_amd import capi
    names, sums, ref, traces, blob = P.case_table(1)
    ctx.mosaic_register_peaks(sums, 1, P.MIN_CELLS, P.CELL)
    assert _info(ctx)[0] == len(names)
    out = np.frombuffer(b"\x5a" * (2 * REC), capi.REG_DTYPE).copy()
    ctx.mosaic_register_peaks(np.zeros((0, 3, 3, 6), np.uint64), 1, P.MIN_CELLS, P.CELL, out=out)
    assert out.tobytes() == b"\x5a" * (2 * REC) and _info(ctx) == (0, 0, 0, 0)                  # valid, nothing launched, nothing written
    assert ctx.L.dsss_mosaic_register_peaks(ctx.h, None, 0, 1, P.MIN_CELLS, C.c_double(P.CELL), None) == 0
    nt = 10007                                                                                  # 2502 workgroups, the last with three tables
    idx = np.arange(nt) % len(names)
    big = np.ascontiguousarray(sums[idx])
    got = ctx.mosaic_register_peaks(big, 1, P.MIN_CELLS, P.CELL).tobytes()
    want = b"".join(blob[k * REC:(k + 1) * REC] for k in idx)
    assert got == want and _info(ctx) == (nt, 0, 64 * nt, 1)


# ---------------------------------------------------------------- 2. argument rules
def test_argument_rules(ctx):
    from diasss_amd import capi
    names, sums, ref, traces, blob = P.case_table(1)
    nt = len(names)
    ctx.mosaic_register_peaks(sums, 1, P.MIN_CELLS, P.CELL)
    before = _info(ctx)
    assert before == (nt, 0, 64 * nt, 1)
    out = np.frombuffer(b"\x3c" * (nt * REC), capi.REG_DTYPE).copy()
    f = ctx.L.dsss_mosaic_register_peaks
    s, o, cell = capi._ptr(sums), capi._ptr(out), C.c_double(P.CELL)
    bad = [(None, nt, 1, P.MIN_CELLS, cell, o), (s, nt, 1, P.MIN_CELLS, cell, None), (s, -1, 1, P.MIN_CELLS, cell, o), (s, nt, -1, P.MIN_CELLS, cell, o),
           (s, nt, 17, P.MIN_CELLS, cell, o), (s, nt, 1, 0, cell, o), (s, nt, 1, -3, cell, o), (s, nt, 1, P.MIN_CELLS, C.c_double(0.0), o),
           (s, nt, 1, P.MIN_CELLS, C.c_double(-0.1), o), (s, nt, 1, P.MIN_CELLS, C.c_double(float("inf")), o), (s, nt, 1, P.MIN_CELLS, C.c_double(float("nan")), o)]
    for args in bad:
        assert f(ctx.h, *args) == E_ARG, args[1:5]
        assert _info(ctx) == before and out.tobytes() == b"\x3c" * (nt * REC)
    assert f(None, s, nt, 1, P.MIN_CELLS, cell, o) == E_ARG
    assert ctx.L.dsss_mosaic_register_info(ctx.h, None) == E_ARG and ctx.L.dsss_mosaic_register_info(None, C.byref(capi.RegCallInfo())) == E_ARG
    fresh = capi.Context(max_frames=1)
    try:
        assert _info(fresh) == (0, 0, 0, 0)                              # zeros before any such call
    finally:
        fresh.close()


# ---------------------------------------------------------------- 3. the four entries
@pytest.fixture(scope="module")
def trajectories(data):
    return {"true": [data[0]["true"], data[1]["true"]], "drifted": [data[0]["pose"], E.drift(data[1]["pose"])]}


def _three_ways(call):
    """the rows without sums, with sums, and under DSSS_REG_PEAKS=host: (rows, info) each, and the sums"""
    dev = call(want_sums=False); idev = _info(call.ctx)
    (hst, sums) = call(want_sums=True); ihst = _info(call.ctx)
    with _host_peaks():
        sw = call(want_sums=False)
    isw = _info(call.ctx)
    again = call(want_sums=False)                                       # the switch is read per call: unset again, the device path
    assert _info(call.ctx) == idev and again.tobytes() == dev.tobytes()
    assert dev.tobytes() == hst.tobytes(), "device path and host path (sums asked for) differ"
    assert dev.tobytes() == sw.tobytes(), "device path and host path (DSSS_REG_PEAKS=host) differ"
    assert ihst == isw
    return dev, hst, sums, idev, ihst


class _call:
    def __init__(self, ctx, fn, *a, **kw):
        self.ctx, self.fn, self.a, self.kw = ctx, fn, a, kw

    def __call__(self, want_sums):
        return self.fn(*self.a, want_sums=want_sums, **self.kw)


def _bounds(idev, ihst, tables, rows, syncs, host_bytes):
    print("device path %s, host path %s" % (idev, ihst))
    assert idev[1] == 0 and idev[0] == tables and idev[2] <= 64 * idev[0] + 24 * rows + 64 * idev[3] and 1 <= idev[3] <= syncs
    assert ihst[0] == 0 and ihst[1] == tables and ihst[2] >= host_bytes and 1 <= ihst[3] <= syncs


CASES = [(t, s, m) for t in ("true", "drifted") for s in (80, 96) for m in (0, 1)]


@pytest.mark.parametrize("traj,seg_pings,use_mask", CASES)
def test_segments(ctx, orc, data, trajectories, traj, seg_pings, use_mask):
    rows = trajectories[traj]
    p = TS._grid(orc, data, [0, 1], rows, CELL, use_mask)
    rpy, off = TS._traj(rows)
    pairs = [(0, 1), (1, 0)]
    dev, hst, sums, idev, ihst = _three_ways(_call(ctx, ctx.mosaic_register_segments, [0, 1], p, pairs, seg_pings, reg=TS._reg(), rpy6=rpy, ping_off=off))
    k = 0
    for i, pr in enumerate(pairs):
        k = TS._same_rows(dev, sums, k, i, TS._ref_pair(orc, data, [0, 1], rows, p, pr, seg_pings))
    assert k == len(dev) and (dev["r"]["zncc"] > -2.0).sum() >= len(dev) // 2
    _bounds(idev, ihst, len(dev), len(dev), 2, 48 * 17 * 17 * len(dev))


@pytest.mark.parametrize("traj,use_mask", [(t, m) for t in ("true", "drifted") for m in (0, 1)])
@pytest.mark.parametrize("three", [False, True])
def test_whole_pairs(ctx, orc, data, trajectories, traj, use_mask, three):
    """dsss_mosaic_register has no segments: the two legs at cell 0.1, and (three) the pairs with frame 2 at cell 0.5"""
    rows = trajectories[traj] + [data[2]["true"]]
    frames = [0, 1, 2]
    p = TS._grid(orc, data, frames, rows, 0.5 if three else CELL, use_mask)
    rpy, off = TS._traj(rows)
    pairs = [(0, 2), (2, 1), (1, 0)] if three else [(0, 1), (1, 0)]
    dev, hst, sums, idev, ihst = _three_ways(_call(ctx, ctx.mosaic_register, frames, p, pairs, reg=TS._reg(), rpy6=rpy, ping_off=off))
    lay = {}
    for f, r in zip(frames, rows):
        g = orc.geo_img(np.ascontiguousarray(r), data[f]["gr"], data[f]["M"])
        lay[f] = R.mean_layer(g[0], g[1], data[f]["norm"], data[f]["mask"], p, p.use_mask)
    for k, (a, b) in enumerate(pairs):
        ref = R.shift_sums(lay[a][0], lay[a][1], lay[b][0], lay[b][1], RADIUS)
        assert (sums[k].astype(np.int64) == ref).all()
        assert R.same_result(dev[k], R.peak(ref, RADIUS, MIN_CELLS, p.cell)), "pair %d" % k
    assert (dev["zncc"] > -2.0).any()
    _bounds(idev, ihst, len(pairs), len(pairs), 2, 48 * 17 * 17 * len(pairs))
    assert idev[3] == 1 and idev[2] == 64 * len(pairs) + 8


@pytest.mark.parametrize("traj,seg_pings,use_mask", CASES)
def test_fan(ctx, orc, data, trajectories, traj, seg_pings, use_mask):
    from diasss_amd import capi
    rows = trajectories[traj]
    p = TS._grid(orc, data, [0, 1], rows, CELL, use_mask)
    rpy, off = TS._traj(rows)
    pairs = [(0, 1)]
    dev, hst, sums, idev, ihst = _three_ways(_call(ctx, ctx.mosaic_register_segments_yaw, [0, 1], p, pairs, seg_pings, yaw=capi.RegYawParams(NYAW, 0, STEP),
                                                   reg=TS._reg(), rpy6=rpy, ping_off=off))
    k = TY._same_rows(dev, sums, 0, 0, TY._ref_pair(orc, data, [0, 1], rows, p, pairs[0], seg_pings, NYAW, STEP))
    assert k == len(dev) and (dev["s"]["r"]["zncc"] > -2.0).sum() >= len(dev) // 2
    _bounds(idev, ihst, len(dev) * NYAW, len(dev), NYAW + 1, 48 * 17 * 17 * len(dev) * NYAW)


@pytest.mark.parametrize("traj,seg_pings,use_mask", CASES)
def test_pyramid(ctx, orc, data, trajectories, traj, seg_pings, use_mask):
    from diasss_amd import capi
    rows = trajectories[traj]
    p = TS._grid(orc, data, [0, 1], rows, CELL, use_mask)
    rpy, off = TS._traj(rows)
    pairs = [(0, 1)]
    dev, hst, sums, idev, ihst = _three_ways(_call(ctx, ctx.mosaic_register_segments_pyr, [0, 1], p, pairs, seg_pings, pyr=capi.RegPyrParams(LEVELS, REFINE),
                                                   reg=TS._reg(), rpy6=rpy, ping_off=off))
    ref = TP._ref_pair(orc, data, [0, 1], rows, p, pairs[0], seg_pings, LEVELS, REFINE, RADIUS, MIN_CELLS)
    assert TP._same_rows(dev, sums, 0, 0, ref) == len(dev) and (dev["level"] == 0).sum() >= len(dev) // 2
    # the rows alive per level, from the reference: all at the top, below it those that had a usable peak one level up
    alive = [len(ref)] + [sum(r["lz"][l + 1] > -2.0 for r in ref) for l in range(LEVELS - 2, -1, -1)]
    host_bytes = 48 * (17 * 17 * alive[0] + 7 * 7 * sum(alive[1:]))
    _bounds(idev, ihst, sum(alive), len(dev), LEVELS + 1, host_bytes)


@pytest.mark.parametrize("entry", ["pair", "segments", "fan", "pyramid"])
def test_call_accounting_is_exact(ctx, orc, data, trajectories, entry):
    """what _bounds holds to inequalities, as equalities: a call is a number of passes (one correlation launch and its fetch: one for the
    pair and the flat entry, one per angle, one per level) and, where a row has a peak to take a centroid at, one centroid download.
    A pass brings down the 8 bytes of the sample-limit flag and n_l records of 64 bytes (device path) or n_l tables (host path)."""
    from diasss_amd import capi
    radius, nyaw, levels = min(r for r in P.RADII if r > 0), 3, 3
    rows = trajectories["true"]
    p = TS._grid(orc, data, [0, 1], rows, CELL, 0)
    rpy, off = TS._traj(rows)
    kw = dict(reg=TS._reg(radius=radius), rpy6=rpy, ping_off=off)
    fn, a = {"pair": (ctx.mosaic_register, ()), "segments": (ctx.mosaic_register_segments, (80,)),
             "fan": (ctx.mosaic_register_segments_yaw, (80, capi.RegYawParams(nyaw, 0, STEP))),
             "pyramid": (ctx.mosaic_register_segments_pyr, (80, capi.RegPyrParams(levels, REFINE)))}[entry]
    dev = fn([0, 1], p, [(0, 1)], *a, **kw); idev = _info(ctx)
    hst, sums = fn([0, 1], p, [(0, 1)], *a, want_sums=True, **kw); ihst = _info(ctx)
    assert dev.tobytes() == hst.tobytes()
    n, top = len(dev), 48 * (2 * radius + 1) ** 2                      # rows (pairs for the pair entry), bytes of a table of the full radius
    if entry == "pair":
        assert n == 1
        n_dev = n_host = [n]; tab = [top]; cen = False
    elif entry == "segments":
        assert n == N // 80
        n_dev = n_host = [n]; tab = [top]; cen = bool((dev["r"]["zncc"] > -2.0).any())
    elif entry == "fan":
        assert n == N // 80
        n_dev = n_host = [n] * nyaw; tab = [top] * nyaw; cen = bool((dev["s"]["r"]["zncc"] > -2.0).any())
    else:
        assert n == N // 80
        n_dev = [n] + [int((dev["lz"][:, l + 1] > -2.0).sum()) for l in range(levels - 2, -1, -1)]      # alive: all at the top, below it those with a peak one level up
        n_host = [n] * levels; tab = [top] + [48 * (2 * REFINE + 1) ** 2] * (levels - 1); cen = bool((dev["level"] == 0).any())
    decided, syncs, cen_bytes = sum(n_dev), len(n_dev) + (1 if cen else 0), 24 * n if cen else 0
    print("%s: device path %s, host path %s, tables per pass %s, centroid %s" % (entry, idev, ihst, n_dev, cen))
    assert cen == (entry != "pair")                                     # the true trajectory: rows with a peak, so the centroid term is exercised
    assert idev == (decided, 0, sum(8 + 64 * k for k in n_dev) + cen_bytes, syncs)
    assert ihst == (0, decided, sum(8 + k * t for k, t in zip(n_host, tab)) + cen_bytes, syncs)


# ---------------------------------------------------------------- 4. cases that must survive the routing
def test_no_overlap_and_segments_off_the_grid(ctx, orc, data, trajectories):
    """a zero table gives the no-usable-shift record: frame 2 moved 300 m aside (windows on the grid, none within the radius), and the
    grid cropped to its middle third (segments without a window)"""
    from diasss_amd import capi
    far = [data[0]["true"], data[2]["true"] + np.array([0, 0, 0, 0, 300.0, 0])]
    wide = TS._grid(orc, data, [0, 2], far, 0.5, 0)
    rpy, off = TS._traj(far)
    pairs = [(0, 2), (2, 0)]
    zero = P.record_bytes(P.peak(np.zeros((17, 17, 6), np.uint64), RADIUS, MIN_CELLS, wide.cell)[0])
    kw = dict(reg=TS._reg(), rpy6=rpy, ping_off=off)
    for fn, a, get in ((ctx.mosaic_register, ([0, 2], wide, pairs), lambda d: d),
                       (ctx.mosaic_register_segments, ([0, 2], wide, pairs, 128), lambda d: d["r"]),
                       (ctx.mosaic_register_segments_yaw, ([0, 2], wide, pairs, 128, capi.RegYawParams(3, 0, STEP)), lambda d: d["s"]["r"]),
                       (ctx.mosaic_register_segments_pyr, ([0, 2], wide, pairs, 128, capi.RegPyrParams(3, 3)), lambda d: d["s"]["r"])):
        dev, hst, sums, idev, ihst = _three_ways(_call(ctx, fn, *a, **kw))
        assert not sums.any() and idev[0] > 0 and idev[1] == 0
        assert np.ascontiguousarray(get(dev)).tobytes() == zero * len(dev)
    full = TS._grid(orc, data, [0, 1], trajectories["drifted"], CELL, 0)
    q = capi.MosaicParams(full.x0 + (full.W // 3) * full.cell, full.y0 + (full.H // 3) * full.cell, full.cell, full.W // 3, full.H // 3, 0, 0)
    rows = trajectories["drifted"]
    rpy, off = TS._traj(rows)
    dev, hst, sums, idev, ihst = _three_ways(_call(ctx, ctx.mosaic_register_segments, [0, 1], q, [(0, 1), (1, 0)], 80, reg=TS._reg(), rpy6=rpy, ping_off=off))
    empty = [k for k in range(len(dev)) if not sums[k].any()]
    assert 4 <= len(empty) < len(dev) and idev[0] == len(dev)
    zero = P.record_bytes(P.peak(np.zeros((17, 17, 6), np.uint64), RADIUS, MIN_CELLS, q.cell)[0])
    assert all(dev[k]["r"].tobytes() == zero for k in empty) and (dev["r"]["zncc"] > -2.0).any()
    k = 0
    for i, pr in enumerate([(0, 1), (1, 0)]):
        k = TS._same_rows(dev, sums, k, i, TS._ref_pair(orc, data, [0, 1], rows, q, pr, 80))


def test_one_frame_as_b_of_two_pairs_and_as_a_and_b(ctx, orc, data, trajectories):
    from diasss_amd import capi
    rows = trajectories["drifted"] + [data[2]["true"]]
    p = TS._grid(orc, data, [0, 1, 2], rows, 0.5, 1)
    rpy, off = TS._traj(rows)
    pairs = [(0, 1), (2, 1), (1, 0)]                                    # frame 1: b of two pairs, and an a
    kw = dict(reg=TS._reg(min_cells=64), rpy6=rpy, ping_off=off)
    dev, hst, sums, idev, ihst = _three_ways(_call(ctx, ctx.mosaic_register_segments, [0, 1, 2], p, pairs, 160, **kw))
    k = 0
    for i, pr in enumerate(pairs):
        k = TS._same_rows(dev, sums, k, i, TS._ref_pair(orc, data, [0, 1, 2], rows, p, pr, 160, min_cells=64))
    assert k == len(dev) == 12 and idev[0] == 12 and (dev["r"]["zncc"] > -2.0).any()
    for fn, extra in ((ctx.mosaic_register_segments_yaw, (capi.RegYawParams(3, 0, STEP),)), (ctx.mosaic_register_segments_pyr, (capi.RegPyrParams(2, 3),))):
        d, h, s, idev, ihst = _three_ways(_call(ctx, fn, [0, 1, 2], p, pairs, 160, *extra, **kw))
        assert len(d) == 12 and idev[1] == 0 and (d["s"]["r"]["zncc"] > -2.0).any()


def test_a_pyramid_row_that_stops_at_a_level(ctx, orc, data):
    """the construction of tests/test_gpu_register_pyr.py::test_a_search_that_stops_on_the_way: its tables are laid out by live rows on
    the device path, so the rows below a stopped one move up"""
    from diasss_amd import capi
    rows = TP._moved(data, PY.MOVE)
    p = TP._grid(orc, data, [0, 1], rows, 1, PY.SEG, use_mask=1)
    rpy, off = TS._traj(rows)
    dev, hst, sums, idev, ihst = _three_ways(_call(ctx, ctx.mosaic_register_segments_pyr, [0, 1], p, [(0, 1)], PY.SEG, pyr=capi.RegPyrParams(3, PY.REFINE),
                                                   reg=capi.RegParams(PY.RADIUS, PY.MIN_CELLS), rpy6=rpy, ping_off=off))
    ref = TP._ref_pair(orc, data, [0, 1], rows, p, (0, 1), PY.SEG, 3)
    assert TP._same_rows(dev, sums, 0, 0, ref) == len(dev)
    levels = [r["level"] for r in ref]
    print("levels %s" % levels)
    assert any(l > 0 for l in levels) and any(l == 0 for l in levels)
    first = min(k for k, l in enumerate(levels) if l != 0)
    assert any(l == 0 for l in levels[first + 1:])                      # a finished row behind a stopped one
    alive = [len(ref)] + [sum(r["lz"][l + 1] > -2.0 for r in ref) for l in (1, 0)]
    assert idev[0] == sum(alive) < 3 * len(ref) and idev[1] == 0 and ihst[1] == sum(alive)


def test_a_fan_row_with_its_best_angle_on_the_border(ctx, orc, data):
    """the turned survey of tests/test_gpu_register_yaw.py under a fan of three: the angle that undoes the turn is the last one"""
    from diasss_amd import capi
    nyaw, step, m = Y.FANS["one_step_up"]
    rows = [data[0]["true"], Y.rotated_survey(orc, data[1]["true"], Y.SEG, m, step, Y.SHIFT, Y.CELL)]
    p = TY._grid(orc, data, [0, 1], rows, Y.CELL, 0)
    rpy, off = TS._traj(rows)
    dev, hst, sums, idev, ihst = _three_ways(_call(ctx, ctx.mosaic_register_segments_yaw, [0, 1], p, [(0, 1)], Y.SEG, yaw=capi.RegYawParams(3, 0, step),
                                                   reg=TS._reg(), rpy6=rpy, ping_off=off))
    ref = TY._ref_pair(orc, data, [0, 1], rows, p, (0, 1), Y.SEG, 3, step)
    assert TY._same_rows(dev, sums, 0, 0, ref) == len(dev)
    print("k %s" % [r["k"] for r in ref])
    assert sum(r["yaw_on_border"] for r in ref) >= 3 and dev["yaw_on_border"].sum() >= 3 and idev[0] == 3 * len(dev)


# ---------------------------------------------------------------- 5. error paths on both paths
def test_row_count_query_on_both_paths(ctx, orc, data, trajectories):
    """cap = 0 asks for the number of rows: the refusal, the count and the untouched info are the same on both paths.  (No existing test
    reaches the 2^24 sample limit of a registration at a small size, so that error is not driven here.)"""
    from diasss_amd import capi
    rows = trajectories["drifted"]
    p = TS._grid(orc, data, [0, 1], rows, 0.5, 0)
    rpy, off = TS._traj(rows)
    pairs = [(0, 1), (1, 0)]
    good = ctx.mosaic_register_segments([0, 1], p, pairs, 80, reg=TS._reg(), rpy6=rpy, ping_off=off)
    before = _info(ctx)
    assert len(good) == 16 and before[0] == 16
    ids = np.array([0, 1], np.int32); pa = np.array([0, 1], np.int32); pb = np.array([1, 0], np.int32)
    seen = []
    for host in (False, True):
        for name, dtype, extra in (("dsss_mosaic_register_segments", capi.REGSEG_DTYPE, ()),
                                   ("dsss_mosaic_register_segments_yaw", capi.REGSEGYAW_DTYPE, (C.byref(capi.RegYawParams(3, 0, STEP)),)),
                                   ("dsss_mosaic_register_segments_pyr", capi.REGSEGPYR_DTYPE, (C.byref(capi.RegPyrParams(3, 3)),))):
            one = np.zeros(1, dtype); n = C.c_int(-1)
            args = (ctx.h, capi._ptr(ids), 2, capi._ptr(rpy), capi._ptr(off), C.byref(p), capi._ptr(pa), capi._ptr(pb), 2, 80, C.byref(TS._reg())) + extra
            if host:
                with _host_peaks():
                    rc = getattr(ctx.L, name)(*args, capi._ptr(one), 0, C.byref(n), None)
            else:
                rc = getattr(ctx.L, name)(*args, capi._ptr(one), 0, C.byref(n), None)
            seen.append((rc, n.value))
            assert not one.tobytes().strip(b"\0")
            assert _info(ctx) == before                                 # a refused call leaves the record of the last good one
    assert len(seen) == 6 and all(s == (E_CAPACITY, 16) for s in seen)
    with pytest.raises(capi.DsssError) as ei:                           # an argument error under the switch, as without it
        with _host_peaks():
            ctx.mosaic_register_segments([0, 1], p, pairs, 0, reg=TS._reg(), rpy6=rpy, ping_off=off)
    assert ei.value.code == E_ARG and "DSSS_REG_PEAKS" not in os.environ
    again = ctx.mosaic_register_segments([0, 1], p, pairs, 80, reg=TS._reg(), rpy6=rpy, ping_off=off)
    assert again.tobytes() == good.tobytes() and _info(ctx) == before

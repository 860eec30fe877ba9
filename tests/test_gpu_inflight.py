"""GPU: every entry held to its idle bytes behind a busy stream (arm A) and beside other contexts in flight (arm B).

The rest of the suite runs one context at a time on an idle GPU, mostly with a synchronisation between one call and the next; a production
step queues the whole hot path with the host far ahead of the device, and bench.py --full runs four contexts on four host threads.  A
copy that is ordered against the host but not against the context's stream gives the right bytes on an idle GPU and the wrong ones once
the stream lags.  The scenarios of tests/inflight_cases.py are run

  idle      on a plain context: the reference bytes (those of pipeline_a and pipeline_b are also held to the oracle, so that agreement
            between two runs is never agreement on a wrong answer; the other scenarios' inputs are held to their references by the tests
            they come from);
  arm A     on a context whose library handle is a proxy that, before every call that takes the context, queues a spin kernel of about
            5 ms on the CONTEXT'S OWN stream: the call is issued with the stream held back, as it is in a production step.  For the calls
            that are asynchronous by contract the event behind the spin must not have fired when the call returns;
  arm B     on several host threads, a context each, released together.

Byte equality everywhere, no tolerance, no excluded output.  Nothing here tries to make anything fail: the spin is a bounded delay, and a
thread that does not come back within its limit fails its test and skips the rest of the module."""
import collections
import ctypes as C
import threading
import time

import numpy as np
import pytest

from tests import inflight_cases as S
from tests.helpers import first_difference, result_bytes

pytestmark = pytest.mark.gpu

SPIN_MS = 5.0                    # outlasts the host side of a call between its entry and its first copy (microseconds up to about 1 ms)
NOT_HELD = ("dsss_create", "dsss_destroy", "dsss_last_error", "dsss_stream")
# dsss_frames_set with images in HBM returns with its work queued: behind a held-back stream the spin must still be running when it comes
# back (on a warm context: the first use of a frame slot, and boxes still on their way, synchronise).  dsss_mosaic_render does NOT return
# with work queued, whatever it downloads: it answers DSSS_E_CAPACITY for a cell of more than 2^24 samples, and reads that flag back
# before it returns (mosaic_flag_down).  For it, and for every other call, the proof that it was issued behind a busy stream is taken at
# its ENTRY: the event behind the spin has not fired when the library is entered.
ASYNC_BY_CONTRACT = {"pipeline_b": "dsss_frames_set_typed", "frames_again": "dsss_frames_set_typed"}
SYNCHRONOUS_BY_CONTRACT = {"mosaic": "dsss_mosaic_render"}

_HUNG = []                       # threads that did not come back, runs that met a HIP error: nothing more is started on the GPU
_IDLE = {}                       # scenario -> (results, bytes, seconds) of the run on a plain context


@pytest.fixture(autouse=True)
def _nothing_after_a_hang():
    if _HUNG:
        pytest.skip("%s did not come back or met a HIP error: nothing more is started on the GPU" % _HUNG[0])


class HeldBack:
    """The library handle of ONE context with its stream held back: before every dsss_* call that takes the context (but NOT_HELD) a spin
    kernel goes onto the context's stream and an event behind it; whether that event had fired when the call returned is kept by name."""

    def __init__(self, L, h, cycles, counts, at_return, at_entry):
        import torch
        self._L, self._h, self._cycles, self._counts, self._at_return, self._at_entry, self._torch = L, h.value, cycles, counts, at_return, at_entry, torch
        self._stream = torch.cuda.ExternalStream(L.dsss_stream(h))

    def __getattr__(self, name):
        fn = getattr(self._L, name)
        if not name.startswith("dsss_"):
            return fn
        torch = self._torch

        def call(*args):
            self._counts[name] += 1
            held = name not in NOT_HELD and len(args) > 0 and isinstance(args[0], C.c_void_p) and args[0].value == self._h
            if not held:
                return fn(*args)
            with torch.cuda.stream(self._stream):
                torch.cuda._sleep(self._cycles)
            ev = torch.cuda.Event()
            ev.record(self._stream)
            busy = not ev.query()                            # the stream lags at the moment the library is entered
            rc = fn(*args)
            self._at_return[name].append(bool(ev.query()))
            self._at_entry[name].append(busy)
            return rc
        return call


class Factory:
    """new_ctx of a scenario: contexts of one run, plain or held back, closed together"""

    def __init__(self, cycles=None):
        self.cycles, self.made = cycles, []
        self.counts = collections.Counter(); self.at_return = collections.defaultdict(list); self.at_entry = collections.defaultdict(list)

    def __call__(self, max_frames):
        from diasss_amd import capi
        c = capi.Context(max_frames=max_frames)
        if self.cycles is not None:
            c.L = HeldBack(c.L, c.h, self.cycles, self.counts, self.at_return, self.at_entry)
        self.made.append(c)
        return c

    def close(self):
        for c in self.made:
            c.close()
        self.made = []


def _run(name, cycles=None):
    """one scenario on contexts of its own -> (results, factory, seconds)"""
    s = S.SCENARIOS[name]
    f = Factory(cycles)
    t0 = time.perf_counter()
    try:
        res = s.run(s.make(f))
    except Exception as ex:
        if getattr(ex, "code", None) == -3 or "HIP error" in str(ex):      # DSSS_E_HIP, or torch's: the device may have faulted
            _HUNG.append("%s (%s)" % (name, ex))
        raise
    finally:
        if not _HUNG:
            f.close()
    return res, f, time.perf_counter() - t0


def _idle(name):
    if name not in _IDLE:
        _run(name)                                           # (inputs, lazy module loads and the allocator's first blocks are not the scenario's time)
        res, _, dt = _run(name)
        b = result_bytes(res)
        assert len(b) > 0
        _IDLE[name] = (res, b, dt)
    return _IDLE[name]


def _same_as_idle(name, res, what):
    idle, b, _ = _idle(name)
    d = first_difference(idle, res, name)
    assert d is None and result_bytes(res) == b, "%s differs from the idle context's: %s" % (what, d)


@pytest.fixture(scope="module")
def spin_cycles():
    """torch.cuda._sleep cycles for SPIN_MS on an idle stream of a context of this library, measured by two events"""
    import torch
    from diasss_amd import capi
    assert hasattr(torch.cuda, "_sleep") and hasattr(torch.cuda, "ExternalStream")
    c = capi.Context(max_frames=1)
    try:
        st = torch.cuda.ExternalStream(c.L.dsss_stream(c.h))

        def ms(cycles):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(st):
                e0.record(st); torch.cuda._sleep(cycles); e1.record(st)
            e1.synchronize()
            return e0.elapsed_time(e1)
        probe = 2_000_000
        ms(probe)
        per_cycle = min(ms(probe) for _ in range(3)) / probe
        cycles = max(1, int(SPIN_MS / per_cycle))
        got = min(ms(cycles) for _ in range(3))
    finally:
        c.close()
    print("held-back stream: %d cycles spin for %.2f ms (wanted %.1f)" % (cycles, got, SPIN_MS))
    assert 2.0 <= got <= 50.0, got
    return cycles


def test_binding_releases_the_gil():
    from diasss_amd import capi
    L = capi.lib()
    assert isinstance(L, C.CDLL) and not isinstance(L, C.PyDLL)


# ---------------------------------------------------------------- the anchor
@pytest.mark.parametrize("name", ["pipeline_a", "pipeline_b"])
def test_idle_pipeline_vs_oracle(orc, name):
    """the idle bytes of the pipeline scenarios under the comparisons and bars of test_gpu_configs.py::test_config_C2_full_pipeline_vs_oracle:
    features, rows and kp7 bit-exact, mini-LMs same iterations and 1e-9, the selected edges identical, LM iterations equal, poses 1e-6.
    C2's counts -- more than 500 closures, more than 100 edges -- belong to its 50 frames; three and four frames cannot reach them.  The
    bars here are set from the ORACLE's counts on these surveys, computed on the CPU before any device run (pipeline_a: 337 rows, 337
    closures, 50 edges; pipeline_b: 88, 88, 16) at about half of each: every stage behind the extraction has something to compare."""
    import torch
    from diasss_amd.pipeline import all_pairs
    from tests.test_gpu_configs import _oracle_backend
    p = S.PIPELINES[name]
    F, N, M = p["F"], p["N"], p["M"]
    _, raws, ins = S.pipeline_inputs(name)
    res = _idle(name)[0]
    g_poses, g_stats, g_feat, g_pairs, g_edges = res[0], res[1], res[2], res[5], res[7]
    assert first_difference(res[9], [g_poses, g_stats]) is None, "the survey run again on the warm context differs from its first run"
    po = orc.orb_params()
    if p["nfeatures"]:
        po.nfeatures = int(p["nfeatures"])
    fr = []
    for f in range(F):
        pose, alt, gr = ins[f]
        kps, desc, _, _ = orc.detect_feature(raws[f].cpu().to(torch.float64).numpy(), None, po)
        fr.append(dict(pose=pose, alt=alt, gr=gr, kps=kps, desc=desc, geo=orc.geo_at_kps(pose, gr, M, kps), bb=orc.geo_bbox(pose, gr, M)))
        k, d, g = g_feat[f]
        assert len(k) == len(kps) and (d == desc).all() and (k["x"] == kps["x"]).all()
        assert (k["y"] == kps["y"]).all() and (k["angle"] == kps["angle"]).all() and (g == fr[f]["geo"]).all()
    src, tgt = all_pairs(F)
    rows = {}
    for q, (i, j) in enumerate(zip(src, tgt)):
        a, b = fr[i], fr[j]
        rows[(i, j)] = orc.robust_matching(int(i), int(j), N, N, a["kps"], a["desc"], a["geo"], a["bb"], b["kps"], b["desc"], b["geo"], b["bb"])
        assert g_pairs[q][3].shape == rows[(i, j)].shape and (g_pairs[q][3] == rows[(i, j)]).all(), "rows of pair %d-%d differ" % (i, j)
    edges, o_poses, o_stats, k7, lc = _oracle_backend(orc, fr, F, N, M, lambda i, j: rows[(i, j)])
    n_lc = 0
    for q in range(len(src)):
        assert g_pairs[q][4].shape == k7[q].shape and (g_pairs[q][4] == k7[q]).all()
        g = g_pairs[q][5]
        assert len(g) == len(lc[q])
        if len(g):
            n_lc += len(g)
            assert (g["iters"] == lc[q]["iters"]).all()
            assert np.abs(g["rel"] - lc[q]["rel"]).max() < 1e-9 and np.allclose(g["var"], lc[q]["var"], rtol=1e-6, atol=0)
    print("%s: %d keypoints, %d rows, %d closures, %d edges, LM %s" % (name, sum(len(f["kps"]) for f in fr), sum(len(r) for r in rows.values()), n_lc, len(edges), g_stats))
    assert len(g_edges) == len(edges)
    assert (g_edges["a"] == edges["a"]).all() and (g_edges["b"] == edges["b"]).all()
    n_rows, min_lc, min_edges = sum(len(r) for r in rows.values()), *{"pipeline_a": (150, 25), "pipeline_b": (50, 10)}[name]
    assert n_rows > min_lc and n_lc > min_lc and len(edges) > min_edges, (n_rows, n_lc, len(edges))
    assert sum(len(q[3]) for q in g_pairs) == n_rows and g_stats[0] >= 1 and g_stats[2] < g_stats[1]      # the device's own rows; the LM moved
    assert g_stats[0] == o_stats[0]
    assert np.abs(g_poses - o_poses).max() < 1e-6


def test_idle_results_agree_among_themselves():
    """what needs no oracle: outputs of one idle run that must be equal because they come from the same input by different roads.
    frames_again: every stage output of a frame depends on the image it holds alone -- whichever of pageable memory, HBM, dsss_frame_set,
    dsss_frames_set, or a frame set again behind a started extraction brought it there.  features_and_match: the matcher over frames whose
    features arrived in records gives what it gave over the frames the records were packed from."""
    res = _idle("frames_again")[0]
    first = {}
    for k, (img, pick) in enumerate(S.SCENARIOS["frames_again"].run.images):
        st = pick(res)[:-2]                                  # (without the candidate taps and where the image lives)
        if img in first:
            d = first_difference(first[img][1], st, "stages %d against stages %d (image %s)" % (k, first[img][0], img))
            assert d is None, d
        else:
            first[img] = (k, st)
    assert first_difference(first["a"][1], first["b"][1]) is not None
    res = _idle("features_and_match")[0]
    assert first_difference(res[3], res[7][0], "matcher over unpacked records against the frames they were packed from") is None
    assert first_difference(res[4], res[7][1:], "SIFT rows after unpack") is None


# ---------------------------------------------------------------- arm A
@pytest.mark.parametrize("name", list(S.SCENARIOS))
def test_behind_a_held_back_stream(spin_cycles, name):
    """every call of the scenario issued behind about 5 ms of spin on the context's own stream: the idle bytes, every entry the table
    names really called, and the calls that return with their work queued really returned before the spin had ended"""
    _, _, solo = _idle(name)
    res, f, dt = _run(name, spin_cycles)
    held = sum(len(v) for v in f.at_return.values())
    print("%s: idle %.3f s, held back %.3f s (%d calls behind a spin, %d of them back before it ended)" % (
        name, solo, dt, held, sum(v.count(False) for v in f.at_return.values())))
    print("  calls: " + ", ".join("%s %d" % (k[5:], n) for k, n in sorted(f.counts.items())))
    print("  back with work queued: " + (", ".join("%s %d of %d" % (k[5:], v.count(False), len(v)) for k, v in sorted(f.at_return.items()) if False in v) or "none"))
    _same_as_idle(name, res, "the run behind a held-back stream")
    missing = [e for e in S.SCENARIOS[name].entries if f.counts[e] == 0]
    assert not missing, "the table says %s drives %s: never called" % (name, missing)
    assert held > 0 and not set(f.at_return) & set(NOT_HELD)
    not_behind = [e for e in S.SCENARIOS[name].entries if e not in NOT_HELD and not f.at_entry[e]]
    assert not not_behind, "the table says %s drives %s: called, but never behind a spin" % (name, not_behind)
    idle_entries = {k: v.count(False) for k, v in f.at_entry.items() if False in v}
    assert not idle_entries, "calls entered with the spin in front of them already over: %s" % idle_entries
    if name in ASYNC_BY_CONTRACT:
        back = f.at_return[ASYNC_BY_CONTRACT[name]]
        assert False in back, "%s never returned before the spin in front of it had ended (%s): the stream was not busy" % (ASYNC_BY_CONTRACT[name], back)
    if name in SYNCHRONOUS_BY_CONTRACT:
        back = f.at_return[SYNCHRONOUS_BY_CONTRACT[name]]
        assert len(back) >= 6 and all(back), "%s came back with work queued (%s): its capacity answer cannot have been read" % (SYNCHRONOUS_BY_CONTRACT[name], back)


# ---------------------------------------------------------------- arm B
def _in_flight(jobs, cycles=None):
    """jobs: [(scenario names in order, repetitions)], one host thread each with contexts of its own, released together by a barrier.
    Every repetition of every thread must have the idle bytes.  join is limited to 20 x the thread's solo time, measured here, at least 30 s."""
    for n in {n for names, _ in jobs for n in names}:
        _idle(n)                                             # the bytes to compare with (and the warm-up of the solo times below)
    once = {n: _run(n, cycles)[2] for n in sorted({n for names, _ in jobs for n in names})}      # solo, in this test, as the threads will run it
    solo = [sum(once[n] for n in names) * reps for names, reps in jobs]
    barrier = threading.Barrier(len(jobs))
    got = [[] for _ in jobs]; failed = [None] * len(jobs); took = [None] * len(jobs)

    def work(k):
        names, reps = jobs[k]
        try:
            barrier.wait(timeout=60)
            t0 = time.perf_counter()
            for rep in range(reps):
                for n in names:
                    got[k].append((n, rep, _run(n, cycles)[0]))
            took[k] = time.perf_counter() - t0
        except BaseException as ex:                          # carried to the test and raised there
            failed[k] = ex

    threads = [threading.Thread(target=work, args=(k,), name="inflight-%d-%s" % (k, "+".join(jobs[k][0])), daemon=True) for k in range(len(jobs))]
    t0 = time.perf_counter()
    for t in threads:
        t.start()
    for k, t in enumerate(threads):
        t.join(max(0.0, max(30.0, 20.0 * solo[k]) - (time.perf_counter() - t0)))
    for t in threads:
        if t.is_alive():
            _HUNG.append(t.name)
    assert not _HUNG, "threads that did not come back: %s" % _HUNG
    for k, ex in enumerate(failed):
        if ex is not None:
            raise ex
    for k, (names, reps) in enumerate(jobs):
        print("thread %d, %s x %d: solo %.3f s, in flight %.3f s" % (k, " + ".join(names), reps, solo[k], took[k]))
        assert len(got[k]) == len(names) * reps
        for n, rep, res in got[k]:
            _same_as_idle(n, res, "thread %d, repetition %d" % (k, rep))


def test_four_contexts_in_flight():
    _in_flight([(("pipeline_a",), 3), (("pipeline_b",), 3), (("mosaic", "register"), 3), (("pg_parts",), 3)])


def test_same_scenario_on_every_thread():
    """four analyses by parts at once: the heaviest use of the shared worker pool and of the analysis threads; then four whole pipelines
    (extraction, matcher, mini-LMs, selection, pose graph: 337 closures and 50 edges each)"""
    _in_flight([(("pg_parts",), 1)] * 4)
    _in_flight([(("pipeline_a",), 1)] * 4)


def test_lifecycle_beside_running_contexts():
    """contexts created and destroyed (streams, hipMalloc / hipFree) while two others run"""
    _in_flight([(("lifecycle",), 1), (("pipeline_a",), 2), (("pg_edges",), 4)])


def test_held_back_and_in_flight(spin_cycles):
    _in_flight([(("frames_again",), 2), (("features_and_match",), 2)], spin_cycles)

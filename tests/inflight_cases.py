"""The scenario table of tests/test_gpu_inflight.py: fixed sequences of library calls whose downloaded results must have the same bytes on an
idle context, behind a held-back stream and beside other contexts in flight.  tests/test_inflight_cpu.py holds the table to its claims
(every entry of include/dsss.h is driven by a scenario or exempt for a stated reason; pg_parts is analysed by parts) without a GPU.

A scenario is (name, make(new_ctx) -> state, run(state) -> results, entries):
  make     builds the contexts it needs through new_ctx(max_frames) (a diasss_amd.capi.Context, plain or held back: the caller decides and
           closes them) and whatever else run needs; inputs are computed once per process and shared, read only;
  run      drives the calls and returns everything it downloaded as nested lists of arrays and scalars (tests.helpers.result_bytes);
  entries  the dsss_* names the scenario is there to drive: behind a held-back stream each of them must have been called.

No reference arithmetic lives here: every input is one an existing test already holds to its reference, at that test's small sizes (the
module named at each scenario).  Sizes that are not the very smallest of their test are the smallest at which the call has something to
decide: a matcher over no keypoints, or a pose graph below the by-parts threshold, would make the comparison empty."""
import collections
import ctypes as C
import functools
import re

import numpy as np

Scenario = collections.namedtuple("Scenario", "name make run entries")


def _orc():
    from oracle import binding
    binding.lib()
    return binding


def _record(buf, K, sift):
    """what a packed feature record defines: its header, the box and the first n rows of every section.  (The record always holds K rows
    a section, and "only the first n rows of a section mean anything", include/dsss.h: the rest is whatever the store held.)"""
    from tests import feature_transport_ref as R
    r = R.parse_record(np.ascontiguousarray(buf, np.uint8), K, sift)
    n = max(0, min(r["n"], K))
    return [[r["n"], r["N"], r["M"], r["pad"]], r["bbox"], r["kps"][:n], r["desc"][:n], r["geo"][:n], r["d128"][:n] if sift else None]


def _struct(s):
    """a ctypes structure of scalars as a list of its fields' values"""
    return [getattr(s, f[0]) for f in s._fields_]


# ---------------------------------------------------------------- pipeline_a, pipeline_b
# pipeline_a: the u16 survey of test_gpu_raw_types.py::test_u16_survey_through_the_pipeline (four legs recorded as uint16, tile 512, pageable
# frames) at 700 x 480 instead of 600 x 256: at that test's size the oracle finds no match in any of the six pairs, and everything behind the
# extraction would be compared empty; at the suite's usual small size it finds 337 rows, 337 closures and 50 edges.
# pipeline_b: the two legs + one of test_gpu_register_segments.py's survey family (640 x 400, seed 7) as f64 frames in HBM, so that the eager
# start of dsss_frames_set runs; nfeatures 1000: another kcap, other geometries, another pair set (3 pairs against 6).
PIPELINES = {"pipeline_a": dict(F=4, N=700, M=480, seed=20240601, dtype="uint16", on_device=False, nfeatures=None),
             "pipeline_b": dict(F=3, N=640, M=400, seed=7, dtype=None, on_device=True, nfeatures=1000)}


@functools.lru_cache(maxsize=None)
def pipeline_inputs(name):
    """(survey, raws (torch tensors, host or device), [(pose, alt, gr)]) of a pipeline scenario"""
    from diasss_amd import synth
    p = PIPELINES[name]
    S = synth.Survey(p["F"], p["N"], p["M"], seed=p["seed"], tile=512)
    raws = [S.frame(f, p["dtype"]) for f in range(p["F"])]
    if p["on_device"]:
        raws = [r.cuda() for r in raws]
    return S, raws, [S.inputs(f) for f in range(p["F"])]


def _pipeline(name):
    p = PIPELINES[name]
    F = p["F"]

    def make(new_ctx):
        from diasss_amd.pipeline import Pipeline
        _, raws, ins = pipeline_inputs(name)
        ctx = new_ctx(F)
        return dict(ctx=ctx, pipe=Pipeline(F, ctx=ctx, nfeatures=p["nfeatures"]), raws=raws, ins=ins)

    def run(st):
        pipe, c, ins = st["pipe"], st["ctx"], st["ins"]
        first = pipe.run(st["raws"], [i[0] for i in ins], [i[1] for i in ins], [i[2] for i in ins])
        first = [np.array(first[0], copy=True), np.array(first[1], copy=True)]
        # the survey again on the warm context, the steady state of a production step: no buffer grows, nothing synchronises on the way in
        poses, stats = pipe.run(st["raws"], [i[0] for i in ins], [i[1] for i in ins], [i[2] for i in ins])
        out = [np.array(poses, copy=True), np.array(stats, copy=True)]
        out.append([c.features_get(f) for f in range(F)])
        out.append([list(c.frame_raw_info(f)) for f in range(F)])
        out.append([c.frame_bbox(f) for f in range(F)])
        pairs = []
        for k in range(len(pipe.src)):
            s, t = int(pipe.src[k]), int(pipe.tgt[k])
            pairs.append([c.pair_is_active(k), list(c.match_dir(k, 0)), list(c.match_dir(k, 1)), c.match_rows(k), c.match_kp7(k), c.lc_get(k),
                          np.float32(c.overlap(s, t))])
        out.append(pairs)
        out.append(list(c.match_total()))
        out.append(c.posegraph_select(F, cap=1 << 14))
        lv, trials = c.posegraph_schedule()
        out.append([lv, trials])
        out.append(first)
        return out

    entries = ("dsss_frames_set_typed", "dsss_extract_many", "dsss_match_pairs", "dsss_lc_solve_all", "dsss_posegraph_solve", "dsss_features_get",
               "dsss_frame_raw_info", "dsss_frame_bbox", "dsss_match_pair_active", "dsss_match_get_dir", "dsss_match_get_rows", "dsss_match_get_kp7",
               "dsss_lc_get", "dsss_overlap", "dsss_match_total", "dsss_posegraph_select", "dsss_posegraph_schedule_get")
    return Scenario(name, make, run, entries + (("dsss_set_params",) if p["nfeatures"] else ()))


# ---------------------------------------------------------------- frames_again
def _frames_again():
    """test_gpu_raw_types.py::test_frame_set_again_with_another_type's geometry (raw_types_ref.SHAPES[3]) and type table: the u16 speckle
    frame, then the u16 flat_with_hot frame on the same id -- another image of the same size and type, so the owned block does not regrow
    -- with an extraction after each; then the same two through dsss_frames_set with the images in HBM (the eager start)."""
    from tests import extract_shapes_ref as X
    from tests import raw_types_ref as R
    N, M, nl, nf = R.SHAPES[3]

    @functools.lru_cache(maxsize=None)
    def inputs():
        a = R.frame("speckle", "u16", N, M); b = R.frame("flat_with_hot", "u16", N, M)
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() != b.tobytes()
        return a, b, X.dr_inputs(N, M)

    def make(new_ctx):
        import torch
        a, b, _ = inputs()
        c = new_ctx(4)
        mp, op = X.device_params(c, R.MASK, R.orb(nl, nf))
        c.set_params(mask=mp, orb=op)
        dev = [torch.from_numpy(q.view(np.int16)).cuda() for q in (a, b)]      # torch has no uint16 arithmetic on every build: int16 storage, the type given
        torch.cuda.synchronize()
        return dict(ctx=c, dev=dev)

    def stages(c, fid):
        """every stage output of a frame.  The last two items are the candidate taps, which only dsss_extract refreshes (dsss_extract_many
        leaves those of the frame's last dsss_extract), and where the image lives; the rest depends on the image alone"""
        norm, mask = c.frame_norm(fid, N, M)
        return [norm, mask, [c.frame_level(fid, l, N, M) for l in range(nl)], list(c.features_get(fid)), list(c.frame_raw_stats(fid)), c.frame_bbox(fid),
                [list(c.frame_candidates(fid, l)) for l in range(nl)], list(c.frame_raw_info(fid))]

    def run(st):
        c = st["ctx"]
        a, b, (pose, alt, gr) = inputs()
        out = []
        for q in (a, b):
            c.frame_set(1, q, N, M, pose, alt, gr)
            c.extract_many([1])
            out.append(stages(c, 1))
        for d in st["dev"]:
            c.frames_set([1, 2], [d, d], [N, N], [M, M], [pose, pose], [alt, alt], [gr, gr], raw_types=[R.RAW_U16, R.RAW_U16])
            c.extract_many([1, 2])
            out.append([stages(c, 1), stages(c, 2)])
        # frames 1 and 2 with image a from pageable memory (the extraction of both is started), frame 1 set again with image b -- a copy into
        # the same owned block while that start is still queued -- then the extraction of the started list
        c.frames_set([1, 2], [a, a], [N, N], [M, M], [pose, pose], [alt, alt], [gr, gr])
        c.frame_set(1, b, N, M, pose, alt, gr)
        c.extract_many([1, 2])
        out.append([stages(c, 1), stages(c, 2)])
        # the same start, and a frame that is NOT of the started list set behind it (a rank sets frames it does not extract): the start stands
        c.frames_set([1, 2], [a, a], [N, N], [M, M], [pose, pose], [alt, alt], [gr, gr])
        c.frame_set(3, b, N, M, pose, alt, gr)
        c.extract_many([1, 2])
        c.extract_many([3])
        out.append([stages(c, 1), stages(c, 2), stages(c, 3)])
        c.frame_set(1, a, N, M, pose, alt, gr)
        out.append(c.extract(1))
        out.append(stages(c, 1))
        c.sync()
        return out

    # which image every stages() of the results saw: run's own bookkeeping, for the consistency check of tests/test_gpu_inflight.py
    run.images = (("a", lambda r: r[0]), ("b", lambda r: r[1]), ("a", lambda r: r[2][0]), ("a", lambda r: r[2][1]), ("b", lambda r: r[3][0]),
                  ("b", lambda r: r[3][1]), ("b", lambda r: r[4][0]), ("a", lambda r: r[4][1]), ("a", lambda r: r[5][0]), ("a", lambda r: r[5][1]), ("b", lambda r: r[5][2]),
                  ("a", lambda r: r[7]))
    return Scenario("frames_again", make, run,
                    ("dsss_set_params", "dsss_frame_set_typed", "dsss_frames_set_typed", "dsss_extract", "dsss_extract_many", "dsss_frame_get_norm",
                     "dsss_frame_get_level", "dsss_frame_get_candidates", "dsss_features_get", "dsss_frame_raw_info", "dsss_frame_raw_stats", "dsss_frame_bbox", "dsss_sync"))


# ---------------------------------------------------------------- features_and_match
MATCH_SIZES = (300, 300)         # test_gpu_matcher.py::test_matcher_sizes: the smallest of its sizes at which rows come out (it asserts > 20)
L2_SIZES = (300, 257)            # test_gpu_sift.py::test_l2_matcher_ties_and_sizes: its one size past a tile of the L2 kernel


@functools.lru_cache(maxsize=None)
def match_inputs():
    """the two frames of test_matcher_sizes at MATCH_SIZES and of test_l2_matcher_ties_and_sizes at L2_SIZES, built as those tests build them"""
    from tests import helpers as H
    N, M = 700, 480
    ham = []
    for f, n in enumerate(MATCH_SIZES):
        pose, alt, gr = H.track(N, M, 0, seed=3)
        pose = pose.copy(); pose[:, 4] += 0.3 * f
        kps, desc = H.random_features(N, M, n, 50 + f + 10 * n)
        if f == 1:
            kps = ham[0]["kps"].copy(); desc = ham[0]["desc"].copy()
            rng = np.random.default_rng(n)
            for i in range(n):
                for b in rng.choice(256, rng.integers(0, 20), replace=False):
                    desc[i, b // 8] ^= np.uint8(1 << (b % 8))
            kps["y"] += rng.integers(-3, 4, n).astype(np.float32)
        ham.append(dict(pose=pose, alt=alt, gr=gr, kps=kps, desc=desc))
    l2 = []
    rng = np.random.default_rng(sum(L2_SIZES))
    protos = rng.integers(0, 256, (6, 128)).astype(np.uint8)
    for f, n in enumerate(L2_SIZES):
        pose, alt, gr = H.track(N, M, 0, seed=3)
        pose = pose.copy(); pose[:, 4] += 0.3 * f
        kps, desc = H.random_features(N, M, n, 50 + f + 10 * n)
        d128 = protos[rng.integers(0, 6, n)].copy()
        d128[rng.random(n) < 0.3, 5] ^= 1
        l2.append(dict(pose=pose, alt=alt, gr=gr, kps=kps, desc=desc, d128=d128.astype(np.float32)))
    return N, M, ham, l2


def _features_and_match():
    def make(new_ctx):
        return dict(ctx=new_ctx(6), fresh=new_ctx(4))

    def getters(c, pair=0):
        return [c.pair_is_active(pair), list(c.match_dir(pair, 0)), list(c.match_dir(pair, 1)), c.match_rows(pair), c.match_kp7(pair), list(c.match_total())]

    def run(st):
        import torch
        from diasss_amd import capi
        from tests import feature_transport_ref as R
        c = st["ctx"]
        N, M, ham, l2 = match_inputs()
        mp, op, mt, pg = c.default_params()
        out = []
        for mode in (0, 1):                                  # Hamming, then L2 on the 32 ORB bytes: set, match, read, nothing in between
            mt.use_l2 = mode
            c.set_params(match=mt)
            for f, fr in enumerate(ham):
                c.frame_set(2 * f, None, N, M, fr["pose"], fr["alt"], fr["gr"])
                c.features_set(2 * f, N, M, fr["kps"], fr["desc"])
            c.match_pairs([0], [2])
            out.append(getters(c))
        out.append([c.descriptor_distance(0, 0, 2, 0), c.descriptor_distance(0, 5, 2, 7), np.float32(c.overlap(0, 2)), c.frame_bbox(2)])
        op.descriptor = capi.DESC_SIFT128; mt.use_l2 = 2     # the 128-byte rows
        c.set_params(orb=op, match=mt)
        for f, fr in enumerate(l2):
            c.frame_set(2 * f, None, N, M, fr["pose"], fr["alt"], fr["gr"])
            c.features_set(2 * f, N, M, fr["kps"], fr["desc"])
            c.features_set_sift(2 * f, fr["d128"])
        c.match_pairs([0], [2])
        out.append(getters(c))
        out.append([c.features_get_sift(0), c.features_get_sift(2)])
        # frame 0's record through a host buffer into frame 4, through a device buffer into frame 2's slot, and the matcher straight behind
        nb = c.pack_bytes()
        host = np.zeros(nb, np.uint8); dev = torch.zeros(nb, dtype=torch.uint8, device="cuda")
        c.frame_set(4, None, N, M, l2[0]["pose"], l2[0]["alt"], l2[0]["gr"])
        c.features_pack(0, host)
        c.features_unpack(4, host)
        c.features_pack(2, dev)
        c.features_unpack(2, dev)
        c.match_pairs([4, 0], [2, 4])
        K = R.capacity(nb, True)
        out.append([getters(c, 0), getters(c, 1), list(c.features_get(4)), c.features_get_sift(4), _record(host, K, True), _record(dev.cpu().numpy(), K, True)])
        out.append(list(c.frame_geo(4, N, M)))
        # a context whose FIRST SIFT rows arrive in records (a rank that extracts nothing itself), and the matcher straight behind
        d = st["fresh"]
        d.set_params(orb=op, match=mt)
        other = np.zeros(nb, np.uint8)
        c.features_pack(2, other)
        for fid, fr, rec in ((0, l2[0], host), (2, l2[1], other)):
            d.frame_set(fid, None, N, M, fr["pose"], fr["alt"], fr["gr"])
            d.features_unpack(fid, rec)
        d.match_pairs([0], [2])
        out.append([getters(d), d.features_get_sift(0), d.features_get_sift(2)])
        return out

    return Scenario("features_and_match", make, run,
                    ("dsss_set_params", "dsss_frame_set_typed", "dsss_features_set", "dsss_features_set_sift", "dsss_features_get", "dsss_features_get_sift",
                     "dsss_features_pack_bytes", "dsss_features_pack", "dsss_features_unpack", "dsss_match_pairs", "dsss_match_pair_active", "dsss_match_get_dir",
                     "dsss_match_get_rows", "dsss_match_get_kp7", "dsss_match_total", "dsss_descriptor_distance", "dsss_overlap", "dsss_frame_bbox",
                     "dsss_frame_get_geo"))


# ---------------------------------------------------------------- lc_and_tri
def _lc_and_tri():
    """helpers.lc_cases' "select" group (test_gpu_ctx_buffers.py::test_select_and_solve_few_many_few, test_gpu_lc_paths.py): the stand-alone
    mini-LMs and triangulations, the batch solve of all pairs with selection and pose graph, and -- these frames being the smallest the
    suite has with loop closures between them -- the online forms: an update over two frames, a windowed one over the third."""
    @functools.lru_cache(maxsize=None)
    def inputs():
        from tests import helpers as H
        orc = _orc()
        g = H.lc_cases(orc, 0)["select"]
        s, t, k = g["lists"][0]
        ps, pt = g["frames"][s][0], g["frames"][t][0]
        in27 = np.zeros((len(k), 27))
        for i, row in enumerate(k):                          # explicit poses as test_triangulate_group builds them; the start point 9 m under the midpoint
            in27[i, :12] = orc.pose12(ps[int(row[0])]); in27[i, 12:24] = orc.pose12(pt[int(row[3])])
            in27[i, 24:] = 0.5 * (ps[int(row[0]), 3:] + pt[int(row[3]), 3:]) - [0.0, 0.0, 9.0]
        return g, in27

    def make(new_ctx):
        from tests.helpers import LC_M, LC_N
        g, _ = inputs()
        c = new_ctx(4)
        for f, (pose, alt, gr) in enumerate(g["frames"]):
            c.frame_set(f, None, LC_N, LC_M, pose, alt, gr)
        return dict(ctx=c)

    def run(st):
        from tests.helpers import LC_N
        c = st["ctx"]
        g, in27 = inputs()
        lists = g["lists"]
        out = []
        for s, t, k in lists:
            out.append([c.lc_solve(s, t, k), c.triangulate(s, t, k)])
        out.append(c.triangulate_poses(lists[0][2], in27))
        c.lc_solve_pairs([l[0] for l in lists], [l[1] for l in lists], [l[2] for l in lists])
        out.append([[c.lc_get(p), c.match_kp7(p)] for p in range(len(lists))])
        out.append(c.posegraph_select(3, cap=1 << 14))
        out.append(list(c.posegraph_solve(3, 3 * LC_N)))
        c.posegraph_reset()
        c.lc_solve_pairs([lists[0][0]], [lists[0][1]], [lists[0][2]])            # pair (0, 1): the closures of the first two frames
        out.append(list(c.posegraph_update(2, 2 * LC_N, want_rpy=True)) + [c.posegraph_online_edges()])
        c.lc_solve_pairs([l[0] for l in lists[1:]], [l[1] for l in lists[1:]], [l[2] for l in lists[1:]])      # the closures that end in frame 2
        out.append(list(c.posegraph_update_window(3, 3 * LC_N, 1)) + [c.posegraph_online_edges()])
        c.posegraph_reset()
        out.append(c.posegraph_online_edges())
        return out

    return Scenario("lc_and_tri", make, run,
                    ("dsss_frame_set_typed", "dsss_lc_solve", "dsss_triangulate", "dsss_triangulate_poses", "dsss_lc_solve_pairs", "dsss_lc_get", "dsss_match_get_kp7",
                     "dsss_posegraph_select", "dsss_posegraph_solve", "dsss_posegraph_update", "dsss_posegraph_update_window", "dsss_posegraph_reset",
                     "dsss_posegraph_online_edges"))


# ---------------------------------------------------------------- pg_edges
def _pg_edges():
    """helpers.pg_small_graph (test_gpu_pg_report.py, test_gpu_ctx_buffers.py::test_report_and_gated_solve_small_large_small): the stand-alone
    solve, the report at its result and the gated solve, back to back.  (dsss_posegraph_update and _update_window work on frames and
    accumulated loop closures, which this graph has none of: lc_and_tri drives them.)"""
    @functools.lru_cache(maxsize=None)
    def inputs():
        from tests.helpers import pg_small_graph
        return pg_small_graph(_orc())

    def make(new_ctx):
        inputs()
        return dict(ctx=new_ctx(2))

    def run(st):
        c = st["ctx"]
        dr, edges = inputs()
        poses, stats = c.posegraph_solve_edges(dr, edges)
        lv, trials = c.posegraph_schedule()
        return [poses, stats, [lv, trials], list(c.posegraph_edge_report(dr, edges, poses)), list(c.posegraph_solve_gated(dr, edges))]

    return Scenario("pg_edges", make, run, ("dsss_posegraph_solve_edges", "dsss_posegraph_edge_report", "dsss_posegraph_solve_gated", "dsss_posegraph_schedule_get"))


# ---------------------------------------------------------------- pg_parts
# _lawnmower_graph(n_lines, per_line, n_lc, seed) of test_gpu_configs.py.  The analysis goes by parts from 1 500 separators on AND only
# where a boundary between two parts is crossed by at most PG_PARTS_CUT_MAX = 12 loop closures (dsss_pg_sym.cpp: pg_analyse).  A survey of
# few long legs never has such a gap (4 x 1000 pings with 960 closures: 1 500 separators, the cheapest gap is crossed by 319), so the legs are
# short and many: 50 x 120 pings, and the fewest closures, in steps of ten, that reach 1 500 separators.  tests/test_inflight_cpu.py asserts all of it.
PG_PARTS_GRAPH = (50, 120, 910, 7)
PG_PARTS_MIN_SEPARATORS, PG_PARTS_CUT_MAX = 1500, 12


@functools.lru_cache(maxsize=None)
def pg_parts_graph(n_lc=PG_PARTS_GRAPH[2]):
    from tests.test_gpu_configs import _lawnmower_graph
    dr, _gt, e = _lawnmower_graph(PG_PARTS_GRAPH[0], PG_PARTS_GRAPH[1], n_lc, PG_PARTS_GRAPH[3])
    return dr, e


def pg_parts_plan(ns, ea, eb):
    """Where the device analysis cuts the chain order of a reduced graph (tests.pg_paths_ref.reduced_graph) into parts, restated from the rule
    in pg_analyse: K = min(8, max(2, ns / 1000)) parts from 1 500 separators on (16 from 65 536), boundary p at the gap crossed by the fewest
    loop closures within a third of a part of ns p / K (ties: the nearest), left out when more than max(12, ns / 16384) closures cross it.
    -> (K, boundaries kept, crossings of every boundary tried).  No boundary kept: the one-graph analysis.
    What this does NOT prove.  It is a restatement of dsss_pg_sym.cpp (pg_analyse, pg_cheapest_gap) in Python: faithful when written, and
    nothing but a reader keeps it so.  It says that pg_symbolic_parts is CALLED; that function can still decline (an interface of more than
    PG_PARTS_IFACE_MAX = 256 separators, or one that does not end up as the last front) and the device then analyses the graph as one,
    silently: no entry reports which analysis a solve took, and the GPU scenario observes none.  The host twin dsss_host_pg_solve_parts cuts
    at equal sizes without that interface limit, so its tables show what by-parts tables of this graph hold (bins, fronts of several panels),
    not that the device's cut succeeds.  With one boundary crossed by 10 closures the interface has some 20 separators, far below the limit."""
    K = 0 if ns < PG_PARTS_MIN_SEPARATORS else (min(8, max(2, ns // 1000)) if ns < 65536 else 16)
    if K < 2 or len(ea) <= ns - 1:
        return K, [], []
    K = min(K, ns // 8)
    lo = np.minimum(ea[ns - 1:], eb[ns - 1:]); hi = np.maximum(ea[ns - 1:], eb[ns - 1:])
    cross = np.zeros(ns + 1, np.int64)
    np.add.at(cross, lo + 1, 1); np.add.at(cross, hi + 1, -1)
    cross = np.cumsum(cross)                                 # cross[g]: closures that span the gap between separators g - 1 and g
    kept, costs, prev = [], [], 0
    for p in range(1, K):
        target, width = ns * p // K, ns // K // 3
        best, cost, dist = -1, 0, 0
        for i in range(max(1, target - width, prev + 1), min(ns, target + width + 1)):
            d = abs(i - target)
            if best < 0 or cross[i] < cost or (cross[i] == cost and d < dist):
                best, cost, dist = i, int(cross[i]), d
        costs.append(cost)
        if best > prev and cost <= max(PG_PARTS_CUT_MAX, ns // 16384):
            kept.append(best); prev = best
    return K, kept, costs


def _pg_parts():
    def make(new_ctx):
        pg_parts_graph()
        return dict(ctx=new_ctx(2))

    def run(st):
        c = st["ctx"]
        dr, e = pg_parts_graph()
        out = []
        for parts in (0, 3):                                 # by parts on the shared pool; then three partitions (the interface path)
            c.set_pg_partitions(parts)
            poses, stats = c.posegraph_solve_edges(dr, e)
            lv, trials = c.posegraph_schedule()
            out.append([poses, stats, lv, trials])
        c.set_pg_partitions(0)
        return out

    return Scenario("pg_parts", make, run, ("dsss_set_pg_partitions", "dsss_posegraph_solve_edges", "dsss_posegraph_schedule_get"))


# ---------------------------------------------------------------- mosaic
MOSAIC_CELL, FOOTPRINT_CELL = 0.8, 0.1            # test_gpu_ctx_buffers.py's coarse cell; a cell at two ping spacings for the footprints
GAIN_BANDS = (8.0, 0.5, 4)                        # helpers.track flies at 9 +- 1 m: four bands of half a metre from 8 m


@functools.lru_cache(maxsize=None)
def mosaic_legs():
    """the two legs of test_gpu_mosaic.py (640 x 400 heading +x, 500 x 700 heading back over it; seeded Rayleigh images)"""
    from tests import helpers as H
    legs = []
    for leg, (N, M) in enumerate(H.MOSAIC_SIZES):
        pose, alt, gr = H.track(N, M, leg, seed=9)
        legs.append((np.random.default_rng(leg).rayleigh(1.0, (N, M)) * 100.0, N, M, pose, alt, gr))
    return legs


def _layers(res):
    layers, info = res
    return [[layers[k] for k in sorted(layers)], _struct(info) if info is not None else None]


def _mosaic():
    def make(new_ctx):
        c = new_ctx(4)
        for i, L in enumerate(mosaic_legs()):
            c.frame_set(i, *L)
        c.extract_many([0, 1])
        return dict(ctx=c)

    def run(st):
        from diasss_amd import capi
        c = st["ctx"]
        ids = [0, 1]
        p = capi.mosaic_grid(c.mosaic_bounds(ids), MOSAIC_CELL)
        fine = capi.mosaic_grid(c.mosaic_bounds(ids), FOOTPRINT_CELL)
        p0 = capi.mosaic_grid(c.mosaic_bounds([0]), MOSAIC_CELL)
        out = []
        c.mosaic_render(ids, fine, download=False)           # every downloading call below is issued behind work that is still queued
        out.append(list(c.mosaic_consistency(ids, p)))
        c.mosaic_render(ids, fine, download=False)
        out.append(list(c.mosaic_render(ids, p)))
        # the column table of leg 0 (a table holds the frames of one M): estimate, install, read back, apply
        c.mosaic_render(ids, fine, download=False)
        S, Cn = c.mosaic_gain_stats([0])
        gain, T = capi.mosaic_gain_table(S, Cn)
        c.mosaic_gain_set(gain)
        c.mosaic_render([0], p0, download=False)
        out.append([S, Cn, gain, T, c.mosaic_gain_get(), c.frame_corrected(0), list(c.mosaic_render([0], p0))])
        # the banded twins
        c.mosaic_render([0], p0, download=False)
        Sb, Cb = c.mosaic_gain_stats([0], bands=GAIN_BANDS)
        gb, Tb = capi.mosaic_gain_table(Sb, Cb, nbands=GAIN_BANDS[2])
        c.mosaic_gain_set(gb, bands=GAIN_BANDS)
        c.mosaic_render([0], p0, download=False)
        table, bands = c.mosaic_gain_get_banded()
        out.append([Sb, Cb, gb, Tb, table, _struct(bands), c.frame_corrected(0), _layers(c.mosaic_composite([0], p0, mode="near", fill_radius=2))])
        c.mosaic_gain_set(None)
        c.mosaic_composite(ids, p, want=())                  # built on the device, nothing downloaded
        out.append(_layers(c.mosaic_composite(ids, p, mode="mid", fill_radius=2)))
        c.mosaic_render_footprint(ids, fine, download=False)
        out.append(list(c.mosaic_render_footprint(ids, fine)))
        c.mosaic_composite_footprint(ids, fine, want=())
        out.append(_layers(c.mosaic_composite_footprint(ids, fine, mode="near", fill_radius=1)))
        return out

    return Scenario("mosaic", make, run,
                    ("dsss_mosaic_bounds", "dsss_mosaic_render", "dsss_mosaic_consistency", "dsss_mosaic_gain_stats", "dsss_mosaic_gain_set", "dsss_mosaic_gain_get",
                     "dsss_mosaic_gain_stats_banded", "dsss_mosaic_gain_set_banded", "dsss_mosaic_gain_get_banded", "dsss_frame_get_corrected", "dsss_frame_get_level",
                     "dsss_mosaic_composite", "dsss_mosaic_render_footprint", "dsss_mosaic_composite_footprint"))


# ---------------------------------------------------------------- register
REG_CELL, REG_RADIUS, REG_MIN_CELLS, REG_SEG_PINGS = 0.5, 8, 256, 160


@functools.lru_cache(maxsize=None)
def register_frames():
    """frames 0 and 1 of test_gpu_register_segments.py -- the two legs of synth.Survey(2, 640, 400, seed=7) -- under its drifted survey:
    dead reckoning, leg 1 with register_edges_ref.drift"""
    from diasss_amd.synth import Survey
    from tests import register_edges_ref as E
    sv = Survey(2, 640, 400, seed=7)
    fr = []
    for f in range(2):
        pose, alt, gr = sv.inputs(f)
        fr.append((sv.frame(f).numpy().copy(), 640, 400, np.ascontiguousarray(pose), alt, gr))
    rows = [fr[0][3], np.ascontiguousarray(E.drift(fr[1][3]))]
    rpy = np.ascontiguousarray(np.concatenate([np.full((2, 6), 7.0e5), rows[0], np.full((3, 6), 7.0e5), rows[1]]))      # unrelated rows in front, as the tests pack them
    off = np.array([2, 2 + 640 + 3], np.int32)
    return fr, rpy, off


def _register():
    def make(new_ctx):
        fr, _, _ = register_frames()
        c = new_ctx(4)
        for i, L in enumerate(fr):
            c.frame_set(i, *L)
        c.extract_many([0, 1])
        return dict(ctx=c)

    def run(st):
        from diasss_amd import capi
        c = st["ctx"]
        _, rpy, off = register_frames()
        ids, pairs = [0, 1], [(0, 1)]
        p = capi.mosaic_grid(c.mosaic_bounds(ids, rpy, off), REG_CELL)
        p.use_mask = 0
        reg = capi.RegParams(REG_RADIUS, REG_MIN_CELLS)
        yaw = capi.RegYawParams(3, 0, 0.01)
        pyr = capi.RegPyrParams(2, 3)
        kw = dict(reg=reg, rpy6=rpy, ping_off=off)
        out = []
        info = lambda: _struct(c.mosaic_register_info())
        for sums in (False, True):                           # the peaks decided on the device; the tables downloaded and decided on the host
            r = c.mosaic_register(ids, p, pairs, want_sums=sums, **kw)
            out.append([list(r) if sums else r, info()])
            r = c.mosaic_register_segments(ids, p, pairs, REG_SEG_PINGS, want_sums=sums, **kw)
            out.append([list(r) if sums else r, info()])
            segs = r[0] if sums else r
            r = c.mosaic_register_segments_yaw(ids, p, pairs, REG_SEG_PINGS, yaw=yaw, want_sums=sums, **kw)
            out.append([list(r) if sums else r, info()])
            segs_yaw = r[0] if sums else r
            r = c.mosaic_register_segments_pyr(ids, p, pairs, REG_SEG_PINGS, pyr=pyr, want_sums=sums, **kw)
            out.append([list(r) if sums else r, info()])
            tables = r[1] if sums else None
        out.append(list(c.mosaic_register_edges(ids, p, pairs, segs, rpy6=rpy, ping_off=off)))
        ep = capi.reg_edge_yaw_params_default()
        ep.fan = yaw
        out.append(list(c.mosaic_register_edges_yaw(ids, p, pairs, segs_yaw, edge_params=ep, rpy6=rpy, ping_off=off)))
        S = 2 * REG_RADIUS + 1                               # the top-level tables of the pyramid rows once more, through the peak entry
        top = np.ascontiguousarray(tables[:, :S * S])
        out.append([c.mosaic_register_peaks(top, REG_RADIUS, max(1, REG_MIN_CELLS >> 2), 2 * p.cell), info()])
        return out

    return Scenario("register", make, run,
                    ("dsss_mosaic_bounds", "dsss_mosaic_register", "dsss_mosaic_register_segments", "dsss_mosaic_register_segments_yaw",
                     "dsss_mosaic_register_segments_pyr", "dsss_mosaic_register_edges", "dsss_mosaic_register_edges_yaw", "dsss_mosaic_register_peaks",
                     "dsss_mosaic_register_info"))


# ---------------------------------------------------------------- transport
TRANSPORT_CASE, TRANSPORT_RANK = (3, 4), 1        # feature_transport_ref.SPLITS' smallest: three frames over four ranks, rank 1 owns frame 0


def _transport():
    """test_gpu_feature_transport.py's gather with the frames of feature_transport_ref.design_frames: round 0 through the host-callback
    transport, round 1 through the device-callback transport, each with the matcher straight behind over own and gathered frames"""
    from tests import feature_transport_ref as R
    F, W = TRANSPORT_CASE

    @functools.lru_cache(maxsize=None)
    def inputs(K):
        orc = _orc()
        return [R.design_frames(orc, TRANSPORT_CASE, rnd, K, False) for rnd in (0, 1)]

    def make(new_ctx):
        c = new_ctx(8)
        mp, op, mt, pg = c.default_params()
        op.nfeatures, op.nlevels = 100, 2                    # the small context of the transport tests: K = 192
        c.set_params(orb=op, match=mt)
        K = R.capacity(c.pack_bytes(), False)
        inputs(K)
        return dict(ctx=c, K=K)

    def run(st):
        from tests.test_gpu_feature_transport import _Peers, _read, _set, _set_geometry
        c, K = st["ctx"], st["K"]
        nb = c.pack_bytes()
        lo, hi = R.block(F, TRANSPORT_RANK, W)
        out = []
        for rnd, frames in enumerate(inputs(K)):
            for f in range(F):
                (_set(c, f, frames[f], False) if lo <= f < hi else _set_geometry(c, f, frames[f]))
            peers = _Peers(c, TRANSPORT_RANK, W, R.gathered(frames, F, W, K, False, 0), device=(rnd == 1))
            c.features_allgather(F)
            pairs = R.MATCH_PAIRS[TRANSPORT_CASE][rnd]
            c.match_pairs([a for a, _ in pairs], [b for _, b in pairs])
            out.append([[_read(c, f, False) for f in range(F)], [_record(R.record_at(peers.own, F, W, f, nb), K, False) for f in range(lo, hi)], peers.calls, list(c.comm_stats()),
                        [c.frame_owner(F, f) for f in range(F)],
                        [[c.pair_is_active(k), list(c.match_dir(k, 0)), list(c.match_dir(k, 1)), c.match_rows(k), c.match_kp7(k)] for k in range(len(pairs))]])
            c.comm_destroy()
        return out

    return Scenario("transport", make, run,
                    ("dsss_set_params", "dsss_features_pack_bytes", "dsss_comm_init_callback", "dsss_comm_init_device_callback", "dsss_features_allgather",
                     "dsss_comm_stats", "dsss_comm_frame_owner", "dsss_comm_destroy", "dsss_features_set", "dsss_match_pairs", "dsss_match_get_dir"))


# ---------------------------------------------------------------- lifecycle
LIFECYCLE_NFEATURES = (500, 1500, 400)            # three values of kcap: test_gpu_ctx_buffers.py's small ORB configuration and the two of its kcap test


def _lifecycle():
    """test_gpu_ctx_buffers.py::test_create_use_destroy_twenty_times at a count of three: create, set_params that changes kcap, extract,
    match, destroy.  The profile entries ride along: launch counts are results, times are not."""
    @functools.lru_cache(maxsize=None)
    def inputs():
        from tests.helpers import survey_frame
        return survey_frame(640, 400, 9, hot=False)

    def make(new_ctx):
        inputs()
        return dict(new_ctx=new_ctx)

    def run(st):
        raw, pose, alt, gr = inputs()
        out = []
        for nf in LIFECYCLE_NFEATURES:
            c = st["new_ctx"](2)
            try:
                op = c.default_params()[1]
                op.nfeatures = nf; op.nlevels = 4
                c.set_params(orb=op)
                c.profile(True)
                c.frame_set(0, raw, 640, 400, pose, alt, gr); c.frame_set(1, raw, 640, 400, pose, alt, gr)
                c.extract_many([0, 1])
                c.match_pairs([0], [1])
                c.lc_solve_all()
                launches = [v[1] for v in c.profile_get().values()]
                c.profile_reset()
                after = [v[1] for v in c.profile_get().values()]
                c.profile(False)
                out.append([list(c.features_get(0)), c.frame_bbox(1), list(c.match_total()), c.match_rows(0), launches, after])
            finally:
                c.close()
        return out

    return Scenario("lifecycle", make, run,
                    ("dsss_set_params", "dsss_frame_set_typed", "dsss_extract_many", "dsss_match_pairs", "dsss_lc_solve_all", "dsss_features_get", "dsss_destroy",
                     "dsss_profile_enable", "dsss_profile_get", "dsss_profile_get_work", "dsss_profile_reset"))


SCENARIOS = collections.OrderedDict((s.name, s) for s in (
    _pipeline("pipeline_a"), _pipeline("pipeline_b"), _frames_again(), _features_and_match(), _lc_and_tri(), _pg_edges(), _pg_parts(), _mosaic(),
    _register(), _transport(), _lifecycle()))

# ---------------------------------------------------------------- what no scenario drives, and why
_HOST = "host arithmetic without a context: no stream to lag behind, no state to share"
EXEMPT = {
    "dsss_mask_params_default": "parameter defaults", "dsss_orb_params_default": "parameter defaults", "dsss_match_params_default": "parameter defaults",
    "dsss_pg_params_default": "parameter defaults", "dsss_pg_gate_params_default": "parameter defaults", "dsss_gain_params_default": "parameter defaults",
    "dsss_comp_params_default": "parameter defaults", "dsss_footprint_params_default": "parameter defaults", "dsss_reg_params_default": "parameter defaults",
    "dsss_reg_edge_params_default": "parameter defaults", "dsss_reg_yaw_params_default": "parameter defaults",
    "dsss_reg_edge_yaw_params_default": "parameter defaults", "dsss_reg_pyr_params_default": "parameter defaults",
    "dsss_strerror": "a table of strings", "dsss_last_error": "reads the context's last message; never held back",
    "dsss_create": "there is no stream to hold back before it; the lifecycle scenario creates three contexts",
    "dsss_stream": "the hold-back itself is built on it; never held back",
    "dsss_raw_type_size": _HOST, "dsss_mosaic_grid": _HOST, "dsss_gain_band": _HOST, "dsss_mosaic_gain_table": _HOST, "dsss_mosaic_gain_table_banded": _HOST,
    "dsss_mosaic_comp_rank": _HOST, "dsss_mosaic_fill_host": _HOST, "dsss_mosaic_footprint_steps": _HOST, "dsss_mosaic_register_peak": _HOST,
    "dsss_register_edge": _HOST, "dsss_register_rotate_rows": _HOST, "dsss_register_yaw_peak": _HOST, "dsss_register_edge_yaw": _HOST,
    "dsss_register_pyr_step": _HOST,
    "dsss_host_quadtree": "host twin", "dsss_host_pg_solve": "host twin", "dsss_host_pg_solve_local": "host twin", "dsss_host_pg_solve_parts": "host twin",
    "dsss_host_pg_bins_profile": "host twin",
    "dsss_comm_unique_id": "RCCL only: one process per GPU", "dsss_comm_init": "RCCL only: one process per GPU",
    "dsss_frame_set": "one line that forwards to dsss_frame_set_typed with DSSS_RAW_F64", "dsss_frames_set": "one line that forwards to dsss_frames_set_typed",
}


def declared_entries(header_text):
    """the functions include/dsss.h declares: every `dsss_name(` at the start of a declaration (a return type in front, no `(*` of a callback type)"""
    text = re.sub(r"/\*.*?\*/", " ", header_text, flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:const\s+)?(?:int|void|size_t|char)\s*\*?\s*(dsss_\w+)\s*\(", text, flags=re.M)))


def covered_entries():
    out = set()
    for s in SCENARIOS.values():
        out.update(s.entries)
    return out

"""GPU: the buffers a context keeps between calls (dsss_buf and the families of diasss_amd/csrc/dsss_internal.h) through
"first allocation", "regrowth with a queued reader behind it" and "below capacity".

Every test drives ONE context through small -> larger -> small again and compares every output, bit for bit, with the same call on a
FRESH context of the same parameters: whatever a regrown, a reused or a too-large buffer could change would show as a differing byte.
Inputs are the smallest the tests of each entry already use.  No test provokes an allocation failure (that path: test_ctx_buffers_cpu.py)."""
import numpy as np
import pytest

from tests.helpers import result_bytes as _bytes          # the bytes of a result: arrays (NaNs by their bits), scalars, nested tuples and lists

pytestmark = pytest.mark.gpu


def _ctx(max_frames=4, orb=None):
    from diasss_amd import capi
    c = capi.Context(max_frames=max_frames)
    if orb is not None:
        c.set_params(orb=orb)
    return c


def _run_sequence(steps, fresh, make):
    """steps on one context made by make(), then each step alone on a context of its own: the same bytes"""
    c = make()
    try:
        kept = [_bytes(s(c)) for s in steps]
    finally:
        c.close()
    for k, s in enumerate(fresh if fresh is not None else steps):
        f = make()
        try:
            alone = _bytes(s(f))
        finally:
            f.close()
        assert len(alone) > 0 and alone == kept[k], "step %d differs from a fresh context's" % k
    return kept


# ---------------------------------------------------------------- mosaic_buf
def test_mosaic_buffer_small_large_small():
    """the two-leg fixture of test_gpu_mosaic.py; a coarse cell, a cell four times finer (a larger mosaic_buf; the call is issued behind a
    render that is still queued: no dsss_sync in between), the coarse one again -- render, consistency map and registration"""
    from diasss_amd import capi
    from tests import helpers as H
    legs = []
    for leg, (N, M) in enumerate(H.MOSAIC_SIZES):
        pose, alt, gr = H.track(N, M, leg, seed=9)
        legs.append((np.random.default_rng(leg).rayleigh(1.0, (N, M)) * 100.0, N, M, pose, alt, gr))

    def make():
        c = _ctx()
        for i, L in enumerate(legs):
            c.frame_set(i, *L)
        c.extract_many([0, 1])
        return c

    def step(cell, queued_first):
        def run(c):
            p = capi.mosaic_grid(c.mosaic_bounds([0, 1]), cell)
            if queued_first:
                c.mosaic_render([0, 1], capi.mosaic_grid(c.mosaic_bounds([0, 1]), 4 * cell), download=False)      # stays queued: no synchronisation
            out = [c.mosaic_render([0, 1], p), c.mosaic_consistency([0, 1], p), c.mosaic_register([0, 1], p, [(0, 1)], want_sums=True)]
            assert out[0][1].sum() > 10000
            return out
        return run

    coarse, fine = 0.8, 0.2
    kept = _run_sequence([step(coarse, False), step(fine, True), step(coarse, False)], [step(coarse, False), step(fine, False), step(coarse, False)], make)
    assert kept[0] == kept[2] and len(kept[1]) > 4 * len(kept[0])


# ---------------------------------------------------------------- pgr_buf, the solver arena, pg_stage
def test_report_and_gated_solve_small_large_small(orc):
    """_small_graph of test_gpu_pg_report.py (9 edges), a graph on the same chain with about four times the edges, the small one again"""
    from tests.helpers import pg_edge as _edge, pg_small_graph as _small_graph
    dr, small = _small_graph(orc)
    rng = np.random.default_rng(41)
    ends = [tuple(int(v) for v in rng.choice(len(dr), 2, replace=False)) for _ in range(36)]
    large = np.concatenate([_edge(orc, dr, a, b, rng.uniform(-0.2, 0.2)) for a, b in ends])

    def step(edges):
        def run(c):
            poses, stats = c.posegraph_solve_edges(dr, edges)
            return [poses, stats, c.posegraph_edge_report(dr, edges, poses), c.posegraph_solve_gated(dr, edges)]
        return run

    kept = _run_sequence([step(small), step(large), step(small)], None, lambda: _ctx(2))
    assert kept[0] == kept[2] and kept[0] != kept[1]


# ---------------------------------------------------------------- pg_edges_host, pg_ab_host, pg_stage, lcs, the pair families
def test_select_and_solve_few_many_few(orc):
    """two pair sets of helpers.lc_cases' "select" group: few loop closures, many, few -- the selected edge list, the poses and the stats"""
    from tests.helpers import LC_M, LC_N, lc_cases
    g = lc_cases(orc, 0)["select"]
    many = g["lists"]
    few = [(many[0][0], many[0][1], many[0][2][:6])]

    def make():
        c = _ctx()
        for f, (pose, alt, gr) in enumerate(g["frames"]):
            c.frame_set(f, None, LC_N, LC_M, pose, alt, gr)
        return c

    def step(lists):
        def run(c):
            c.lc_solve_pairs([l[0] for l in lists], [l[1] for l in lists], [l[2] for l in lists])
            edges = c.posegraph_select(3)
            poses, rpy, stats = c.posegraph_solve(3, 3 * LC_N)
            return [edges, poses, rpy, stats]
        return run

    probe = make()
    try:
        n_few = len(step(few)(probe)[0]); n_many = len(step(many)(probe)[0])
    finally:
        probe.close()
    assert 0 < n_few < n_many
    kept = _run_sequence([step(few), step(many), step(few)], None, make)
    assert kept[0] == kept[2] and kept[0] != kept[1]


# ---------------------------------------------------------------- ex_scratch, ex_pinned, a frame's images and pack
def test_extraction_small_large_small():
    """the small ORB configuration of test_extract_small_orb_config_and_reuse (500 features, 4 levels) at 640 x 400, a 1000 x 512 frame in
    the same slot (ex_scratch and ex_pinned regrow, the frame's own buffers are rebuilt), the small frame again"""
    from tests.helpers import survey_frame as _frame
    small = _frame(640, 400, 9, hot=False); large = _frame(1000, 512, 5, hot=False)

    def make():
        c = _ctx()
        op = c.default_params()[1]
        op.nfeatures = 500; op.nlevels = 4
        c.set_params(orb=op)
        return c

    def step(fr):
        def run(c):
            raw, pose, alt, gr = fr
            c.frame_set(1, raw, raw.shape[0], raw.shape[1], pose, alt, gr)
            n = c.extract(1)
            assert n > 50
            return [np.int64(n), c.features_get(1), c.frame_bbox(1)]
        return run

    kept = _run_sequence([step(small), step(large), step(small)], None, make)
    assert kept[0] == kept[2] and kept[0] != kept[1]


# ---------------------------------------------------------------- the store family and desc128 under a changed kcap
def test_set_params_changes_kcap_after_the_store_exists():
    """extract (SIFT rows too, so that desc128 exists), change nfeatures so that kcap changes, extract again: equal to a fresh context of the
    new parameters -- the store and desc128 are rebuilt by the family rule"""
    from diasss_amd import capi
    from tests.helpers import survey_frame as _frame
    raw, pose, alt, gr = _frame(640, 400, 9, hot=False)

    def params(c, nfeatures):
        op = c.default_params()[1]
        op.nfeatures = nfeatures; op.nlevels = 4; op.descriptor = capi.DESC_SIFT128
        return op

    def extract(c):
        c.frame_set(0, raw, 640, 400, pose, alt, gr)
        n = c.extract(0)
        assert n > 50
        return [np.int64(n), c.features_get(0), c.features_get_sift(0)]

    c = _ctx()
    try:
        c.set_params(orb=params(c, 1500))
        first = _bytes(extract(c))
        c.set_params(orb=params(c, 400))              # kcap 1536 + 64 -> 448 + 64 ...: another stride, every store buffer is rebuilt
        second = _bytes(extract(c))
        c.set_params(orb=params(c, 1500))             # ... and back up
        third = _bytes(extract(c))
    finally:
        c.close()
    for nf, got in ((400, second), (1500, first)):
        f = _ctx()
        try:
            f.set_params(orb=params(f, nf))
            assert _bytes(extract(f)) == got, "nfeatures %d differs from a fresh context's" % nf
        finally:
            f.close()
    assert third == first and second != first


# ---------------------------------------------------------------- destruction order
def _twenty_contexts():
    """the body of the test below, run in a process of its own (python -c)"""
    from tests.helpers import survey_frame as _frame
    raw, pose, alt, gr = _frame(640, 400, 9, hot=False)

    def use():
        c = _ctx(2)
        try:
            op = c.default_params()[1]
            op.nfeatures = 500; op.nlevels = 4
            c.set_params(orb=op)
            c.frame_set(0, raw, 640, 400, pose, alt, gr); c.frame_set(1, raw, 640, 400, pose, alt, gr)
            c.extract_many([0, 1])
            c.match_pairs([0], [1])
            c.lc_solve_all()
            return _bytes([c.features_get(0), c.frame_bbox(1), np.array(c.match_total()), c.match_rows(0)])
        finally:
            c.close()

    first = use()
    for _ in range(19):
        use()
    assert use() == first, "the 21st context's result differs from the first's"
    print("twenty contexts ok: %d result bytes" % len(first))


def test_create_use_destroy_twenty_times():
    """create, use (extract, match, loop closures) and destroy a context 20 times in ONE process, then use one more: the last result equals
    the first and the process ends with status 0 -- the test is about that process, so it starts one.  Guards the order of dsss_destroy:
    the buffers' destructors run at `delete`, after the streams are gone."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", "from tests.test_gpu_ctx_buffers import _twenty_contexts; _twenty_contexts()"],
                         cwd=root, capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr[-2000:])
    assert out.returncode == 0
    assert "twenty contexts ok" in out.stdout

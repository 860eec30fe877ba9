"""The pipelined kernel of the binned subtrees (pg_factor_subtree_kernel, diasss_amd/csrc/dsss_pg_bins.hip) against its serial form
(DSSS_PG_BINS=serial), bit for bit, on graphs that reach every branch of its column pipeline.  A race in a kernel like this shows as differing
bits long before it shows as anything else, so every case is solved three times under the default and once under the serial switch, and all four
results must agree in the bytes of the poses and of the statistics.

What a case reaches is not taken on trust: the host analysis (dsss_host_pg_bins_profile: the one-graph analysis with the device solve's bin
cost, which is what dsss_pg.hip runs below 1 500 separators) is run on the case's reduced graph -- separators as pg_solve::separators picks
them -- and the test asserts from its tables that the branch is there.  The kernel's constants as the tests name them: PG_NIDX = 4 map entries
per thread held in registers for the next column, PG_PCH = 42 updates staged ahead per column, 42 blocks the binning limit."""
import ctypes as C

import numpy as np
import pytest

from tests import pg_paths_ref as P
from tests.pg_step_ref import _reduced

pytestmark = pytest.mark.gpu

PG_NIDX, PG_PCH, MAX_BLOCKS = 4, 42, 42
PROFILE = "bins cols one_col_bins noupd_after_upd fresh notfresh max_nonfresh max_blocks max_roots consecutive_U max_cols max_T".split()


@pytest.fixture(scope="module")
def ctx():
    from diasss_amd import capi
    c = capi.Context(max_frames=2)
    yield c
    c.close()


def _profile(dr, e):
    from diasss_amd import capi
    ns, ea, eb, cx, cy = _reduced(dr, e)
    assert ns < 1500, "above 1 500 separators the device analyses by parts: the one-graph profile would not be its analysis"
    out = np.zeros(12, np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert capi.lib().dsss_host_pg_bins_profile(ns, p(ea), p(eb), len(ea), p(cx), p(cy), p(out)) == 0
    return dict(zip(PROFILE, out.tolist()))


def _four_solves(ctx, dr, e, monkeypatch):
    """three solves under the default and one under the serial switch: all four the same bytes"""
    runs = []
    for k in range(4):
        if k == 3:
            monkeypatch.setenv("DSSS_PG_BINS", "serial")
        X, st = ctx.posegraph_solve_edges(dr, e)
        runs.append((X.tobytes(), np.asarray(st).tobytes(), np.asarray(st).copy()))
    monkeypatch.delenv("DSSS_PG_BINS")
    for k in (1, 2, 3):
        assert runs[k][0] == runs[0][0], "poses of solve %d (%s) differ from the first" % (k, "serial" if k == 3 else "default")
        assert runs[k][1] == runs[0][1], "statistics of solve %d (%s) differ from the first" % (k, "serial" if k == 3 else "default")
    return runs[0][2]


# name -> (builder(orc) -> (dr, edges, ...), DSSS_PG_BIN_COST or None, what the analysis must show)
BRANCHES = {
    # a clique of 40: a bin of one column; columns with more sources than the register budget; a root whose update matrix takes terms from consecutive columns
    "clique_40": (lambda o: P._clique(o, 40), None,
                  lambda s: s["one_col_bins"] >= 1 and s["max_nonfresh"] > PG_NIDX and s["consecutive_U"] >= 2 and s["fresh"] >= 1),
    # a clique of 42: a column of 42 blocks, the binning limit (threads 250 and 251 own a row of it as well as the right-hand side, thread 250 also the pivot)
    "clique_42": (lambda o: P._clique(o, 42), None, lambda s: s["max_blocks"] == MAX_BLOCKS),
    # the band: columns without updates directly after columns with updates; predecessors that are a source and one that is not; bins with several roots
    "band": (P._band, None, lambda s: s["noupd_after_upd"] >= 1 and s["fresh"] >= 1 and s["notfresh"] >= 1 and s["max_roots"] >= 2 and s["consecutive_U"] >= 2),
    # closures between random poses: many predecessors that are no source, many roots per bin
    "wild_variances": (P._wild_variances, None, lambda s: s["notfresh"] >= 5 and s["max_roots"] >= 2 and s["noupd_after_upd"] >= 1),
    # the band as ONE bin: a column with more sources than one staged chunk (the rest is staged in place)
    "band_one_bin": (P._band, 1e12, lambda s: s["bins"] == 1 and PG_PCH < s["max_nonfresh"] <= 2 * PG_PCH),
    # the hub as ONE bin: a column with 300 sources, several chunks staged in place
    "hub_one_bin": (P._hub, 1e12, lambda s: s["bins"] == 1 and s["max_nonfresh"] > 3 * PG_PCH),
}


@pytest.mark.parametrize("name", list(BRANCHES))
def test_branch_of_the_column_pipeline_has_the_serial_bits(orc, ctx, monkeypatch, name):
    from diasss_amd import capi
    build, cost, claims = BRANCHES[name]
    dr, e = build(orc)[:2]
    e = P._convert(capi, e)
    if cost is not None:
        monkeypatch.setenv("DSSS_PG_BIN_COST", repr(cost))
    s = _profile(dr, e)
    print(name, s)
    assert claims(s), "the analysis does not show what this case is for: %s" % s
    st = _four_solves(ctx, dr, e, monkeypatch)
    assert st[0] >= 1 and np.isfinite(st[2]) and st[2] <= st[1]


def test_failed_pivot_and_a_clean_solve_after_it(orc, ctx, monkeypatch):
    """factor_fails of tests/pg_paths_ref.py: every trial's factorisation fails (*fail = 1), nothing is accepted; the same bytes from both forms, and
    the clean solve after it on the same context has the bytes of a fresh context's"""
    from diasss_amd import capi
    dr, e, _p = P.build(orc, "factor_fails")
    st = _four_solves(ctx, dr, e, monkeypatch)
    assert st[0] == 0 and st[1] == st[2], "factor_fails accepted a trial: %s" % st
    dr, e, _p = P._clean(orc)
    X, st = ctx.posegraph_solve_edges(dr, e)
    fresh = capi.Context(max_frames=2)
    try:
        Xf, stf = fresh.posegraph_solve_edges(dr, e)
    finally:
        fresh.close()
    assert X.tobytes() == Xf.tobytes() and np.asarray(st).tobytes() == np.asarray(stf).tobytes()
    assert st[0] >= 1


@pytest.fixture(scope="module")
def lawnmower():
    from tests.test_gpu_configs import _lawnmower_graph
    dr, _gt, e = _lawnmower_graph(30, 1000, 3000, 11)          # 30 000 poses, 3 000 closures: the ordinary case
    return dr, e


@pytest.mark.parametrize("parts", [0, 3])
def test_lawnmower_graph_has_the_serial_bits(ctx, monkeypatch, lawnmower, parts):
    dr, e = lawnmower
    ctx.set_pg_partitions(parts)
    try:
        st = _four_solves(ctx, dr, e, monkeypatch)
    finally:
        ctx.set_pg_partitions(0)
    assert st[0] >= 1 and np.isfinite(st[2]) and st[2] < st[1]

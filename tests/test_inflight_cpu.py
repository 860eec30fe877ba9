"""No GPU: the claims of the scenario table of tests/inflight_cases.py that tests/test_gpu_inflight.py rests on.

  coverage         every function include/dsss.h declares is driven by a scenario or exempt for a stated reason: an entry added later
                   without a scenario fails here;
  byte comparison  the helper that compares two nested results reports one flipped bit anywhere, and takes NaNs by their bits;
  pg_parts         its graph is handed to the analysis BY PARTS on the device (the rule of pg_analyse restated on the reduced graph: the limits
                   of that proof are stated at inflight_cases.pg_parts_plan), the next smaller one is not, and the host twin's tables of the
                   parts hold binned columns and a front of more than one panel."""
import ctypes as C
import os

import numpy as np

from tests import inflight_cases as S
from tests import pg_paths_ref as P
from tests.helpers import first_difference, result_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_entry_is_driven_or_exempt():
    with open(os.path.join(ROOT, "include", "dsss.h")) as f:
        declared = set(S.declared_entries(f.read()))
    assert len(declared) >= 117 and {"dsss_create", "dsss_strerror", "dsss_stream", "dsss_raw_type_size", "dsss_mosaic_register_segments_pyr"} <= declared
    driven = S.covered_entries()
    assert not driven - declared, "the table names entries the header does not declare: %s" % sorted(driven - declared)
    assert not set(S.EXEMPT) - declared, "exemptions for entries the header does not declare: %s" % sorted(set(S.EXEMPT) - declared)
    assert not driven & set(S.EXEMPT), "both driven and exempt: %s" % sorted(driven & set(S.EXEMPT))
    missing = declared - driven - set(S.EXEMPT)
    assert not missing, "entries without a scenario (add one to tests/inflight_cases.py, or an exemption with its reason): %s" % sorted(missing)
    assert all(isinstance(r, str) and len(r) > 8 for r in S.EXEMPT.values())
    # what is exempt takes no context, or is one of the four calls the hold-back leaves alone, or forwards in one line
    for name in S.EXEMPT:
        assert (name.endswith("_default") or name.startswith("dsss_host_") or name in ("dsss_strerror", "dsss_last_error", "dsss_create", "dsss_stream",
                "dsss_comm_unique_id", "dsss_comm_init", "dsss_frame_set", "dsss_frames_set") or S.EXEMPT[name] == S._HOST), name


def test_the_table_has_the_scenarios_and_they_name_their_entries():
    assert list(S.SCENARIOS) == ["pipeline_a", "pipeline_b", "frames_again", "features_and_match", "lc_and_tri", "pg_edges", "pg_parts", "mosaic", "register",
                                 "transport", "lifecycle"]
    for s in S.SCENARIOS.values():
        assert callable(s.make) and callable(s.run) and len(s.entries) == len(set(s.entries)) > 0
    a, b = S.PIPELINES["pipeline_a"], S.PIPELINES["pipeline_b"]
    assert (a["N"], a["M"]) != (b["N"], b["M"]) and a["nfeatures"] != b["nfeatures"] and a["F"] != b["F"] and a["on_device"] != b["on_device"]


def test_one_bit_anywhere_in_a_nested_result_is_reported():
    rec = np.zeros(3, [("a", "<i4"), ("v", "<f8", (2,))])
    base = [np.arange(12, dtype=np.float64).reshape(3, 4), (np.uint8(7), [np.array([np.nan, 1.0]), 3, 2.5, None, True]), rec, []]

    def copy(x):
        if isinstance(x, (list, tuple)):
            return type(x)(copy(v) for v in x)
        return x.copy() if isinstance(x, np.ndarray) else x

    assert first_difference(base, copy(base)) is None and result_bytes(base) == result_bytes(copy(base))
    # one bit in every array leaf, found at its path
    for path, leaf in (("result[0]", lambda r: r[0]), ("result[1][1][0]", lambda r: r[1][1][0]), ("result[2]", lambda r: r[2])):
        other = copy(base)
        raw = leaf(other).view(np.uint8).reshape(-1)
        for byte in (0, len(raw) - 1):
            raw[byte] ^= 1
            d = first_difference(base, other)
            assert d is not None and d.startswith(path + ":") and "1 of" in d and "byte %d" % byte in d, d
            assert result_bytes(base) != result_bytes(other)
            raw[byte] ^= 1
        assert first_difference(base, other) is None
    # scalars, None, lengths
    for k, v in ((1, 4), (2, 2.5000000000000004), (3, 0), (4, False)):
        other = copy(base)
        other[1][1][k] = v
        d = first_difference(base, other)
        assert d is not None and d.startswith("result[1][1][%d]" % k), d
    other = copy(base); other[3] = [np.zeros(0)]
    assert first_difference(base, other).startswith("result[3]")
    # NaNs by their bits: the same NaN is equal, another payload or sign is not, and -0.0 is not 0.0
    q = np.array([np.nan]); q2 = q.copy(); q2.view(np.uint64)[0] ^= 1
    assert first_difference([q], [q.copy()]) is None
    assert first_difference([q], [q2]) is not None and first_difference([q], [-q]) is not None
    assert first_difference([np.array([0.0])], [np.array([-0.0])]) is not None


def test_pg_parts_graph_is_analysed_by_parts():
    from diasss_amd import capi
    from tests.test_pg_symbolic_host import _values
    dr, e = S.pg_parts_graph()
    ns, ea, eb, cx, cy = P.reduced_graph(dr, e)
    K, kept, costs = S.pg_parts_plan(ns, ea, eb)
    print("pg_parts: %d poses, %d closures, %d separators; %d parts wanted, boundaries kept %s, closures across each boundary tried %s" % (
        len(dr), len(e), ns, K, kept, costs))
    assert ns >= S.PG_PARTS_MIN_SEPARATORS and len(ea) > ns - 1
    assert K >= 2 and len(kept) == len(costs) >= 1 and max(costs) <= S.PG_PARTS_CUT_MAX, "the device would analyse this graph as one"
    # the smallest of its family in steps of ten closures: the one before stays below the threshold
    dr0, e0 = S.pg_parts_graph(S.PG_PARTS_GRAPH[2] - 10)
    ns0, ea0, eb0, _, _ = P.reduced_graph(dr0, e0)
    assert ns0 < S.PG_PARTS_MIN_SEPARATORS and S.pg_parts_plan(ns0, ea0, eb0)[1] == []
    # a survey of few long legs of the same size is NOT analysed by parts: why the legs are short (the cut rule, not the size, decides)
    from tests.test_gpu_configs import _lawnmower_graph
    dr4, _gt, e4 = _lawnmower_graph(4, 1000, 960, 7)
    ns4, ea4, eb4, _, _ = P.reduced_graph(dr4, e4)
    assert ns4 >= S.PG_PARTS_MIN_SEPARATORS and S.pg_parts_plan(ns4, ea4, eb4)[1] == []
    # the host twin's tables, analysed by the same number of parts and as one graph: bins, and a front of more than one panel
    aval, rhs = _values(ns, ea, eb, 5)
    x = np.zeros((ns, 6)); st = np.zeros(8, np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = capi.lib().dsss_host_pg_solve_parts(ns, p(ea), p(eb), len(ea), p(cx), p(cy), len(kept) + 1, p(np.ascontiguousarray(aval)),
                                             p(np.ascontiguousarray(rhs)), p(x), p(st))
    one = P.twin_stats(dr, e)
    print("pg_parts: twin by parts %s, as one graph %s (nnzL, fronts, panels, levels, front doubles, comm, binned columns, largest front)" % (st.tolist(), one.tolist()))
    assert rc == 0 and np.isfinite(x).all()
    for tables in (st, one):
        assert tables[6] > 0, "no binned columns"
        assert tables[2] > tables[1] > 1, "no front of more than one panel"


def test_binding_releases_the_gil():
    """the threads of arm B run at the same time only because ctypes.CDLL drops the GIL around a call (PyDLL keeps it)"""
    from diasss_amd import capi
    L = capi.lib()
    assert isinstance(L, C.CDLL) and not isinstance(L, C.PyDLL)

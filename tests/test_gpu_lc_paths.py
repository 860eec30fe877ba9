"""GPU parity of lc_kernel and tri_kernel (dsss_lc.hip) on rows that leave the LM by every exit it has: tests.helpers.lc_cases, checked on
the oracle alone by tests/test_lc_paths_cpu.py.

Which row is compared how is decided on the oracle (helpers.lc_reference): a row whose path survives a one-ulp move of both slant ranges
and of the target ping's x (seven runs, same counters, same non-finite pattern) is PATH-STABLE and compared in full -- iteration count,
non-finite pattern, and every output within max(floor, 16 x the spread of the seven runs), the floors being the project's tolerances
(rel 1e-9, var and err1 1e-6 relative, score 1e-6; triangulation 1e-9).  The others are knife-edge (the oracle cannot decide them: the
device's libm and glibc differ in the last ulp) and are held to the NaN pattern of var, a finite rel and err1 <= err0.  Every test prints
the largest deviation it saw next to the largest it would have allowed."""
import numpy as np
import pytest

from tests.helpers import LC_M, LC_N, LC_SEAM_N, _nonfinite_code, _spread, lc_cases, lc_long_flip_list, lc_reference, lc_seam_case, tri_reference

pytestmark = pytest.mark.gpu

GROUPS = ("consistent-opposite", "consistent-same", "noisy-slant", "wrong-flip", "tiny-slant", "long-slant", "zero-slant", "zero-baseline",
          "tilted", "mid-list-flip", "mid-list-flip-src", "edges", "ragged", "pairs", "select")
TRI_GROUPS = ("noisy-slant", "wrong-flip", "tiny-slant", "zero-slant", "zero-baseline")


@pytest.fixture(scope="module")
def ctx():
    from diasss_amd import capi
    c = capi.Context(max_frames=4)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases(orc):
    return lc_cases(orc, 0)


def _load(ctx, frames):
    for f, (pose, alt, gr) in enumerate(frames):
        ctx.frame_set(f, None, LC_N, LC_M, pose, alt, gr)


def _within(g, o, tol, what, stat):
    """same non-finite values in the same places, finite ones within tol (element-wise); stat collects (deviation, allowance)"""
    g = np.asarray(g, np.float64); o = np.asarray(o, np.float64); tol = np.broadcast_to(tol, o.shape)
    assert (_nonfinite_code(g) == _nonfinite_code(o)).all(), "%s: non-finite pattern differs" % what
    fin = np.isfinite(o)
    if fin.any():
        dev = np.abs(g[fin] - o[fin])
        k = int(np.argmax(dev / tol[fin]))
        if what not in stat or dev[k] / tol[fin][k] > stat[what][0] / stat[what][1]:
            stat[what] = (float(dev[k]), float(tol[fin][k]))
        assert (dev <= tol[fin]).all(), "%s: deviation %.3e where %.3e is allowed" % (what, dev[k], tol[fin][k])


def _check_lc(name, g, ref, stat):
    o, st, sp = ref["lcs"], ref["stable"], ref["spread"]
    assert len(g) == len(o)
    # every row, knife-edge ones included
    assert (np.isnan(g["var"]) == np.isnan(o["var"])).all(), name
    assert np.isfinite(g["rel"]).all(), name
    ke = ~st
    assert (g["err1"][ke] <= g["err0"][ke]).all(), name
    # path-stable rows
    gs, os_ = g[st], o[st]
    assert (gs["iters"] == os_["iters"]).all(), (name, gs["iters"], os_["iters"])
    _within(gs["rel"], os_["rel"], np.maximum(1e-9, 16 * sp["rel"][st]), "rel", stat)
    _within(gs["var"], os_["var"], np.maximum(1e-6 * np.abs(np.nan_to_num(os_["var"])), 16 * sp["var"][st]), "var", stat)
    _within(gs["err1"], os_["err1"], np.maximum(1e-6 * np.abs(np.nan_to_num(os_["err1"], posinf=0.0)), 16 * sp["err1"][st]) + 1e-300, "err1", stat)
    _within(gs["score"], os_["score"], np.maximum(1e-6, 16 * sp["score"][st]), "score", stat)


def _report(name, stat):
    print("%-20s " % name + "  ".join("%s %.2e (allowed %.2e)" % (k, v[0], v[1]) for k, v in stat.items()))


@pytest.mark.parametrize("name", GROUPS)
def test_lc_solve_group(ctx, orc, cases, name):
    """dsss_lc_solve, list by list, against orc_lc_solve"""
    g = cases[name]
    _load(ctx, g["frames"])
    stat = {}
    for li, (s, t, k) in enumerate(g["lists"]):
        if not len(k):
            continue
        got = ctx.lc_solve(s, t, k)
        ref = lc_reference(orc, g["frames"], s, t, k, key=(name, li))
        _check_lc((name, li), got, ref, stat)
        if name == "zero-baseline":
            # A non-finite score is reached by knife-edge rows only (helpers.lc_cases), so no row with one gets the full comparison.  What
            # holds for every row that pairs a point with itself, on any libm: both geo samples are the same bits, ini = 0 exactly, and
            # the score is 0 / fin - 2 = NaN (fin = 0) or exactly -2.  Whether fin is 0 is the last ulp of the final yaw: reported, not asserted.
            same = g["same_point"]
            sc = got["score"][same]
            assert (np.isnan(sc) | (sc == -2.0)).all(), sc
            print("zero-baseline: score NaN on %d of %d same-point rows (oracle %d), same rows as the oracle: %s"
                  % (np.isnan(sc).sum(), same.sum(), np.isnan(ref["lcs"]["score"][same]).sum(), (np.isnan(sc) == np.isnan(ref["lcs"]["score"][same])).all()))
    _report(name, stat)


def test_lc_solve_pairs_straddling_wavefronts(ctx, orc, cases):
    """dsss_lc_solve_pairs over lists of 3, 0, 5, 1 and 7 rows of pairs (0,1), (0,2), (1,2), (2,1), (0,1): each wavefront (four problems) holds
    rows of two pairs with different frames and flip flags, one list is empty, one pair is reversed.  lc_get(p) = dsss_lc_solve of that
    list byte for byte, and the oracle within the rule above."""
    g = cases["pairs"]
    _load(ctx, g["frames"])
    lists = g["lists"]
    assert [len(l[2]) for l in lists] == [3, 0, 5, 1, 7] and [(l[0], l[1]) for l in lists] == [(0, 1), (0, 2), (1, 2), (2, 1), (0, 1)]
    ctx.lc_solve_pairs([l[0] for l in lists], [l[1] for l in lists], [l[2] for l in lists])
    got = [ctx.lc_get(p) for p in range(len(lists))]
    stat = {}
    for p, (s, t, k) in enumerate(lists):
        assert len(got[p]) == len(k)
        if not len(k):
            continue
        assert got[p].tobytes() == ctx.lc_solve(s, t, k).tobytes(), p
        _check_lc(("pairs", p), got[p], lc_reference(orc, g["frames"], s, t, k, key=("pairs", p)), stat)
    _report("pairs (one launch)", stat)


def _differs(a, b):
    return np.array([x.tobytes() != y.tobytes() for x, y in zip(a, b)])


def _lc_switch_mid_list(ctx, orc, cases, name, col):
    """the list of group `name`, whose yaw (of the pings in kp7 column col: 0 source, 3 target) crosses 2 pi / 3 at row `switch`"""
    g = cases[name]
    _load(ctx, g["frames"])
    s, t, k = g["lists"][0]; sw = g["switch"]
    pose = g["frames"][t if col == 3 else s][0]
    yaw = np.abs(pose[k[:, col].astype(int), 2])
    assert (yaw[:sw] < 2).all() and yaw[sw] > 2.2 and (yaw[sw + 1:sw + 9] < 2).all()
    alone = ctx.lc_solve(s, t, k)
    ctx.lc_solve_pairs([s], [t], [k])
    assert ctx.lc_get(0).tobytes() == alone.tobytes()
    ref = lc_reference(orc, g["frames"], s, t, k, key=(name, 0))
    stat = {}
    _check_lc(name, alone, ref, stat)
    tail = k[sw + 1:]
    g_tail = ctx.lc_solve(s, t, tail)
    r_tail = lc_reference(orc, g["frames"], s, t, tail, key=(name, "tail"))
    _check_lc(name + " tail", g_tail, r_tail, stat)
    d_dev = _differs(g_tail, alone[sw + 1:])
    d_orc = _differs(r_tail["lcs"], ref["lcs"][sw + 1:])
    assert (d_dev == d_orc).all() and d_orc[:8].all() and not d_orc[8:].any()
    _report(name, stat)


def test_sticky_flip_that_switches_on_mid_list(ctx, orc, cases):
    """the target's yaw crosses 2 pi / 3 at row `switch` of the list; the rows after it have the small yaw again and stay flipped
    (optimizer.cpp:650,700-703).  Stand-alone form = pairs form byte for byte; both = the oracle; and the rows behind the switch differ from what
    they give in a list that starts behind it exactly where the oracle's differ."""
    _lc_switch_mid_list(ctx, orc, cases, "mid-list-flip", 3)


def test_sticky_flip_that_switches_on_mid_list_source_side(ctx, orc, cases):
    """the same with the step in the SOURCE frame's yaw (flag bit 0): 24 rows, switch at row 12"""
    g = cases["mid-list-flip-src"]
    assert len(g["lists"][0][2]) == 24 and g["switch"] == 12
    _lc_switch_mid_list(ctx, orc, cases, "mid-list-flip-src", 0)


def _check_tri(got, ref, what, stat):
    """dsss_triangulate against tri_reference: the non-finite pattern on every row, path-stable rows within max(1e-9, 16 x spread)"""
    st = ref["stable"]
    assert got.shape == ref["out"].shape
    assert (np.isfinite(got) == np.isfinite(ref["out"])).all()
    _within(got[st], ref["out"][st], np.maximum(1e-9, 16 * ref["spread"][st]), what, stat)


@pytest.mark.parametrize("name", ("mid-list-flip", "mid-list-flip-src"))
def test_triangulate_sticky_flip_mid_list(ctx, orc, cases, name):
    """dsss_triangulate takes the sticky flags of its list as dsss_lc_solve does: the full list and the rows behind the switch alone, each
    against orc_triangulate, and the two device results differ on exactly the rows where the oracle's differ (the eight small-yaw rows)"""
    g = cases[name]
    _load(ctx, g["frames"])
    s, t, k = g["lists"][0]; sw = g["switch"]
    stat = {}
    full = ctx.triangulate(s, t, k)
    ref = tri_reference(orc, g["frames"], s, t, k, key=(name, 0))
    _check_tri(full, ref, "triangulate", stat)
    tail = k[sw + 1:]
    g_tail = ctx.triangulate(s, t, tail)
    r_tail = tri_reference(orc, g["frames"], s, t, tail, key=(name, "tail"))
    _check_tri(g_tail, r_tail, "triangulate tail", stat)
    d_dev = _differs(g_tail, full[sw + 1:])
    d_orc = _differs(r_tail["out"], ref["out"][sw + 1:])
    assert (d_dev == d_orc).all() and d_orc[:8].all() and not d_orc[8:].any()
    _report(name + " (tri)", stat)


def test_one_row_lists(ctx, orc, cases):
    """lists of ONE row through dsss_lc_solve and dsss_triangulate, against the oracle on the same one-row list: a row below the yaw threshold (no
    flag) and the row at the switch, flagged by itself -- on the target side (bit 1, mid-list-flip) and on the source side (bit 0, mid-list-flip-src)"""
    stat = {}
    for name, rows in (("mid-list-flip", (0, None)), ("mid-list-flip-src", (None,))):
        g = cases[name]
        _load(ctx, g["frames"])
        s, t, k = g["lists"][0]
        for i in (g["switch"] if r is None else r for r in rows):
            one = k[i:i + 1]
            got = ctx.lc_solve(s, t, one)
            assert len(got) == 1
            _check_lc((name, "one row", i), got, lc_reference(orc, g["frames"], s, t, one, key=(name, "row", i)), stat)
            _check_tri(ctx.triangulate(s, t, one), tri_reference(orc, g["frames"], s, t, one, key=(name, "row", i)), "triangulate", stat)
    _report("one-row lists", stat)


def test_triangulate_flag_crosses_into_the_second_block(ctx, orc):
    """65 rows (helpers.lc_long_flip_list): tri_kernel's second block holds row 64 alone, and its flag was switched on by row 63 of the first.
    Against orc_triangulate on the whole list; row 64 alone (no flag) gives other bits, on the device as on the oracle."""
    g = lc_long_flip_list(orc)
    _load(ctx, g["frames"])
    s, t, k = g["list"]
    assert len(k) == 65 and g["switch"] == 63
    stat = {}
    full = ctx.triangulate(s, t, k)
    ref = tri_reference(orc, g["frames"], s, t, k, key=("long-flip", 0))
    _check_tri(full, ref, "triangulate", stat)
    last = ctx.triangulate(s, t, k[64:])
    r_last = tri_reference(orc, g["frames"], s, t, k[64:], key=("long-flip", "last"))
    _check_tri(last, r_last, "triangulate last row", stat)
    assert r_last["out"].tobytes() != ref["out"][64:].tobytes() and last.tobytes() != full[64:].tobytes()
    _report("65 rows (tri)", stat)


def _tri_one_reference(orc, kp7, in27):
    """orc_triangulate_one on the row and its six one-ulp neighbours (both slant ranges, the target pose's x)"""
    n = len(kp7)
    out = np.zeros((7, n, 3)); stable = np.ones(n, bool)
    traces = []
    for i in range(n):
        base = None
        for v, (col, to) in enumerate([(None, 0)] + [(c, d) for c in (2, 5, "x") for d in (np.inf, -np.inf)]):
            k = kp7[i].copy(); q = in27[i].copy()
            if col == "x":
                q[21] = np.nextafter(q[21], to)
            elif col is not None:
                k[col] = np.nextafter(k[col], to)
            out[v, i], tr = orc.triangulate_one_trace(k, q[:12], q[12:24], q[24:])
            if base is None:
                base = tr; traces.append(tr)
            else:
                stable[i] &= all(tr[c] == base[c] for c in orc.TRACE_COUNTERS) and (_nonfinite_code(out[v, i]) == _nonfinite_code(out[0, i])).all()
    return out[0], np.array(traces), stable, _spread(out)


@pytest.mark.parametrize("name", TRI_GROUPS)
def test_triangulate_group(ctx, orc, cases, name):
    """dsss_triangulate against orc_triangulate, and dsss_triangulate_poses (explicit poses; start points 0.3 m and 5 m off) against
    orc_triangulate_one: floor 1e-9.  The device returns no iteration count here; the oracle's trace says which exits the rows took."""
    g = cases[name]
    _load(ctx, g["frames"])
    s, t, k = g["lists"][0]
    ref = tri_reference(orc, g["frames"], s, t, k, key=(name, 0))
    got = ctx.triangulate(s, t, k)
    st = ref["stable"]; stat = {}
    assert (np.isfinite(got) == np.isfinite(ref["out"])).all()
    _within(got[st], ref["out"][st], np.maximum(1e-9, 16 * ref["spread"][st]), "triangulate", stat)
    tr = ref["trace"]
    line = "exits: rejected %d lamMax %d stop %d chol %d, iters %d..%d" % ((tr["rejected"] > 0).sum(), (tr["lammax_exit"] > 0).sum(),
                                                                          (tr["stop_nosuccess"] > 0).sum(), (tr["chol_fail"] > 0).sum(), tr["iters"].min(), tr["iters"].max())
    ps, pt = g["frames"][s][0], g["frames"][t][0]
    rng = np.random.default_rng(11)
    for off in (0.3, 5.0):
        in27 = np.zeros((len(k), 27))
        for i, row in enumerate(k):
            in27[i, :12] = orc.pose12(ps[int(row[0])]); in27[i, 12:24] = orc.pose12(pt[int(row[3])])
            in27[i, 24:] = ref["out"][i, :3] + rng.normal(0, off, 3)
        exp, tr1, st1, sp1 = _tri_one_reference(orc, k, in27)
        assert (~st1).sum() <= 0.10 * len(k), (name, off, (~st1).sum())
        g2 = ctx.triangulate_poses(k, in27)
        assert (np.isfinite(g2[:, :3]) == np.isfinite(exp)).all()
        _within(g2[st1, :3], exp[st1], np.maximum(1e-9, 16 * sp1[st1]), "poses %.1f m" % off, stat)
        line += " | start %.1f m off: rejected %d lamMax %d stop %d iters %d..%d" % (off, (tr1["rejected"] > 0).sum(), (tr1["lammax_exit"] > 0).sum(),
                                                                                       (tr1["stop_nosuccess"] > 0).sum(), tr1["iters"].min(), tr1["iters"].max())
    _report(name + " (tri)", stat)
    print("%-20s %s" % ("", line))


def test_selection_and_solve_after_bad_rows(ctx, orc, cases):
    """a 3-frame set whose lists mix good rows, zero-slant rows (NaN variances) and zero-baseline rows (NaN variances, NaN scores): the
    selection gives the oracle's edges, none of them carries a NaN variance, and the pose-graph solve goes through and lands on the oracle's poses"""
    g = cases["select"]
    _load(ctx, g["frames"])
    lists = g["lists"]
    src = [l[0] for l in lists]; tgt = [l[1] for l in lists]
    ctx.lc_solve_pairs(src, tgt, [l[2] for l in lists])
    refs = [lc_reference(orc, g["frames"], s, t, k, key=("select", p)) for p, (s, t, k) in enumerate(lists)]
    lcs = np.concatenate([r["lcs"] for r in refs]); kp7 = np.concatenate([l[2] for l in lists])
    assert np.isnan(lcs["var"]).any(1).sum() >= 9 and np.isnan(lcs["score"]).sum() >= 1
    off = np.cumsum([0] + [len(l[2]) for l in lists])
    o_edges = orc.pg_select_lc([LC_N] * 3, src, tgt, off, kp7, lcs)
    g_edges = ctx.posegraph_select(3)
    assert len(g_edges) == len(o_edges) and len(o_edges) >= 20
    assert (g_edges["a"] == o_edges["a"]).all() and (g_edges["b"] == o_edges["b"]).all()
    assert np.allclose(g_edges["rel"], o_edges["rel"], rtol=0, atol=1e-9)
    assert np.isfinite(g_edges["var"]).all() and (g_edges["var"] > 0).all()
    dr = np.concatenate([f[0] for f in g["frames"]])
    o_out, o_stats = orc.pg_solve(dr, o_edges)
    g_out, _, g_stats = ctx.posegraph_solve(3, 3 * LC_N, want_rpy=False)
    assert g_stats[0] == o_stats[0]
    assert np.abs(g_out - o_out).max() < 1e-6


def test_selection_at_the_scan_seams(orc):
    """helpers.lc_seam_case (its preconditions: tests/test_lc_paths_cpu.py): 4 200 poses, edges at the first and last thread of a scan chunk,
    on both sides of a wavefront boundary, around the block seam 4096 and at the last pose.  The selection gives the oracle's edges in the
    oracle's order; a buffer of exactly that many edges takes the same list; one edge less is DSSS_E_CAPACITY, after which the context
    repeats the full call with the same bits.  Own context: the frames are longer than the module's."""
    from diasss_amd import capi
    E_CAPACITY = -5
    g = lc_seam_case(orc)
    o_edges = g["edges"]; ne = len(o_edges)
    c = capi.Context(max_frames=4)
    try:
        for f, (pose, alt, gr) in enumerate(g["frames"]):
            c.frame_set(f, None, LC_SEAM_N, LC_M, pose, alt, gr)
        c.lc_solve_pairs([l[0] for l in g["lists"]], [l[1] for l in g["lists"]], [l[2] for l in g["lists"]])
        g_edges = c.posegraph_select(3)
        assert len(g_edges) == ne
        assert (g_edges["a"] == o_edges["a"]).all() and (g_edges["b"] == o_edges["b"]).all()
        print("seam selection: %d edges, max |rel - oracle| %.2e" % (ne, np.abs(g_edges["rel"] - o_edges["rel"]).max()))
        assert np.allclose(g_edges["rel"], o_edges["rel"], rtol=0, atol=1e-9)
        assert c.posegraph_select(3, cap=ne).tobytes() == g_edges.tobytes()
        with pytest.raises(capi.DsssError) as ei:
            c.posegraph_select(3, cap=ne - 1)
        assert ei.value.code == E_CAPACITY
        assert c.posegraph_select(3).tobytes() == g_edges.tobytes()
    finally:
        c.close()


def test_range_check_on_all_entry_points(ctx, orc, cases):
    """bin 0, bin M, ping N, ping -1 and a NaN ping, on the source and on the target side, are refused with DSSS_E_ARG by dsss_lc_solve,
    dsss_lc_solve_pairs and dsss_triangulate before anything reaches the device; the next valid call gives the bytes it gave before"""
    from diasss_amd import capi
    E_ARG = -2
    g = cases["consistent-opposite"]
    _load(ctx, g["frames"])
    s, t, k = g["lists"][0]
    k = k[:7]
    lc0 = ctx.lc_solve(s, t, k); tri0 = ctx.triangulate(s, t, k)
    ctx.lc_solve_pairs([s], [t], [k]); pairs0 = ctx.lc_get(0)
    assert pairs0.tobytes() == lc0.tobytes()
    for side in (0, 3):
        for col, val in ((1, 0.0), (1, float(LC_M)), (0, float(LC_N)), (0, -1.0), (0, np.nan)):
            bad = k.copy(); bad[5, side + col] = val
            for call in (lambda: ctx.lc_solve(s, t, bad), lambda: ctx.lc_solve_pairs([s], [t], [bad]), lambda: ctx.triangulate(s, t, bad)):
                with pytest.raises(capi.DsssError) as ei:
                    call()
                assert ei.value.code == E_ARG, (side, col, val)
            assert ctx.lc_solve(s, t, k).tobytes() == lc0.tobytes()
            assert ctx.triangulate(s, t, k).tobytes() == tri0.tobytes()
            ctx.lc_solve_pairs([s], [t], [k])
            assert ctx.lc_get(0).tobytes() == pairs0.tobytes()


E_ARG, E_STATE = -2, -4


def test_refused_lc_solve_pairs_leaves_an_empty_result_set(orc, cases):
    """dsss_lc_solve_pairs refused for one bad kp7 row (as in test_range_check_on_all_entry_points) of its second pair: the context holds an
    empty result set -- not the new offsets over rows that were never uploaded -- and the next valid call gives the bytes it gave before.
    Own context: every capacity starts at 0."""
    from diasss_amd import capi
    from tests.test_gpu_matcher import _assert_empty_result_set, _refused
    g = cases["consistent-opposite"]
    s, t, k = g["lists"][0]
    k = k[:7]
    bad = k.copy(); bad[5, 1] = float(LC_M)
    c = capi.Context(max_frames=4)
    try:
        _load(c, g["frames"])
        c.lc_solve_pairs([s, s], [t, t], [k, k[:3]])
        first = [c.lc_get(0).tobytes(), c.lc_get(1).tobytes()]
        assert len(c.lc_get(0)) == 7 and len(c.lc_get(1)) == 3
        _refused(E_ARG, lambda: c.lc_solve_pairs([s, s, s], [t, t, t], [k, bad, k]))
        _assert_empty_result_set(c)
        c.lc_solve_pairs([s, s], [t, t], [k, k[:3]])
        assert [c.lc_get(0).tobytes(), c.lc_get(1).tobytes()] == first
    finally:
        c.close()


def test_pair_buffers_grow_in_both_orders(orc, cases):
    """dsss_lc_solve_pairs first on a fresh context (it allocates the pair index and the row buffers, no correspondences), then the matcher
    (which grows its own buffers beside them), then dsss_lc_solve_pairs twice more (nothing to grow) and a matcher call below the capacity:
    the same bytes every time, the matcher on the oracle, and no correspondences to read while the result set is dsss_lc_solve_pairs'."""
    from diasss_amd import capi
    from tests.test_gpu_matcher import _check_pair, _mkframes, _refused, _same_leg_pair
    g = cases["pairs"]
    lists = g["lists"]
    src = [l[0] for l in lists]; tgt = [l[1] for l in lists]; kl = [l[2] for l in lists]
    c = capi.Context(max_frames=4)
    try:
        def lc_pairs():
            c.lc_solve_pairs(src, tgt, kl)
            got = [c.lc_get(p) for p in range(len(lists))]
            assert [len(x) for x in got] == [3, 0, 5, 1, 7]
            return [x.tobytes() for x in got]
        _load(c, g["frames"])
        first = lc_pairs()
        _refused(E_STATE, lambda: c.match_dir(0, 0))
        assert len(c.match_rows(0)) == 0
        fr = dict(enumerate(_mkframes(orc, c, (64, 64, 64))))
        c.match_pairs([0, 0, 1], [1, 2, 2])
        for p, (i, j) in enumerate(((0, 1), (0, 2), (1, 2))):
            _check_pair(c, orc, p, i, j, fr)
        c.lc_solve_all()
        assert [len(c.lc_get(p)) for p in range(3)] == [len(c.match_kp7(p)) for p in range(3)]
        _load(c, g["frames"])
        assert lc_pairs() == first
        assert lc_pairs() == first
        fr = _same_leg_pair(orc, c, 64)                           # one pair, with rows: the write pass into the row buffers dsss_lc_solve_pairs allocated
        c.match_pairs([0], [2])
        assert _check_pair(c, orc, 0, 0, 2, fr) > 0
        c.lc_solve_all()
        assert len(c.lc_get(0)) == len(c.match_kp7(0)) > 0
    finally:
        c.close()

"""GPU parity of what dsss_match_pairs runs BEHIND the nearest-neighbour kernels -- scc_kernel, pair_rows_kernel<false/true>, scan2_kernel and the
kp7_flip flags dsss_lc_solve_all reads -- on the designed pairs of tests/matcher_tail_ref.py.  Which branch each pair takes is asserted on the
oracle alone by tests/test_matcher_tail_cpu.py; here every pair goes through match_pairs and the full comparison of test_gpu_matcher._check_pair:
first-stage and SCC correspondences, history, count, model, rows and kp7 bit-exact.  The sticky yaw flags have no getter: they are seen through
lc_get, against the oracle's LoopClosingTFs of the pair's kp7 list under the rule and the tolerances of test_gpu_lc_paths._check_lc, and against
dsss_lc_solve of the same list byte for byte (that entry point computes its flags in the LM kernel, not in pair_rows_kernel)."""
import numpy as np
import pytest

from tests import helpers as H
from tests import matcher_tail_ref as R
from tests.test_gpu_lc_paths import _check_lc, _report
from tests.test_gpu_matcher import _check_pair

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from diasss_amd import capi
    c = capi.Context(max_frames=4)
    yield c
    c.close()


def _load(ctx, fr):
    for fid, f in fr.items():
        ctx.frame_set(fid, None, f["N"], f["M"], f["pose"], f["alt"], f["gr"])
        ctx.features_set(fid, f["N"], f["M"], f["kps"], f["desc"], geo=f["geo"], bbox=f["bb"])


def _run_pair(ctx, orc, c, params=None, rec=None):
    i, j = c["ids"]
    ctx.match_pairs([i], [j])
    n = _check_pair(ctx, orc, 0, i, j, c["fr"], params)
    if rec is not None:
        assert n == len(rec["rows"]) and len(ctx.match_kp7(0)) == len(rec["kp7"])
        assert ctx.match_total() == (len(rec["rows"]), len(rec["kp7"]))
    return n


@pytest.mark.parametrize("name", R.NAMES)
def test_designed_pair(ctx, orc, name):
    """every pair of the case table: merged pairs with more than 256 rows a phase, direction 1 / direction 2 / the tie / an empty history on
    either side and on both, merge_thr at equality, opposite parity with different row counts (both orders) and the same parity with
    different row counts, the SCC edges (pix_err at equality, equal clusters in both orders, several strict improvements, nloc of 1, 2,
    256 and 257), the nadir rejection with truncated bins"""
    c = R.case(name)
    rec = R.branch_record(c, key=name)
    _load(ctx, c["fr"])
    _run_pair(ctx, orc, c, rec=rec)
    assert ctx.pair_is_active(0)
    ctx.lc_solve_all()
    assert len(ctx.lc_get(0)) == len(rec["kp7"])


def test_scc_iteration_budgets(orc):
    """scc_iters of 1, 2, 255, 256, 257 and the default 1000 on the pairs whose only winning hypothesis is iteration 255 or 256, and on the graded
    clusters (history empty with matches at a budget of 1).  Own context, budgets in rising order: the stream of generator words behind the
    pointer tables grows with every step."""
    from diasss_amd import capi
    c = capi.Context(max_frames=4)
    try:
        mp, op, mt, pg = c.default_params()
        assert mt.scc_iters == 1000
        for it in R.SCC_ITERS:
            mt.scc_iters = it
            c.set_params(match=mt)
            for name in ("late-255", "late-256", "graded"):
                case = R.case(name)
                _load(c, case["fr"])
                p = R.match_params(scc_iters=it)
                _run_pair(c, orc, case, p, R.branch_record(case, p, key=(name, it)))
    finally:
        c.close()


@pytest.mark.parametrize("name", R.STICKY)
def test_sticky_yaw_flags_from_the_matcher(ctx, orc, name):
    """the prefix OR of pair_rows_kernel: the first row with a large yaw mid-chunk (a), in the second 256-chunk of phase 1 with small-yaw rows
    in the third (b), in phase 1 of a merged pair whose phase 2 opens with small-yaw rows (c), for the source flag, the target flag and both;
    and a list whose only large-yaw row is nadir-rejected (no flag)"""
    c = R.sticky_case(name)
    rec = R.branch_record(c, key=("sticky", name))
    _load(ctx, c["fr"])
    _run_pair(ctx, orc, c, rec=rec)
    ctx.lc_solve_all()
    got = ctx.lc_get(0)
    kp7 = rec["kp7"]
    assert len(got) == len(kp7)
    ref = H.lc_reference(orc, dict(zip(c["ids"], c["frames"])), c["ids"][0], c["ids"][1], kp7, key=("sticky", name))
    stat = {}
    _check_lc(name, got, ref, stat)
    _report("sticky " + name, stat)
    alone = ctx.lc_solve(c["ids"][0], c["ids"][1], kp7)
    assert got.tobytes() == alone.tobytes(), "the matcher's flags are not those dsss_lc_solve derives from the same list"
    if not name.startswith("nadir-only"):
        # every row between the switch and the next large-yaw row has its flag from the prefix alone (rows in the third chunk, rows of phase 2
        # among them): in a list that starts behind the switch each of them comes out with other bits, so the equality above sees each of them
        ys, yt = R.large_yaw(c, kp7)
        sw = int(np.argmax(ys | yt))
        nfollow = R.rows_behind_switch(ys | yt, sw)
        tail = ctx.lc_solve(c["ids"][0], c["ids"][1], kp7[sw + 1:])
        same = [q for q in range(nfollow) if tail[q].tobytes() == got[sw + 1 + q].tobytes()]
        assert nfollow >= 3 and not same, "rows behind the switch whose bits do not depend on the flag: %s" % same


def test_many_active_pairs(orc):
    """325 pairs of 26 small frames in one call: more than 256 active pairs (scan2_kernel carries its totals into a second chunk), inactive
    pairs in the middle of the list, active pairs without rows; then the same list reversed"""
    from diasss_amd import capi
    m = R.many_case()
    c = capi.Context(max_frames=R.MANY_F)
    try:
        _load(c, m["fr"])
        for src, tgt in ((m["src"], m["tgt"]), (m["src"][::-1], m["tgt"][::-1])):
            c.match_pairs(src, tgt)
            tot_r = tot_k = 0
            nk = []
            nact = 0
            for p, (i, j) in enumerate(zip(src, tgt)):
                act = R.many_active(m, i, j)
                assert c.pair_is_active(p) == act, p
                nact += act
                n = _check_pair(c, orc, p, i, j, m["fr"])
                assert act or n == 0
                tot_r += n; nk.append(len(c.match_kp7(p))); tot_k += nk[-1]
            assert nact >= 257 and tot_r > 1000
            assert c.match_total() == (tot_r, tot_k)
            c.lc_solve_all()
            assert [len(c.lc_get(p)) for p in range(len(src))] == nk
    finally:
        c.close()

"""Preconditions of tests/test_gpu_matcher_tail.py, on the oracle alone (no GPU): every designed pair of tests/matcher_tail_ref.py gives
the first-stage maps it was designed for and reaches the branch of SCC_x / ConsistentCheck / GetKpsPairs / the sticky yaw flags it is
named for.  A GPU comparison on a pair that fails one of these would go green on the wrong branch."""
import numpy as np
import pytest

from tests import helpers as H
from tests import matcher_tail_ref as R


def _rec(name, **kw):
    return R.branch_record(R.case(name), key=name, **kw)


@pytest.mark.parametrize("name", R.NAMES)
def test_first_stage_is_the_designed_one(orc, name):
    c = R.case(name)
    rec = _rec(name)
    assert (rec["d01"]["nn"] == c["map_ab"]).all() and (rec["d10"]["nn"] == c["map_ba"]).all()
    assert max(len(f["kps"]) for f in c["fr"].values()) <= 2000


def test_merged_pairs(orc):
    r = _rec("merge-table")
    assert r["hist"] == (1, 1) and r["count"] == (420, 420) and r["model"] == (7.0, 7.0) and r["branch"] == "merge" and len(r["rows"]) == 460
    c = R.case("merge-long"); r = _rec("merge-long")
    na, nb = (len(c["fr"][f]["kps"]) for f in c["ids"])
    assert na != nb and na % 256 and nb % 256 and na > 1024 and nb > 1024
    assert r["branch"] == "merge" and r["n_phase1"] > 256 and r["inl"][1] > 256
    # valid rows of phase 1 in every 256-chunk of frame A, with invalid entries between them (mutual matches, outliers)
    c1, c2 = r["d01"]["corres"], r["d10"]["corres"]
    valid1 = np.array([m != -1 and c2[m] != q for q, m in enumerate(c1)])
    per_chunk = [int(valid1[q:q + 256].sum()) for q in range(0, na, 256)]
    assert all(0 < v < min(256, na - 256 * k) for k, v in enumerate(per_chunk)) and len(set(per_chunk)) > 1
    assert 0 < (c2 == -1).sum() and len(r["kp7"]) == len(r["rows"])


def test_branches_without_a_merge(orc):
    r = _rec("dir1"); assert not r["merge"] and r["model"] == (7.0, 40.0) and r["inl"] == (300, 200) and r["branch"] == 1 and len(r["rows"]) == 300
    r = _rec("dir2"); assert not r["merge"] and r["inl"] == (200, 300) and r["branch"] == 2 and len(r["rows"]) == 300
    r = _rec("tie"); assert not r["merge"] and r["inl"] == (200, 200) and r["branch"] == 2 and len(r["rows"]) == 200
    r = _rec("empty-hist-1"); assert r["hist"][0] == 0 and r["hist"][1] >= 1 and r["branch"] == 2 and len(r["rows"]) == 100
    r = _rec("empty-hist-2"); assert r["hist"][0] >= 1 and r["hist"][1] == 0 and r["branch"] == 1 and len(r["rows"]) == 100
    r = _rec("empty-hist-both"); assert r["hist"] == (0, 0) and r["count"] == (0, 0) and len(r["rows"]) == 0


def test_merge_threshold_at_equality(orc):
    r = _rec("merge-thr-eq")
    assert r["model"] == (7.0, 9.5) and np.float64(r["kp_diff"]).tobytes() == np.float64(2.5).tobytes() and r["branch"] == "merge" and len(r["rows"]) == 220
    r = _rec("merge-thr-eq-rev")
    assert r["model"] == (9.5, 7.0) and r["kp_diff"] == 2.5 and r["branch"] == "merge" and len(r["rows"]) == 220
    r = _rec("merge-thr-above")
    assert r["model"] == (7.0, 9.75) and r["kp_diff"] == 2.75 and r["branch"] == 1 and len(r["rows"]) == 120


def test_parity_and_row_counts(orc):
    for name, model in (("parity-no-merge", (7.0, 53.0)), ("parity-no-merge-swapped", (53.0, 7.0))):
        r = _rec(name)
        assert r["img_diff"] == 60 and r["model"] == model and r["kp_diff"] == 14 and not r["merge"] and r["inl"] == (420, 420), name
    for name, model in (("parity-merge", (67.0, 7.0)), ("parity-merge-swapped", (7.0, 67.0))):
        r = _rec(name)
        assert r["img_diff"] == 60 and r["model"] == model and r["kp_diff"] == 0 and r["branch"] == "merge", name
        assert r["n_phase1"] == 40 and len(r["rows"]) == 40 + r["inl"][1]
    r = _rec("same-parity-different-rows")
    assert r["img_diff"] == 0 and r["model"] == (7.0, 7.0) and r["branch"] == "merge" and r["n_phase1"] == 40


def test_scc_edges(orc):
    r = _rec("pix-err-eq")
    assert r["model"] == (7.5, 7.5) and r["count"] == (43, 43)          # 5 and 10 are inliers at exactly pix_err = 2.5
    a, b = _rec("two-equal"), _rec("two-equal-reversed")
    assert a["count"] == b["count"] == (30, 30)
    assert set(a["model"]) <= {5.0, 50.0} and set(b["model"]) <= {5.0, 50.0}
    assert a["model"][0] != b["model"][0] and a["model"][1] != b["model"][1]                  # the earlier hypothesis wins, whichever cluster it is
    r = _rec("graded")
    assert min(r["hist"]) >= 3 and r["count"] == (100, 100) and r["model"] == (85.0, 85.0)
    for n in R.NLOCS:
        r = _rec("nloc-%d" % n)
        assert r["inl"] == (n, n) and r["count"] == (n, n) and r["model"] == (7.0, 7.0) and len(r["rows"]) == n


def test_scc_iteration_counts(orc):
    """the late-winner pairs under every scc_iters of the device test: in direction 1 the only hypothesis that counts three is iteration 255
    of one pair and iteration 256 of the other, so the budgets on either side of the 256-thread stride give different results; with a
    budget of 1 or 2 a direction may end with matches and no hypothesis that counts any (history empty, nloc > 0)"""
    for name, first in (("late-255", 256), ("late-256", 257)):
        cnt = {}
        for it in R.SCC_ITERS:
            r = R.branch_record(R.case(name), R.match_params(scc_iters=it), key=(name, it))
            cnt[it] = r["count"][0]
            assert r["d01"]["ncand"].sum() == 53
        assert [cnt[it] for it in R.SCC_ITERS if it < first] == [1 if it > 2 else cnt[it] for it in R.SCC_ITERS if it < first], cnt
        assert all(cnt[it] == 3 for it in R.SCC_ITERS if it >= first) and cnt[255] == 1, cnt
    r = R.branch_record(R.case("graded"), R.match_params(scc_iters=1), key=("graded", 1))
    assert r["hist"][1] == 0 and (r["d10"]["nn"] != -1).sum() == 193 and (r["d10"]["corres"] == -1).all()


def test_nadir_rejection_and_truncation(orc):
    c = R.case("nadir"); r = _rec("nadir")
    assert r["branch"] == "merge" and r["n_phase1"] > 100
    rows, kp7 = r["rows"], r["kp7"]
    bs, bt = rows[:, 3].astype(int), rows[:, 5].astype(int)
    rej_s, rej_t = np.abs(bs - 240) < 20, np.abs(bt - 160) < 20
    assert len(kp7) == (~(rej_s | rej_t)).sum() and (rej_s & ~rej_t).sum() > 20 and (rej_t & ~rej_s).sum() > 20 and (rej_s & rej_t).sum() >= 4
    for side, col, Mh in (("s", 3, 240), ("t", 5, 160)):
        x = rows[:, col]; b = x.astype(int)
        for d in (-21, -20, -19, 19, 20, 21):
            assert ((b - Mh) == d).any(), (side, d)
        assert ((x - b) == 0.75).any() and (x == Mh + 19.75).any() and (x == Mh - 20 + 0.75).any(), "truncation: 19.75 is rejected, -19.25 is kept"
        assert (b == 1).any() and (b == 2 * Mh - 1).any() and (b >= 1).all()
        assert set(np.unique(kp7[:, 1 if side == "s" else 4] - Mh)) >= {-21.0, -20.0, 20.0, 21.0}
    assert ((rows[:, 2] - np.floor(rows[:, 2])) == 0.75).any() and ((rows[:, 4] - np.floor(rows[:, 4])) == 0.75).any()
    # the kp7 offset and the row offset part ways inside the first chunk of each phase
    na = len(c["fr"][0]["kps"])
    assert na > 512 and len(c["fr"][2]["kps"]) > 512
    keep = ~(rej_s | rej_t)
    assert 0 < keep[:100].sum() < 100 and 0 < keep[r["n_phase1"]:r["n_phase1"] + 100].sum() < 100


@pytest.mark.parametrize("name", R.STICKY)
def test_sticky_lists_switch_where_they_say(orc, name):
    c = R.sticky_case(name)
    r = R.branch_record(c, key=("sticky", name))
    assert (r["d01"]["nn"] == c["map_ab"]).all() and (r["d10"]["nn"] == c["map_ba"]).all()
    assert r["branch"] == "merge"
    kp7 = r["kp7"]
    ys, yt = R.large_yaw(c, kp7)
    n1 = r["n_phase1"]
    fs, ft = c["frames"]
    # most LMs of the list are well-posed: the oracle decides them (path-stable under helpers.lc_reference), so the device test compares them in full
    stable = H.lc_reference(orc, dict(zip(c["ids"], c["frames"])), c["ids"][0], c["ids"][1], kp7, key=("sticky", name))["stable"]
    print(name, "rows", len(kp7), "path-stable", int(stable.sum()))
    assert stable.sum() > len(kp7) / 2
    if name.startswith("nadir-only"):
        # the one row with a large yaw (source side, or target side: there the flag would move the oracle's result far beyond the tolerance)
        # is within 20 bins of nadir on that side: it is a row, not a kp7 row
        assert len(r["rows"]) == 17 and len(kp7) == 16 and not ys.any() and not yt.any()
        pose, ycol, xcol = (fs[0], 2, 3) if name == "nadir-only" else (ft[0], 4, 5)
        big = np.abs(pose[r["rows"][:, ycol].astype(int), 2]) > R.YAW_THR
        assert big.sum() == 1 and abs(int(r["rows"][big, xcol][0]) - R.STICKY_M // 2) < 20
        k = int(np.argmax(big)); assert 0 < k < 16
        if name == "nadir-only-tgt":
            full = orc.lc_solve(kp7, *fs, R.STICKY_M, *ft, R.STICKY_M)
            pf = ft[0].copy(); pf[int(kp7[0, 3]), 2] = 3.14                      # the same list with the flag on from its first row
            flagged = orc.lc_solve(kp7, *fs, R.STICKY_M, pf, ft[1], ft[2], R.STICKY_M)
            assert (np.abs(full["rel"][1:] - flagged["rel"][1:]).max(1) > 1e-6).all()
        return
    which = {"src": (ys,), "tgt": (yt,), "both": (ys, yt)}[name.split("-")[0]]
    if name.startswith("src"): assert not yt.any()
    if name.startswith("tgt"): assert not ys.any()
    na = len(c["fr"][0]["kps"])
    for flag in which:
        sw = int(np.argmax(flag))
        assert flag.any() and sw > 0 and not flag[sw + 1:sw + 4].any(), "small-yaw rows behind the switch"
        # the rows behind the switch depend on the flag: in a list that starts behind it, the rows up to its next large-yaw row come out
        # differently.  A half turn of the TARGET moves the result by far more than the tolerances of the device test (1e-9 on rel); a half
        # turn of the SOURCE leaves the problem what it was up to rounding (both sss factors see the plane across the track, which a half
        # turn maps onto itself), so those rows differ in their last bits only -- the device test therefore also holds the matcher's lists
        # to dsss_lc_solve of the same rows byte for byte.
        full = orc.lc_solve(kp7, *fs, R.STICKY_M, *ft, R.STICKY_M)
        tail = orc.lc_solve(kp7[sw + 1:], *fs, R.STICKY_M, *ft, R.STICKY_M)
        nfollow = R.rows_behind_switch(ys | yt, sw)
        assert nfollow >= 3
        d = np.abs(full["rel"][sw + 1:sw + 1 + nfollow] - tail["rel"][:nfollow]).max(1)
        if flag is yt: assert (d > 1e-6).all(), d
        else: assert (d > 0).all(), d
        if name.endswith("-a"): assert n1 == 0 and 8 <= sw < 200
        if name.endswith("-b"):
            assert sw < n1 and na > 512
            a_idx = [q for q, m in enumerate(r["d01"]["corres"]) if m != -1 and r["d10"]["corres"][m] != q]
            assert 256 <= a_idx[sw] < 512 and sum(1 for q in a_idx if q >= 512) >= 3 and len(c["fr"][2]["kps"]) > 256
            assert not (ys | yt)[sw + 1:n1].any(), "the rows of the third chunk have the flag from the carry alone"
        if name.endswith("-c"): assert sw < n1 and not (ys | yt)[n1:n1 + 3].any(), "phase 2 opens with small-yaw rows"
    if name == "both": assert int(np.argmax(ys)) != int(np.argmax(yt))


def test_many_pairs_case(orc):
    c = R.many_case()
    act = [R.many_active(c, i, j) for i, j in zip(c["src"], c["tgt"])]
    assert len(act) == 325 and sum(act) >= 257
    idle = [p for p, a in enumerate(act) if not a]
    assert len(idle) == 49 and min(idle) > 0 and max(idle) < 324 and sum(act[:max(idle)]) > 256      # inactive ones on both sides of the 256th active pair
    assert all(12 <= len(f["kps"]) <= 40 for k, f in c["fr"].items() if k != R.MANY_EMPTY) and len(c["fr"][R.MANY_EMPTY]["kps"]) == 0
    nrows = []
    for p, (i, j) in enumerate(zip(c["src"], c["tgt"])):
        a, b = c["fr"][i], c["fr"][j]
        rows = orc.robust_matching(i, j, a["N"], b["N"], a["kps"], a["desc"], a["geo"], a["bb"], b["kps"], b["desc"], b["geo"], b["bb"])
        nrows.append(len(rows))
        if not act[p]: assert len(rows) == 0
        if act[p] and (i in R.MANY_ALONE or j in R.MANY_ALONE): assert len(rows) == 0
    assert sum(1 for p, n in enumerate(nrows) if act[p] and n == 0) >= 40 and sum(1 for n in nrows if n > 3) >= 100 and sum(nrows) > 1000
    # totals cross the 256-pair chunk of the offset scan with rows on both sides of it
    live = [n for p, n in enumerate(nrows) if act[p]]
    assert sum(live[:256]) > 0 and sum(live[256:]) > 0


@pytest.mark.parametrize("kind,accepted,ties", [("lattice", (398, 407), (42, 23)), ("cluster", (46, 84), (292, 211)), ("cell_edges", (160, 208), (1430, 1283))])
def test_corner_case_geometry_under_both_descriptor_rules(orc, kind, accepted, ties):
    """the frames of test_gpu_matcher.py::test_matcher_geo_grid_corner_cases(_l2): what the oracle accepts in direction 1 under the Hamming and
    the L2-on-bytes rule, and on how many keypoints with several candidates best = second (the fold's tie rule decides): far more than the 10
    accepted matches the device tests ask for, with the palette of four descriptors as it is"""
    from tests.test_gpu_matcher import geo_grid_corner_frames
    fr = geo_grid_corner_frames(kind)
    a, b = fr[0], fr[2]
    for use_l2 in (0, 1):
        d = orc.match_dir(0, 2, b["N"], a["kps"], a["desc"], a["geo"], b["kps"], b["desc"], b["geo"], b["bb"], R.match_params(use_l2=use_l2), scc=False)
        multi = d["ncand"] > 1
        assert (d["nn"] >= 0).sum() == accepted[use_l2] > 10
        assert (d["best"][multi] == d["second"][multi]).sum() == ties[use_l2] > 10


@pytest.mark.parametrize("use_l2", [0, 1])
def test_first_stage_decision_table_is_the_oracles(orc, use_l2):
    """tests/matcher_decision_ref.py: the written table of first-stage results is what the oracle computes, so no designed query misses its
    exit; every exit occurs (accepted and refused in both directions of both pairs, and the ratio decides where the table says it does)"""
    from tests import matcher_decision_ref as D
    for ratio, by_dir in D.EXPECT[use_l2].items():
        for (other, d), want in by_dir.items():
            assert D.oracle_nn(use_l2, ratio, other, d).tolist() == want, (use_l2, ratio, other, d)
    a, b = D.EXPECT[use_l2][0.35], D.EXPECT[use_l2][1.0]
    assert [k for k in a if a[k] != b[k]] == [(1, 0), (2, 0)] and a[1, 0][6] == -1 and b[1, 0][6] == 5 and b[2, 0][4] == 2 and b[2, 0][6] == 6
    if use_l2 == 0:                                             # 85 flipped bits: refused with ids of different parity, accepted with the same
        assert a[1, 0][3] == -1 and a[2, 0][3] == 1



def _first_stage_restated(a, b, ratio, nbytes=128, strict=True, l2_bound=350.0, radius=8.0):
    """the L2 branch of orc_match_nn in numpy; nbytes = 32 reads a quarter of every row, strict = False turns `best < l2_bound` into `<=`"""
    out = []
    for i in range(len(a["kps"])):
        x, y = a["geo"][i]
        nn = -1
        if not (x < b["bb"][0] or y < b["bb"][2] or x > b["bb"][1] or y > b["bb"][3]):
            best = second = 1000.0; bid = -1; nc = 0
            for j in range(len(b["kps"])):
                if not np.sqrt((x - b["geo"][j, 0]) ** 2 + (y - b["geo"][j, 1]) ** 2) < radius: continue
                nc += 1
                d = np.sqrt(float(((a["desc"][i, :nbytes].astype(int) - b["desc"][j, :nbytes].astype(int)) ** 2).sum()))
                if d < best: second, best, bid = best, d, j
                elif d < second: second = d
            inside = (best < l2_bound) if strict else (best <= l2_bound)
            with np.errstate(invalid="ignore"):              # 0 / 0 is a NaN as in C: the ratio test fails
                r = np.float64(best) / np.float64(second)
            if nc and ((bid != -1 and inside and r <= ratio) or (nc == 1 and inside)): nn = bid
        out.append(nn)
    return out


def test_first_stage_decision_table_of_the_l2_128_design_is_the_oracles(orc):
    """the written table of use_l2 = 2 (tests/matcher_decision_ref.py) is what the oracle computes at every ratio, the rows are built as the
    module says (every difference in bytes 32 to 127 and in two 16-byte words or more, bytes of 128 and above in every base row), and the
    restated rule shows what the table is worth: read 32 bytes of a row, or accept at the bound, and it fails"""
    from tests import matcher_decision_ref as D
    fr = D.frames(2)
    assert [len(fr[f]["kps"]) for f in (0, 1, 2)] == [12, 14, 13] and all(fr[f]["desc"].shape[1] == 128 for f in fr)
    for ratio in D.RATIOS128:
        for (other, d), want in D.EXPECT[2][ratio].items():
            got = D.oracle_nn(2, ratio, other, d).tolist()
            print("use_l2 2 ratio %.2f frame %d direction %d: oracle %s" % (ratio, other, d, got))
            assert got == want, (ratio, other, d)
    # the rows
    site0 = {s: k for k, s in enumerate("ABCDEFGHIJKL")}
    sq = {"S100": 100, "S400": 400, "S900": 900, "S1600": 1600, "BELOW": 350 * 350 - 1, "AT": 350 * 350}
    for f in (1, 2):
        for k, (site, _, diffs, _) in enumerate(D.FRAME128[f]):
            delta = fr[f]["desc"][k].astype(int) - fr[0]["desc"][site0[site]].astype(int)
            if diffs == "far":
                assert (np.abs(delta) == 90).all() and (delta ** 2).sum() == 1036800 > 1000000
                continue
            assert (delta[:32] == 0).all() and len({p // 16 for p in np.nonzero(delta)[0]}) >= 2, (f, k)
            assert (delta ** 2).sum() == sum(v * v for v in diffs) and (delta ** 2).sum() in sq.values()
    assert all((fr[0]["desc"][k][:32] >= 128).any() and (fr[0]["desc"][k][32:] >= 128).sum() == 48 for k in range(12))
    assert (fr[1]["desc"][5] != fr[1]["desc"][6]).any() and (fr[2]["desc"][6] != fr[2]["desc"][7]).any(), "the tied candidates are different rows"
    # what decides where: the ratio at 0.5 exactly, the tie's lower index, the nc == 1 exit alone at 0.2
    E = D.EXPECT[2]
    assert E[0.35][1, 0][8] == -1 and E[0.5][1, 0][8] == 8 and E[0.5][2, 0][8] == 9
    assert E[0.35][1, 0][6] == -1 and E[1.0][1, 0][6] == 5 and E[1.0][2, 0][6] == 6
    assert E[0.2][1, 0][2] == 1 and E[0.2][2, 0][3] == 1 and E[0.2][1, 0][4] == -1
    pairs = [(ratio, other, d) for ratio in D.RATIOS128 for other in (1, 2) for d in (0, 1)]
    def restated(ratio, other, d, **kw):
        a, b = (fr[0], fr[other]) if d == 0 else (fr[other], fr[0])
        return _first_stage_restated(a, b, ratio, **kw)
    assert all(restated(*p) == E[p[0]][p[1], p[2]] for p in pairs)
    assert all(restated(*p, nbytes=32) != E[p[0]][p[1], p[2]] for p in pairs), "32 bytes of a row: every directed pair at every ratio fails"
    assert all(restated(*p, strict=False) != E[p[0]][p[1], p[2]] for p in pairs), "best <= l2_bound: every directed pair at every ratio fails"

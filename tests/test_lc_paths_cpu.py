"""The hard cases of tests.helpers.lc_cases on the oracle alone: before the device is compared on them (tests/test_gpu_lc_paths.py) they have to
take the exits they are built for, and the oracle has to be able to decide them.  Everything here comes from the trace of the path
(orc_lc_solve_trace / orc_triangulate_trace: the loops of orc_lc_solve / orc_triangulate_one with counters; outputs identical)."""
import numpy as np
import pytest

from tests.helpers import LC_M, LC_SEAM_N, LC_SEAM_POSES, LC_SEAM_RESIDUES, lc_cases, lc_long_flip_list, lc_reference, lc_seam_case, tri_reference

EXITS = ("rejected", "lammax_exit", "stop_nosuccess", "iter_cap", "chol_fail", "marg_fail")


@pytest.fixture(scope="module")
def refs(orc):
    G = lc_cases(orc, 0)
    return {name: [(lc_reference(orc, g["frames"], s, t, k, key=(name, li)), tri_reference(orc, g["frames"], s, t, k, key=(name, li)))
                   for li, (s, t, k) in enumerate(g["lists"]) if len(k)] for name, g in G.items()}


def _rows(refs, name, what=0):
    return np.concatenate([r[what]["trace"] for r in refs[name]])


def test_trace_entry_points_return_the_plain_results(orc):
    """the traced entry points run the loop of the plain ones: same bytes out, and the trace's iteration count is the returned one"""
    G = lc_cases(orc, 0)
    for name in ("noisy-slant", "wrong-flip", "zero-slant", "zero-baseline"):
        g = G[name]; s, t, k = g["lists"][0]
        (ps, as_, gs), (pt, at, gt) = g["frames"][s], g["frames"][t]
        plain = orc.lc_solve(k, ps, as_, gs, LC_M, pt, at, gt, LC_M)
        traced, tr = orc.lc_solve_trace(k, ps, as_, gs, LC_M, pt, at, gt, LC_M)
        assert plain.tobytes() == traced.tobytes() and (tr["iters"] == plain["iters"]).all()
        tp = orc.triangulate(k, ps, as_, gs, LC_M, pt, at, gt, LC_M)
        tt, ttr = orc.triangulate_trace(k, ps, as_, gs, LC_M, pt, at, gt, LC_M)
        assert tp.tobytes() == tt.tobytes()
        Ts, Tt = orc.pose12(ps[int(k[0, 0])]), orc.pose12(pt[int(k[0, 3])])
        a, it = orc.triangulate_one(k[0], Ts, Tt, tp[0, :3] + 0.3)
        b, tr1 = orc.triangulate_one_trace(k[0], Ts, Tt, tp[0, :3] + 0.3)
        assert a.tobytes() == b.tobytes() and it == tr1["iters"]


def test_every_exit_is_taken(refs):
    """Every exit of the mini-LM is taken by at least 3 rows of one group; linChange < 0 is reported, not required (it never fired).
    A Cholesky that fails and then succeeds inside one trial sequence (the sharpest use of the array H and its factor share) was looked for in
    the zero-baseline and tiny-slant groups of seeds 0..3 and in every other group of seed 0: no row has one.  H = J^T J + lambda I with
    lambda >= 1e-5 either factors at the first lambda or holds a non-finite entry and fails at all ten (zero-slant); the assertion below
    keeps that statement true, and a row that ever breaks it belongs into a group of its own."""
    best = {e: (0, None) for e in EXITS + ("lin_neg",)}
    for name in refs:
        tr = _rows(refs, name)
        for e in best:
            n = int((tr[e] > 0).sum())
            if n > best[e][0]:
                best[e] = (n, name)
        print("%-20s rows %3d iters %3d..%3d  " % (name, len(tr), tr["iters"].min(), tr["iters"].max())
              + "  ".join("%s %d" % (e, (tr[e] > 0).sum()) for e in best) + "  smallest margin %.1e" % tr["margin"].min())
    print("exit -> (rows, group):", best)
    for e in EXITS:
        assert best[e][0] >= 3, (e, best[e])
    assert max(_rows(refs, n)["iters"].max() for n in refs) == 100 and _rows(refs, "tiny-slant")["iters"].min() >= 9      # long dependent paths
    for name in refs:                                        # no fail-then-succeed Cholesky: failures come in tens, with no accepted step
        tr = _rows(refs, name)
        bad = tr["chol_fail"] > 0
        assert (tr["chol_fail"][bad] == 10).all() and (tr["iters"][bad] == 0).all(), name


def test_no_fail_then_succeed_cholesky_in_other_seeds(orc):
    for seed in (1, 2, 3):
        G = lc_cases(orc, seed)
        for name in ("zero-baseline", "tiny-slant"):
            g = G[name]; s, t, k = g["lists"][0]
            (ps, as_, gs), (pt, at, gt) = g["frames"][s], g["frames"][t]
            _, tr = orc.lc_solve_trace(k, ps, as_, gs, LC_M, pt, at, gt, LC_M)
            assert (tr["chol_fail"] == 0).all(), (seed, name)


def test_triangulation_exits(refs):
    """the 3-DoF LM of orc_triangulate_one on the same rows (what tri_kernel is then fed): rejected steps, the lamMax exit, stop without
    success and ten failed Choleskys (sigma 0 of the zero-slant rows) each on 3 rows or more, paths of 20 and more accepted steps.
    NOT reached from the groups' own start points: the 100-iteration cap (longest path printed below; the explicit-pose form with a start
    point 5 m off does reach it on tiny-slant rows, tests/test_gpu_lc_paths.py prints it), linChange < 0, and a Cholesky that fails and
    then succeeds; the triangulation has no marginal."""
    allr = np.concatenate([_rows(refs, n, 1) for n in refs])
    for name in refs:
        tr = _rows(refs, name, 1)
        print("%-20s tri rows %3d iters %3d..%3d  " % (name, len(tr), tr["iters"].min(), tr["iters"].max())
              + "  ".join("%s %d" % (e, (tr[e] > 0).sum()) for e in ("rejected", "lammax_exit", "stop_nosuccess", "iter_cap", "chol_fail", "lin_neg")))
    for e, name in (("rejected", "noisy-slant"), ("lammax_exit", "noisy-slant"), ("stop_nosuccess", "tiny-slant"), ("chol_fail", "zero-slant")):
        assert (_rows(refs, name, 1)[e] > 0).sum() >= 3, (e, name)
    assert _rows(refs, "tiny-slant", 1)["iters"].max() >= 20
    assert (_rows(refs, "zero-slant", 1)["iters"] == 0).all()
    assert (allr["iter_cap"] == 0).all() and (allr["lin_neg"] == 0).all()      # keeps the docstring true: a row that breaks it is a new case to compare
    bad = allr["chol_fail"] > 0
    assert (allr["chol_fail"][bad] == 10).all()


def test_degenerate_groups(orc, refs):
    r = refs["zero-slant"][0][0]
    assert (r["lcs"]["iters"] == 0).all() and np.isnan(r["lcs"]["var"]).all() and np.isfinite(r["lcs"]["rel"]).all()
    assert (r["trace"]["chol_fail"] == 10).all() and (r["trace"]["lammax_exit"] == 1).all()
    # zero-baseline: 6 rows pair a point with itself (NaN variances and NaN scores live there, and only there: see lc_cases), 58 pair it with
    # the same ping 10 bins away.  A non-finite score is NOT reached by any path-stable row of any group (moving the target's x by one ulp
    # makes ini > 0 and the score finite), so the device is held on that exit only to what holds for every row of the kind:
    # ini = 0 exactly, hence score = NaN or exactly -2 (tests/test_gpu_lc_paths.py).
    z = refs["zero-baseline"][0][0]
    same = lc_cases(orc, 0)["zero-baseline"]["same_point"]
    nanv = np.isnan(z["lcs"]["var"]).any(1)
    print("zero-baseline: NaN variances on %d rows (%d path-stable), non-finite score on %d (%d path-stable), knife-edge %d; iters %d..%d"
          % (nanv.sum(), (nanv & z["stable"]).sum(), (~np.isfinite(z["lcs"]["score"])).sum(), (~np.isfinite(z["lcs"]["score"]) & z["stable"]).sum(),
             (~z["stable"]).sum(), z["lcs"]["iters"].min(), z["lcs"]["iters"].max()))
    assert nanv.sum() >= 1 and (~nanv).sum() >= 1
    assert (np.isnan(z["lcs"]["var"]).all(1) == nanv).all()                    # all six or none
    assert not nanv[~same].any() and z["stable"][~same].all()                  # the decidable kind is decided
    sc = z["lcs"]["score"][same]
    assert (np.isnan(sc) | (sc == -2.0)).all() and np.isnan(sc).any()
    assert np.isfinite(z["lcs"]["rel"]).all()


def test_at_most_a_tenth_of_a_group_is_knife_edge(refs):
    """a row whose path changes when a slant range or the target ping's x moves by one ulp cannot be decided by the oracle, and the device is
    held to less on it: such rows stay under 10 % of every group, for the mini-LM and for the triangulation"""
    for name, lists in refs.items():
        for what in (0, 1):
            st = np.concatenate([r[what]["stable"] for r in lists])
            print("%-20s %s knife-edge %d of %d" % (name, ("lc", "tri")[what], (~st).sum(), len(st)))
            assert (~st).sum() <= 0.10 * len(st), (name, what)


@pytest.mark.parametrize("name,col", (("mid-list-flip", 3), ("mid-list-flip-src", 0)))
def test_mid_list_switch_groups(orc, refs, name, col):
    """the two sticky-flag groups are what the device tests take them for: 24 rows; the yaw of the pings in kp7 column col (3 target, 0 source)
    is small up to row 12, large at row 12, small on the next eight rows and large on the last three; and the oracle gives the eight small-yaw
    rows behind the switch other bits in the full list than in the list that starts behind the switch -- loop closure and triangulation --
    and the last three the same bits.  (Knife-edge rows of the groups: test_at_most_a_tenth_of_a_group_is_knife_edge.)"""
    g = lc_cases(orc, 0)[name]
    s, t, k = g["lists"][0]; sw = g["switch"]
    assert len(k) == 24 and sw == 12
    yaw = np.abs(g["frames"][t if col == 3 else s][0][k[:, col].astype(int), 2])
    assert (yaw[:sw] < 2).all() and yaw[sw] > 2.2 and (yaw[sw + 1:sw + 9] < 2).all() and (yaw[sw + 9:] > 2.2).all()
    lc, tri = refs[name][0]
    tail = k[sw + 1:]
    lc_t = lc_reference(orc, g["frames"], s, t, tail, key=(name, "tail")); tri_t = tri_reference(orc, g["frames"], s, t, tail, key=(name, "tail"))
    for full, part in ((lc["lcs"][sw + 1:], lc_t["lcs"]), (tri["out"][sw + 1:], tri_t["out"])):
        d = np.array([a.tobytes() != b.tobytes() for a, b in zip(full, part)])
        assert d[:8].all() and not d[8:].any(), (name, d)
    print("%-20s tail alone: knife-edge lc %d tri %d of %d" % (name, (~lc_t["stable"]).sum(), (~tri_t["stable"]).sum(), len(tail)))


def test_long_flip_list(orc):
    """helpers.lc_long_flip_list: 65 rows, the target's yaw large at row 63 only; the oracle's triangulation of row 64 in the list differs from
    that of row 64 alone (the flag is sticky), and at most a tenth of the rows is knife-edge"""
    g = lc_long_flip_list(orc)
    s, t, k = g["list"]
    assert len(k) == 65 and g["switch"] == 63
    yaw = np.abs(g["frames"][t][0][k[:, 3].astype(int), 2])
    assert (yaw[:63] < 2).all() and yaw[63] > 2.2 and yaw[64] < 2
    ref = tri_reference(orc, g["frames"], s, t, k, key=("long-flip", 0))
    last = tri_reference(orc, g["frames"], s, t, k[64:], key=("long-flip", "last"))
    assert last["out"].tobytes() != ref["out"][64:].tobytes()
    print("long-flip: knife-edge %d of 65" % (~ref["stable"]).sum())
    assert (~ref["stable"]).sum() <= 6 and ref["stable"][64] and last["stable"][0]


def test_selection_seam_case_reaches_every_seam(orc):
    """helpers.lc_seam_case on the oracle alone, before the device's ordered compaction is held to it (tests/test_gpu_lc_paths.py): the
    oracle's selection has an edge whose target pose is the first (g mod 256 = 0) and the last (255) thread of a scan chunk, the last lane
    of a wavefront and the first of the next (63, 64), and edges at the poses around the block seam 4096 and at the very last pose 4199."""
    g = lc_seam_case(orc)
    assert [len(f[0]) for f in g["frames"]] == [LC_SEAM_N] * 3 and 3 * LC_SEAM_N > 4096 and (3 * LC_SEAM_N) % 256 != 0
    assert [(s, t) for s, t, _ in g["lists"]] == [(0, 1), (0, 2), (1, 2)]
    for (s, t, k), lcs in zip(g["lists"], g["lcs"]):
        assert len(k) == len(lcs) == 2 * sum(w // LC_SEAM_N == t for w in g["wanted"])
    score = np.concatenate([l["score"] for l in g["lcs"]])
    b = g["edges"]["b"]
    print("seam case: %d rows, %d with score > 0, %d edges, per residue %s"
          % (len(score), (score > 0).sum(), len(b), {r: int((b % 256 == r).sum()) for r in LC_SEAM_RESIDUES}))
    assert (np.diff(b) > 0).all() and set(b.tolist()) <= set(g["wanted"])
    for r in LC_SEAM_RESIDUES:
        assert (b % 256 == r).any(), r
    for p in LC_SEAM_POSES:
        assert p in b, p


def _inv_longdouble(A):
    """Gauss-Jordan with partial pivoting in long double"""
    n = len(A)
    W = np.concatenate([A.astype(np.longdouble), np.eye(n, dtype=np.longdouble)], 1)
    for c in range(n):
        p = c + int(np.argmax(np.abs(W[c:, c])))
        W[[c, p]] = W[[p, c]]
        W[c] = W[c] / W[c, c]
        for r in range(n):
            if r != c:
                W[r] = W[r] - W[r, c] * W[c]
    return W[:, n:]


def test_marginal_variance_is_the_inverse_of_the_traced_information(orc):
    """a witness that is not the oracle's Cholesky: where the marginal succeeded, var = diag((J^T J)^-1) of X2's block, with J the traced
    Jacobian at the final values, product and inverse in long double; rtol 1e-6"""
    G = lc_cases(orc, 0)
    n = 0
    for name in ("consistent-opposite", "consistent-same", "noisy-slant", "wrong-flip", "tiny-slant", "long-slant", "tilted", "edges", "mid-list-flip"):
        g = G[name]; s, t, k = g["lists"][0]
        (ps, as_, gs), (pt, at, gt) = g["frames"][s], g["frames"][t]
        lcs, tr, J, r = orc.lc_solve_trace(k, ps, as_, gs, LC_M, pt, at, gt, LC_M, want_J=True)
        assert np.allclose(0.5 * (r ** 2).sum(1), lcs["err1"], rtol=1e-12)     # r is the residual at the values that were returned
        worst = 0.0
        for i in np.nonzero(tr["marg_fail"] == 0)[0]:
            Jl = J[i].astype(np.longdouble)
            want = np.diag(_inv_longdouble(Jl.T @ Jl))[9:15].astype(np.float64)
            worst = max(worst, float(np.abs(lcs["var"][i] / want - 1).max()))
            n += 1
        print("%-20s largest relative deviation of var from the long double inverse: %.2e" % (name, worst))
        assert worst < 1e-6, name
    assert n > 300

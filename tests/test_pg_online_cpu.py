"""The reference of the online pose-graph protocol (tests/pg_online_ref.py) and the oracle entry it stands on (orc_pg_solve_init),
checked on the CPU: what tests/test_gpu_pg_online.py holds dsss_posegraph_update / dsss_posegraph_update_window to has to be right
on its own.  Synthetic chains of 300 pings in three "frames" of 100 with hand-written loop closures."""
import ctypes as C
import numpy as np
import pytest

from tests import pg_online_ref as R

N_POSES, ROWS = 300, [100, 100, 100]
VAR = [1e-6, 1e-6, 1e-5, 1e-3, 0.5, 1e-2]


def _chain():
    """out 150 pings, back 150 pings 5 m to the side (the chain of test_posegraph_edges_api_small_cases)"""
    n = N_POSES
    dr = np.zeros((n, 6)); dr[:, 3] = 0.05 * np.arange(n); dr[:, 2] = 0.01 * np.sin(np.arange(n) / 30.0)
    dr[150:, 2] += 3.14159265359; dr[150:, 4] += 5.0; dr[150:, 3] = dr[149, 3] - 0.05 * np.arange(150)
    return dr


def _edge(orc, dr, a, b, dy):
    """closure a -> b measuring the dead-reckoned relative pose moved by dy metres"""
    e = np.zeros(1, orc.LCEDGE_DTYPE)
    Ta = orc.Pose(); Tb = orc.Pose(); Tr = orc.Pose()
    orc.lib().orc_pose_from_rodrigues(orc.dp(np.ascontiguousarray(dr[a])), C.byref(Ta))
    orc.lib().orc_pose_from_rodrigues(orc.dp(np.ascontiguousarray(dr[b])), C.byref(Tb))
    orc.lib().orc_pose_between(C.byref(Ta), C.byref(Tb), C.byref(Tr))
    rel = np.concatenate([np.array(Tr.R), np.array(Tr.t)]); rel[10] += dy
    e["a"] = a; e["b"] = b; e["rel"][0] = rel; e["var"][0] = VAR
    return e


def _edges(orc, dr, spec):
    return np.concatenate([_edge(orc, dr, a, b, dy) for a, b, dy in spec]) if spec else R.empty_edges(orc)


# closures ascending in b: frame 0 -> 1, 0 -> 2, 1 -> 2, inside frame 2, inside frame 0 (frozen for every window below)
SPEC = [(10, 60, 0.05), (20, 130, 0.2), (60, 160, -0.1), (40, 230, 0.3), (120, 250, 0.1), (210, 280, -0.05)]


def _params(orc, noise):
    p = orc.pg_params(); p.add_noise = noise
    return p


@pytest.mark.parametrize("noise", [0, 1])
def test_solve_init_without_start_and_prior_is_pg_solve(orc, noise):
    dr = _chain(); edges = _edges(orc, dr, SPEC)
    p = _params(orc, noise)
    out, st = orc.pg_solve(dr, edges, p)
    out2, st2, tr = orc.pg_solve_init(dr, edges, p)
    assert (out == out2).all() and (st == st2).all()
    assert int(tr[:, 4].sum()) == int(st[0]) and tr[0, 0] == st[1]           # one accepted row per LM iteration; the first trial starts at err0
    acc = tr[tr[:, 4] == 1]
    assert acc[-1, 1] == st[2] and (acc[1:, 0] == acc[:-1, 1]).all()         # ... and the accepted trials chain up to the final error
    out3, st3, _ = orc.pg_solve_init(dr, edges, p, solver="sparse")
    o_sp, s_sp = orc.pg_solve(dr, edges, p, solver="sparse")
    assert (out3 == o_sp).all() and (st3 == s_sp).all()


@pytest.mark.parametrize("noise", [0, 1])
def test_solve_init_start_and_prior_are_the_ones_given(orc, noise):
    """the start of pg_solve handed back as x0 for the first k poses, and DR[0] as the prior, change nothing: the poses behind the start keep
    THEIR draws of the one normal stream (6 i .. 6 i + 5), whatever n_init is.  A start or a prior moved by a centimetre shows in err0."""
    dr = _chain(); edges = _edges(orc, dr, SPEC)
    p = _params(orc, noise)
    p0 = _params(orc, noise); p0.max_iters = 0
    start, st0 = orc.pg_solve(dr, edges, p0)                                   # max_iters = 0: the initial estimate comes back
    out, st = orc.pg_solve(dr, edges, p)
    for k in (1, 137, N_POSES):
        o2, s2, _ = orc.pg_solve_init(dr, edges, p, x0=start[:k], prior=orc.pose12(dr[0]))
        assert (o2 == out).all() and (s2 == st).all()
    moved = start[:137].copy(); moved[50, 10] += 0.01
    _, s3, _ = orc.pg_solve_init(dr, edges, p0, x0=moved)
    assert abs(s3[1] - st0[1]) > 0.1                                           # (two chain factors see it: 0.5 (0.01 / sigma_y = 0.01)^2 each, plus their cross terms)
    prior = orc.pose12(dr[0]); prior[9] += 0.01
    _, s4, _ = orc.pg_solve_init(dr, edges, p0, x0=start, prior=prior)
    if noise == 0:                                                             # (pose 0 starts ON the prior: the moved prior adds its own term, sigma 1e-6)
        assert np.isclose(s4[1] - st0[1], 0.5 * (0.01 / 1e-6) ** 2, rtol=1e-6)
    else:
        assert abs(s4[1] - st0[1]) > 1e7


def test_fold_identity(orc):
    """E_full(frozen + Y) - E_full(frozen + Y') = E_win(Y) - E_win(Y') for window trajectories that share their first pose with
    X_prev[p0]: the folded closures keep their residuals, the dropped ones, the prior and the chain factor across the border are constant"""
    dr = _chain(); edges = _edges(orc, dr, SPEC)
    rng = np.random.default_rng(5)
    X_prev, _ = orc.pg_solve(dr, edges)                                        # some trajectory off the dead reckoning
    for p0 in (100, 200, 137):
        we, (inside, folded, dropped) = R.window_problem(orc, edges, p0, X_prev)
        assert (inside, folded, dropped) == {100: (2, 3, 1), 200: (1, 2, 3), 137: (1, 3, 2)}[p0]
        assert (we["b"] == edges["b"][dropped:] - p0).all() and (we["a"] == np.maximum(edges["a"][dropped:] - p0, 0)).all()
        Ys = []
        for _ in range(2):
            Y = X_prev[p0:].copy()
            Y[1:, 9:] += rng.normal(0, 0.05, (len(Y) - 1, 3))                # positions moved; the first pose stays X_prev[p0]
            Ys.append(Y)
        full = [orc.pg_error_at(dr, edges, np.concatenate([X_prev[:p0], Y])) for Y in Ys]
        win = [orc.pg_error_at(dr[p0:], we, Y) for Y in Ys]
        assert abs(win[0] - win[1]) > 1.0
        assert np.isclose(full[0] - full[1], win[0] - win[1], rtol=1e-9, atol=0)
    with pytest.raises(ValueError):
        R.window_problem(orc, _edges(orc, dr, [(250, 50, 0.1)]), 100, X_prev)   # from the window back into the frozen part


def test_window_that_covers_everything_is_the_global_problem(orc):
    dr = _chain(); edges = _edges(orc, dr, SPEC)
    p = orc.pg_params()
    X_prev, _ = orc.pg_solve(dr[:200], edges[edges["b"] < 200])
    g_out, g_st, _ = orc.pg_solve_init(dr, edges, p, x0=X_prev)                # the global update: warm start, prior at DR[0]
    for window, warm_n in ((3, 200), (7, 200), (0, 200)):
        assert R.window_bounds(ROWS, 3, window, warm_n) == (0, 0)
        out, st, info = R.update(orc, dr, ROWS, edges, X_prev, warm_n, window, p)
        assert (out == g_out).all() and (st == g_st).all() and (info["inside"], info["folded"], info["dropped"]) == (len(edges), 0, 0)
    c_out, c_st = orc.pg_solve(dr, edges, p)                                   # nothing warm: the cold batch solve, whatever the window
    for window in (0, 1, 2):
        assert R.window_bounds(ROWS, 3, window, 0) == (0, 0)
        out, st, _ = R.update(orc, dr, ROWS, edges, np.zeros((0, 12)), 0, window, p)
        assert (out == c_out).all() and (st == c_st).all()


def test_window_bounds_and_backward_extension():
    rows = [100, 50, 70, 30]
    assert R.window_bounds(rows, 4, 1, 250) == (3, 220)
    assert R.window_bounds(rows, 4, 2, 250) == (2, 150)
    assert R.window_bounds(rows, 4, 1, 220) == (2, 150)                        # the new frame alone: back to the last frame with an estimate
    assert R.window_bounds(rows, 4, 1, 221) == (3, 220)
    assert R.window_bounds(rows, 4, 1, 150) == (1, 100)                        # two new frames at once
    assert R.window_bounds(rows, 4, 1, 100) == (0, 0)
    assert R.window_bounds(rows, 4, 2, 120) == (1, 100)                        # an estimate that ends inside a frame anchors at that frame
    assert R.window_bounds(rows, 3, 1, 250) == (2, 150)                        # fewer frames than the estimate covers
    assert R.window_bounds(rows, 4, 0, 250) == (0, 0) and R.window_bounds(rows, 4, 9, 250) == (0, 0)


def test_accumulation_rule(orc):
    def mk(spec):                                                              # (a, b, tag): the tag travels in var[0]
        e = np.zeros(len(spec), orc.LCEDGE_DTYPE)
        for k, (a, b, tag) in enumerate(spec):
            e["a"][k] = a; e["b"][k] = b; e["var"][k, 0] = tag
        return e
    def view(e):
        return [(int(a), int(b), int(t)) for a, b, t in zip(e["a"], e["b"], e["var"][:, 0])]
    acc = R.accumulate(R.empty_edges(orc), mk([(1, 10, 1), (2, 12, 1), (3, 15, 1)]))
    assert view(acc) == [(1, 10, 1), (2, 12, 1), (3, 15, 1)]
    acc = R.accumulate(acc, mk([(4, 15, 2), (5, 20, 2)]))                      # starts AT the last target ping: replaces it, appends
    assert view(acc) == [(1, 10, 1), (2, 12, 1), (4, 15, 2), (5, 20, 2)]
    acc = R.accumulate(acc, mk([(6, 21, 3), (7, 25, 3)]))                      # starts behind everything: plain append
    assert view(acc) == [(1, 10, 1), (2, 12, 1), (4, 15, 2), (5, 20, 2), (6, 21, 3), (7, 25, 3)]
    acc = R.accumulate(acc, mk([(8, 12, 4), (9, 13, 4), (0, 25, 4)]))          # starts inside: replaces 12 and 25, 13 is sorted in
    assert view(acc) == [(1, 10, 1), (8, 12, 4), (9, 13, 4), (4, 15, 2), (5, 20, 2), (6, 21, 3), (0, 25, 4)]
    assert view(R.accumulate(acc, R.empty_edges(orc))) == view(acc)            # an empty set changes nothing
    acc = R.accumulate(acc, mk([(1, 5, 5)]))                                   # ... and one in front of everything goes to the front
    assert view(acc)[0] == (1, 5, 5) and len(acc) == 8


@pytest.mark.parametrize("window", [0, 1, 2])
def test_reference_update_never_raises_the_full_objective(orc, window):
    """frames arrive one by one with the closures that end in them; every update's result has a full-graph objective no larger than its
    start's (the previous estimate, new pings at DR o noise), and leaves the frozen part as it was"""
    dr = _chain(); edges = _edges(orc, dr, SPEC)
    p = orc.pg_params(); p0 = orc.pg_params(); p0.max_iters = 0
    X = np.zeros((0, 12)); warm_n = 0
    seen = set()
    for nf in (1, 2, 3, 3):
        rows = ROWS[:nf]; total = sum(rows)
        acc = edges[edges["b"] < total]
        start, _, _ = R.update(orc, dr, rows, acc, X, warm_n, window, p0)
        out, st, info = R.update(orc, dr, rows, acc, X, warm_n, window, p)
        e_start = orc.pg_error_at(dr[:total], acc, start); e_out = orc.pg_error_at(dr[:total], acc, out)
        assert e_out <= e_start * (1 + 1e-12)
        assert st[2] <= st[1] and (out[:info["p0"]] == X[:info["p0"]]).all()
        if info["p0"]:
            seen.add((info["inside"] > 0, info["folded"] > 0, info["dropped"] > 0))
        X, warm_n = out, total
    assert bool(seen) == (window > 0)

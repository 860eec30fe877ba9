"""Pose graphs that drive the pose-graph LM (dsss_pg.hip: lm_loop / trial) through every exit and through elimination orders the lawnmower
surveys never produce, and the oracle-only rule that says whether a case may be compared path for path (no GPU).  Shared by
tests/test_pg_paths_cpu.py (every case qualifies and takes the path it is named for) and tests/test_gpu_pg_paths.py.

A case is a builder returning (dr, edges, params).  qualify(orc, name) runs it through the oracle's three linear solvers (envelope
Cholesky, sparse LU, envelope with one step of full refinement in long double) and reads everything from orc.pg_solve_path, which records
EVERY trial: the failed factorisations and the trials with a negative linearised change as well as the decided ones.

The cases and their margins (tests/test_pg_paths_cpu.py prints them again); what does not qualify is named so that nobody tries it twice:
  LM-path cases: the lawnmower graph of 1 200 poses and 60 closures, 12 closures turned about z and given one variance on all six components.
    stop_after_reject   lambda0 = 1e8, yaw 2.0 rad, variance 1e-6, noise off: the `stop` break on a rejected trial after 17 accepted ones, default
                        rel_tol, margin 5e5.  With the default lambda0 no input takes that break without a marginal decision: yaw 1.0 / 2.5 rad x
                        variance 1e-4 / 1e-6 x two picks of the 12 closures x noise on / off x rel_tol 3e-3 .. 1e-1 gives 15 runs that reach it,
                        11 of them marginal, the other 4 with at most two iterations made and another rel_tol.
    lambda0_1e8, lambda_factor_100   yaw 0.8 rad.  On the clean graph the abs_tol exit, at yaw 1.0 a fidelity, lies within a factor 2 of its threshold.
    min_fidelity_*      yaw 2.5 rad, variance 3e-7, noise off: the plain run is RRRRRRRRRARAAARRRR, its first accepted trial has the ratio 0.174, and
                        both thresholds turn it into a rejection (ten rejections, lambda_max exit; largest ratio 0.174).  The factor-2 rule forbids
                        any trial with a ratio in [0.25, 1] (0.5) or [0.45, 1.8] (0.9), and every converging run has accepted trials with a ratio
                        near 1: no run that accepts anything qualifies.  Of yaw 2.0 / 2.5 / 3.0 x variance 1e-5 / 1e-6 / 3e-7 x four picks, four
                        runs qualify, all of this kind.
    factor_fails        variance 1e-307 on one closure: the weights are finite (3e153), their squares times the squared lever arm are not, in every
                        solver.  At 1e-300 only the envelope Cholesky fails (an overflow of ITS products; the sparse LU solves that system and
                        accepts seven trials): the solvers disagree, which rule (c) refuses.
    a factorisation that fails k times and is then rescued by lambda: none exists on the oracle.  Variances 1e-20 .. 1e-40 on one closure, with
                        the default schedule and with lambda_factor 1e4, lambda_max 1e30: the envelope Cholesky fails where rounding makes a pivot
                        negative, the sparse LU never does, and the two take different paths at every variance -- such a failure is a property of
                        the solver's rounding, not of the problem, and cannot be compared path for path.
  Topology cases: ground-truth closures, default parameters, noise on.  With the dead-reckoning drift of the lawnmower graphs the last trial of every
    run changes the objective by 1e-12 relative or less: rounding margins 0.005 .. 5 over 20 seeds each of hub, band, clique and random_pairs, i.e.
    the last accept decision rests on rounding and no seed qualifies.  The drift of hub (x 500), band, clique, clique_48 and random_pairs (x 1000) is
    therefore larger: the minimum is 1e3 .. 3e4 instead of 1e-2, and the run ends on a trial whose change is far above rounding.  hub at x 700 ..
    x 3000 is marginal, x 500 is not.  ends and wild_variances qualify with the plain drift (margins 17.7 and 55.6).
    random_pairs        ne = 0.75 n on a grid of 50 poses: the largest front has 299 block rows at n = 850, 295 at 900, 360 at 950 (358 are needed for
                        pg_front_bwd_part_kernel, 145 for more than PG_RSU32_MAX_TILES tiles on a level).  Its envelope is the whole reduced matrix
                        and costs the envelope Cholesky 14 s a run against 0.9 s of the sparse LU, so rule (c) is held here with the sparse LU and
                        the sparse LU with full_refine = 1 alone; the envelope run, made once, takes the same path AAA and differs from the sparse
                        reference by 2.9e-13 in the poses and 2.6e-15 relative in the objective.  (hub: 0.5 s, wild_variances: 0.9 s, both in.)
    clique              a clique of 40 poses does NOT give a front wider than two panels: its columns have at most 40 rows, which the
                        analysis hands to the binned subtree kernel (30 columns binned, one front of 12 block rows).  clique_48 is added for the
                        front: one front of 49 block rows in 4 panels.
    wild_variances      pairs at least 50 poses apart, drawn until 200 are distinct.
"""
import functools

import numpy as np

from tests import pg_online_ref as R

POSE_BAR, OBJ_BAR = 1e-6, 1e-6          # the device's bars; the oracle's three solvers have to agree ten times closer
BASE = (4, 300, 60, 7)                  # _lawnmower_graph(n_lines, per_line, n_lc, seed): 1 200 poses, 60 closures


def _base():
    from tests.test_gpu_configs import _lawnmower_graph
    dr, gt, e = _lawnmower_graph(*BASE)
    return dr, gt, e


def _edges(orc, a, b, gt, var=(1e-5, 1e-5, 1e-4, 1e-2, 1e-2, 1e-2)):
    """closures a -> b measured on the ground truth gt (n x 6 rotation vector, translation)"""
    from scipy.spatial.transform import Rotation as Rot
    a = np.asarray(a, np.int32); b = np.asarray(b, np.int32)
    Ra = Rot.from_rotvec(gt[a, :3]).as_matrix(); Rb = Rot.from_rotvec(gt[b, :3]).as_matrix()
    e = np.zeros(len(a), orc.LCEDGE_DTYPE)
    e["a"] = a; e["b"] = b
    e["rel"][:, :9] = np.einsum("nji,njk->nik", Ra, Rb).reshape(-1, 9)
    e["rel"][:, 9:] = np.einsum("nji,nj->ni", Ra, gt[b, 3:] - gt[a, 3:])
    e["var"] = np.broadcast_to(np.asarray(var, np.float64), (len(a), 6))
    return e


def _convert(orc, e):
    out = np.zeros(len(e), orc.LCEDGE_DTYPE)
    for k in ("a", "b", "rel", "var"):
        out[k] = e[k]
    return out


def _params(orc, **kw):
    p = orc.pg_params()
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def _yawed(orc, ang, var, nbad=12, pick_seed=1, **kw):
    """the base graph with nbad of its closures turned by `ang` rad about z and given the variance `var` on all six components"""
    from scipy.spatial.transform import Rotation as Rot
    dr, _gt, e = _base()
    e = _convert(orc, e)
    bad = np.random.default_rng(pick_seed).choice(len(e), nbad, replace=False)
    Rz = Rot.from_rotvec([0, 0, ang]).as_matrix()
    for b in bad:
        e["rel"][b, :9] = (e["rel"][b, :9].reshape(3, 3) @ Rz).reshape(9)
    e["var"][bad] = var
    return dr, e, _params(orc, **kw)


def _clean(orc, **kw):
    dr, _gt, e = _base()
    return dr, _convert(orc, e), _params(orc, **kw)


def _walk(n, seed, spacing=0.05, drift=1.0):
    """a gently curving track of n poses with its drifting dead reckoning: (dr, gt)"""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    yaw = 0.3 * np.sin(k / 211.0)
    gt = np.zeros((n, 6))
    gt[:, 2] = yaw
    gt[:, 3] = np.cumsum(np.cos(yaw)) * spacing; gt[:, 4] = np.cumsum(np.sin(yaw)) * spacing; gt[:, 5] = 0.2 * np.sin(k / 500.0)
    gt[:, 0] = 0.01 * np.sin(k / 333.0); gt[:, 1] = 0.01 * np.cos(k / 411.0)
    dr = gt.copy()
    dr[:, 3] += drift * np.cumsum(rng.normal(0, 2e-4, n)); dr[:, 4] += drift * np.cumsum(rng.normal(0, 2e-4, n)); dr[:, 2] += drift * np.cumsum(rng.normal(0, 2e-7, n))
    return dr, gt


def _pairs(a, b):
    """unique (a, b) pairs, a != b, in ascending order of (a, b)"""
    a = np.asarray(a, np.int64); b = np.asarray(b, np.int64)
    keep = a != b
    key = np.unique(a[keep] * (1 << 31) + b[keep])
    return (key >> 31).astype(np.int32), (key & ((1 << 31) - 1)).astype(np.int32)


# ---------------------------------------------------------------- topology cases
def _hub(orc, seed=11):
    n = 1200
    dr, gt = _walk(n, seed, drift=500.0)
    others = np.random.default_rng(12).choice(np.setdiff1d(np.arange(n), [600]), 300, replace=False)
    a, b = _pairs(np.full(300, 600), others)
    return dr, _edges(orc, a, b, gt), _params(orc)


def _clique(orc, k=40, seed=13):
    n = 15 * k
    dr, gt = _walk(n, seed, drift=1000.0)
    m = np.arange(k) * 15 + 7
    ia, ib = np.triu_indices(k, 1)
    return dr, _edges(orc, m[ia], m[ib], gt), _params(orc)


RANDOM_PAIRS = (950, 712)               # the smallest size at which the twin reports the fronts wanted: see the module docstring


def _random_pairs(orc, n=None, ne=None, seed=17):
    n = n or RANDOM_PAIRS[0]; ne = ne or RANDOM_PAIRS[1]
    dr, gt = _walk(n, seed, drift=1000.0)
    rng = np.random.default_rng(18)
    a, b = _pairs(rng.integers(0, n, ne), rng.integers(0, n, ne))
    return dr, _edges(orc, a, b, gt), _params(orc)


def _band(orc, seed=19):
    n = 400
    dr, gt = _walk(n, seed, drift=1000.0)
    a = np.repeat(np.arange(n), 4); b = a + np.tile(np.arange(2, 6), n)
    keep = b < n
    return dr, _edges(orc, a[keep], b[keep], gt), _params(orc)


def _ends(orc):
    n = 500
    dr, gt = _walk(n, 23)
    return dr, _edges(orc, [0, 0, n - 1, 1], [n - 1, 1, n - 2, n - 1], gt), _params(orc)


def _tiny(orc, n):
    """n poses, noise off, one closure (0, n - 1) that is 2 cm and 1 mrad wrong: the minimum is not zero.  n = 1 has no closure."""
    dr, gt = _walk(max(n, 2), 29)
    dr, gt = dr[:n], gt[:n]
    if n < 2:
        return dr, np.zeros(0, orc.LCEDGE_DTYPE), _params(orc, add_noise=0)
    g2 = gt.copy(); g2[n - 1, 3] += 0.02; g2[n - 1, 2] += 1e-3
    return dr, _edges(orc, [0], [n - 1], g2), _params(orc, add_noise=0)


def _wild_variances(orc):
    """200 closures between random poses at least 50 apart, drawn until 200 pairs are distinct; each of the six variances of each closure
    log-uniform over twelve decades"""
    n = 1200
    dr, gt = _walk(n, 31)
    rng = np.random.default_rng(32)
    seen = []
    while len(seen) < 200:
        a, b = int(rng.integers(0, n)), int(rng.integers(0, n))
        if abs(b - a) >= 50 and (min(a, b), max(a, b)) not in seen:
            seen.append((min(a, b), max(a, b)))
    a, b = _pairs(*np.array(seen).T)
    e = _edges(orc, a, b, gt)
    e["var"] = 10.0 ** rng.uniform(-10, 2, (len(e), 6))
    return dr, e, _params(orc)


# ---------------------------------------------------------------- the cases
# name -> (builder, oracle solver of the reference, what the trace must show)
LM_CASES = {
    "reject_then_accept": lambda o: _yawed(o, 1.0, 1e-6, add_noise=0),
    "accept_then_reject": lambda o: _yawed(o, 2.5, 1e-4, pick_seed=3),
    "interleaved": lambda o: _yawed(o, 2.5, 1e-4),
    "all_rejected_lammax": lambda o: _yawed(o, 2.5, 1e-7, add_noise=0),
    "stop_after_reject": lambda o: _yawed(o, 2.0, 1e-6, add_noise=0, lambda0=1e8),
    "lambda0_1e-12": lambda o: _clean(o, lambda0=1e-12),
    "lambda0_1e8": lambda o: _yawed(o, 0.8, 1e-6, add_noise=0, lambda0=1e8),
    "lambda_factor_2": lambda o: _yawed(o, 1.0, 1e-6, add_noise=0, lambda_factor=2.0),
    "lambda_factor_100": lambda o: _yawed(o, 0.8, 1e-6, add_noise=0, lambda_factor=100.0),
    "lambda_max_1e-3": lambda o: _yawed(o, 2.5, 1e-7, add_noise=0, lambda_max=1e-3),
    "min_fidelity_0.5": lambda o: _yawed(o, 2.5, 3e-7, add_noise=0, min_fidelity=0.5),
    "min_fidelity_0.9": lambda o: _yawed(o, 2.5, 3e-7, add_noise=0, min_fidelity=0.9),
    "max_iters_1": lambda o: _clean(o, max_iters=1),
    "max_iters_2": lambda o: _clean(o, max_iters=2),
    "abs_tol_early": lambda o: _clean(o, abs_tol=1.0),
    "factor_fails": lambda o: _factor_fails(o, 1e-307),
}
TOPOLOGY_CASES = {
    "hub": _hub, "clique": _clique, "clique_48": lambda o: _clique(o, 48), "random_pairs": _random_pairs, "band": _band, "ends": _ends,
    "tiny_1": lambda o: _tiny(o, 1), "tiny_2": lambda o: _tiny(o, 2), "tiny_3": lambda o: _tiny(o, 3), "tiny_7": lambda o: _tiny(o, 7),
    "wild_variances": _wild_variances,
}
SPARSE_REFERENCE = ("random_pairs", "hub", "wild_variances")      # the envelope of these is as wide as the graph: sparse LU is the reference
CASES = dict(LM_CASES, **TOPOLOGY_CASES)


def _factor_fails(orc, var, **kw):
    dr, _gt, e = _base()
    e = _convert(orc, e)
    e["var"][0] = var
    return dr, e, _params(orc, **kw)


def build(orc, name):
    return CASES[name](orc)


def path_string(path):
    """one letter per trial: A accepted, R rejected, N linearised change negative or not finite, F factorisation failed"""
    return "".join("F" if k == 2 else "N" if k == 1 else ("A" if acc else "R") for acc, k in zip(path[:, 4].astype(int), path[:, 5].astype(int)))


def exit_taken(path, stats, params):
    """which exit ended the run, from the oracle's record alone"""
    iters, _e0, err, lam = stats
    if not len(path):
        return "no_trial"
    s = path_string(path)
    if s[-1] != "A":
        return "lambda_max" if lam >= params.lambda_max else "stop_after_reject"
    if iters >= params.max_iters:
        return "max_iters"
    cur = path[-1, 0]
    if err <= 0:
        return "zero"
    if (cur - err) / cur <= params.rel_tol:
        return "rel_tol"
    if cur - err <= params.abs_tol:
        return "abs_tol"
    return "?"


@functools.lru_cache(maxsize=None)
def _reference(orc, name):
    dr, e, p = build(orc, name)
    solver = "sparse" if name in SPARSE_REFERENCE else "envelope"
    return (dr, e, p) + tuple(orc.pg_solve_path(dr, e, p, solver=solver))


def reference(orc, name):
    """(dr, edges, params, poses, stats, trace, path, ntrials) of the case on the oracle, computed once and shared: leave it unchanged"""
    return _reference(orc, name)


@functools.lru_cache(maxsize=None)
def qualify(orc, name):
    """May the device be held to this case path for path?  Decided from the oracle alone.  Returns a dict: ok, why (the rules broken),
    path (string), exit, marginal, margin (rounding margin), spread_pose, spread_obj (the three solvers), ntrials, iters, lam."""
    dr, e, p, X, st, trace, path, ntrials = reference(orc, name)
    why = []
    marginal = R.is_marginal(trace, p)
    if marginal:
        why.append("a decision within a factor 2 of its threshold")
    margin = R.rounding_margin(trace, 6 * (len(dr) + len(e)))
    if margin < 10:
        why.append("rounding margin %.2g < 10" % margin)
    others = [("sparse", 0), ("envelope", 1)] if name not in SPARSE_REFERENCE else [("sparse", 1)] + ([("envelope", 0)] if name != "random_pairs" else [])
    sp = so = 0.0
    for solver, fr in others:
        X2, st2, _t2, path2, nt2 = orc.pg_solve_path(dr, e, p, solver=solver, full_refine=fr)
        if nt2 != ntrials or path_string(path2) != path_string(path) or st2[0] != st[0] or st2[3] != st[3]:
            why.append("%s full_refine %d takes another path: %s" % (solver, fr, path_string(path2)))
            continue
        sp = max(sp, float(np.abs(X2 - X).max()))
        so = max(so, abs(st2[2] - st[2]) / st[2] if st[2] > 0 else 0.0)
    if sp > POSE_BAR / 10:
        why.append("solvers differ by %.2g in the poses" % sp)
    if so > OBJ_BAR / 10:
        why.append("solvers differ by %.2g relative in the objective" % so)
    return dict(ok=not why, why=why, path=path_string(path), exit=exit_taken(path, st, p), marginal=marginal, margin=margin, spread_pose=sp, spread_obj=so,
                ntrials=ntrials, iters=int(st[0]), lam=float(st[3]))


def reduced_graph(dr, e):
    """the reduced system's graph as the host twin takes it (dsss_host_pg_solve): separators = poses a closure touches + the two ends,
    ns - 1 chain couplings first, then one chord per closure; coordinates = the separators' dead-reckoned x, y"""
    n = len(dr)
    sep = np.unique(np.concatenate([[0, n - 1], e["a"], e["b"]])).astype(np.int64)
    idx = -np.ones(n, np.int64); idx[sep] = np.arange(len(sep))
    ns = len(sep)
    ea = np.concatenate([np.arange(ns - 1), idx[e["a"]]]).astype(np.int32)
    eb = np.concatenate([np.arange(1, ns), idx[e["b"]]]).astype(np.int32)
    return ns, ea, eb, np.ascontiguousarray(dr[sep, 3]), np.ascontiguousarray(dr[sep, 4])


def twin_stats(dr, e):
    """analysis-only run of the host twin on the case's reduced graph -> stats8 (nnzL, fronts, panels, levels, front doubles, comm doubles,
    binned columns, block rows of the largest front)"""
    import ctypes as C
    from diasss_amd import capi
    ns, ea, eb, cx, cy = reduced_graph(dr, e)
    st = np.zeros(8, np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = capi.lib().dsss_host_pg_solve(ns, p(ea), p(eb), len(ea), p(cx), p(cy), None, 1, None, None, None, p(st))
    assert rc == 0, rc
    return st


# a front of f block rows has 6 f - 96 rows below its first 96-column panel: pg_front_bwd_part_kernel runs above PG_BWD_SPLIT = 2048 rows
# (f >= 358), and the 64 x 64 tiles of that trailing block number nt (nt + 1) / 2 with nt = ceil(rows / 64): above PG_RSU32_MAX_TILES = 80
# from nt = 13 (f >= 145), above PG_RSU_MAX_TILES = 320 (row solve and update as two launches) from nt = 25.  (dsss_pg_kernels.h;
# pg_build_schedule.)
FRONT_ROWS_FOR_BWD_SPLIT = 358
FRONT_ROWS_FOR_RSU32 = 145
PG_BWD_SPLIT, PG_RSU32_MAX_TILES, PG_RSU_MAX_TILES = 2048, 80, 320


def level_tiles_at_least(rows):
    """64 x 64 tiles of a level of the schedule whose tallest panel has `rows` scalar rows below it: that panel's own lower triangle of
    tiles, whatever else is on the level (pg_build_schedule)"""
    nt = (int(rows) + 63) // 64
    return nt * (nt + 1) // 2

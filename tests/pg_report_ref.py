"""Witnesses for the loop-closure residual report and the chi-square gated solve, computed with the oracle alone (no GPU):
whitened residuals through orc_pose_between / orc_pose_log, the gate rule around orc.pg_solve, the corrupted lawnmower graphs
both test files use.  Shared by tests/test_gpu_pg_report.py and tests/test_pg_report_cpu.py."""
import ctypes as C
import numpy as np

GATE, DECADE, MAX_SOLVES = 22.458, 10.0, 8          # dsss_pg_gate_params_default

# (_lawnmower_graph arguments, corrupted fraction, solves, corrupted edges, clean edges dropped, clean edges): the rule on the oracle
GATE_GRAPHS = [((6, 400, 150, 5), 0.10, 2, 14, 1, 135),
               ((4, 300, 60, 7), 0.20, 2, 12, 0, 48),
               ((6, 400, 150, 9), 0.30, 3, 45, 1, 105),
               ((3, 200, 40, 11), 0.25, 2, 10, 0, 30)]


def _pose(row12):
    from oracle import binding as O
    T = O.Pose()
    for k in range(9): T.R[k] = row12[k]
    for k in range(3): T.t[k] = row12[9 + k]
    return T


def edge_residuals(orc, edges, poses12):
    """xi[e] = Log(rel_e^-1 X_a^-1 X_b) and sigma[e] = sqrt(var_e), from the oracle's pose algebra"""
    L = orc.lib()
    poses12 = np.ascontiguousarray(poses12, np.float64).reshape(-1, 12)
    xi = np.zeros((len(edges), 6)); out = np.zeros(6)
    h = orc.Pose(); er = orc.Pose()
    for e in range(len(edges)):
        Ta = _pose(poses12[edges["a"][e]]); Tb = _pose(poses12[edges["b"][e]]); M = _pose(edges["rel"][e])
        L.orc_pose_between(C.byref(Ta), C.byref(Tb), C.byref(h))
        L.orc_pose_between(C.byref(M), C.byref(h), C.byref(er))
        L.orc_pose_log(C.byref(er), orc.dp(out))
        xi[e] = out
    return xi, np.sqrt(np.asarray(edges["var"], np.float64).reshape(-1, 6))


def residual_bound(xi, sigma):
    """the project's 1e-9 bar for loop-closure quantities with a floor for the rounding of 100 m coordinates, whitened"""
    return (1e-12 + 1e-9 * np.abs(xi)) / sigma


def chi2_bound(xi, sigma):
    """what residual_bound implies for chi2 = sum r^2: |(r + d)^2 - r^2| <= 2 |r| b + b^2 per component"""
    b = residual_bound(xi, sigma); r = np.abs(xi) / sigma
    return (2 * r * b + b * b).sum(axis=1)


def dr_poses(orc, dr):
    return np.stack([orc.pose12(p) for p in np.ascontiguousarray(dr, np.float64).reshape(-1, 6)])


def corrupted_graph(args, frac):
    """the lawnmower graph with int(frac ne) closures moved: rel[9] and rel[10] each by +-U(2, 8) m -> (dr, edges, corrupted mask)"""
    from tests.test_gpu_configs import _lawnmower_graph
    n_lines, per_line, n_lc, seed = args
    dr, _, edges = _lawnmower_graph(n_lines, per_line, n_lc, seed=seed)
    ne = len(edges)
    rng = np.random.default_rng(seed + 100)
    bad = rng.choice(ne, int(frac * ne), replace=False)
    edges = edges.copy()
    for k in (9, 10):
        edges["rel"][bad, k] += rng.choice([-1.0, 1.0], len(bad)) * rng.uniform(2.0, 8.0, len(bad))
    mask = np.zeros(ne, bool); mask[bad] = True
    return dr, edges, mask


def oracle_gate(orc, dr, edges, gate=GATE, decade=DECADE, max_solves=MAX_SOLVES):
    """the gate rule with orc.pg_solve as the solver and edge_residuals as the report -> (poses, keep, solves, closest relative
    distance of a kept edge's chi2 to a round's threshold)"""
    keep = np.ones(len(edges), bool)
    solves, margin = 0, np.inf
    while True:
        kept = np.ascontiguousarray(edges[keep])
        poses, _ = orc.pg_solve(dr, kept)
        solves += 1
        if len(kept) == 0:
            break
        xi, sg = edge_residuals(orc, kept, poses)
        chi2 = ((xi / sg) ** 2).sum(axis=1)
        chi2[~np.isfinite(chi2)] = np.inf
        m = chi2.max()
        thr = gate if m <= gate else max(gate, m / decade)
        margin = min(margin, float(np.abs(chi2 / thr - 1.0).min()))
        if m <= gate or solves == max_solves:
            break
        idx = np.flatnonzero(keep)
        keep[idx[chi2 > thr]] = False
    return poses, keep, solves, margin

"""GPU: the loop-closure residual report (dsss_posegraph_edge_report) against the oracle's own pose algebra, and the chi-square
gated solve (dsss_posegraph_solve_gated) against the same rule run around orc.pg_solve.  Witnesses in tests/pg_report_ref.py.
Tolerances: per residual component (1e-12 + 1e-9 |xi_ref|) / sigma -- the project's 1e-9 bar for loop-closure quantities with a
floor for the rounding of 100 m coordinates --, chi2 to what that implies, sums to 1e-9 relative, poses to 1e-6."""
import ctypes as C
import numpy as np
import pytest

from tests import pg_report_ref as R
from tests.helpers import pg_edge as _edge, pg_small_graph as _small_graph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from diasss_amd import capi
    c = capi.Context(max_frames=2)
    yield c
    c.close()


def _check_report(orc, dr, edges, poses12, got, what):
    """one report against the witnesses; returns the largest deviations in units of their bounds"""
    chi2, r6, sums = got
    xi, sg = R.edge_residuals(orc, edges, poses12)
    r_ref = xi / sg
    dev = [0.0, 0.0]
    if len(edges):
        d = np.abs(r6 - r_ref) / R.residual_bound(xi, sg)
        dc = np.abs(chi2 - (r_ref ** 2).sum(axis=1)) / R.chi2_bound(xi, sg)
        dev = [float(d.max()), float(dc.max())]
        print("%s: max |r - r_ref| = %.3g of its bound, max |chi2 - ref| = %.3g of its bound (largest chi2 %.4g)" % (what, dev[0], dev[1], chi2.max()))
        assert d.max() <= 1.0, what
        assert dc.max() <= 1.0, what
        assert (chi2 == (((((r6[:, 0] ** 2 + r6[:, 1] ** 2) + r6[:, 2] ** 2) + r6[:, 3] ** 2) + r6[:, 4] ** 2) + r6[:, 5] ** 2)).all(), what      # index order 0..5
    e_all = orc.pg_error_at(dr, edges, poses12)
    e_chain = orc.pg_error_at(dr, edges[:0], poses12)
    e_lc = 0.5 * (r_ref ** 2).sum()
    rel = lambda a, b: abs(a - b) / max(abs(b), 1e-300) if b != 0 else abs(a)
    print("%s: sums3 = %r, oracle %.17g (chain %.17g, closures %.17g): relative %.3g / %.3g / %.3g"
          % (what, sums.tolist(), e_all, e_chain, e_lc, rel(sums[2], e_all), rel(sums[0], e_chain), rel(sums[1], e_lc)))
    assert sums[0] + sums[1] == sums[2], what
    assert abs(sums[2] - e_all) <= 1e-9 * abs(e_all), what
    assert abs(sums[0] - e_chain) <= 1e-9 * abs(e_chain) + 1e-9 * abs(e_all), what
    assert abs(sums[1] - e_lc) <= 1e-9 * abs(e_lc) + 1e-9 * abs(e_all), what
    return dev


def _same(a, b):
    return all((np.asarray(x) == np.asarray(y)).all() for x, y in zip(a, b))


@pytest.mark.parametrize("graph", ["small9", "lawnmower"])
def test_report_parity(ctx, orc, graph):
    import torch
    from tests.test_gpu_configs import _lawnmower_graph
    if graph == "small9":
        dr, edges = _small_graph(orc)
    else:
        dr, _, edges = _lawnmower_graph(6, 400, 150, seed=5)
    solved, stats = ctx.posegraph_solve_edges(dr, edges)
    for what, poses in (("dead reckoning", R.dr_poses(orc, dr)), ("solved", solved)):
        got = ctx.posegraph_edge_report(dr, edges, poses)
        _check_report(orc, dr, edges, poses, got, "%s / %s" % (graph, what))
        for _ in range(3):                                                  # fixed-order sums, no atomics: the same bits every call
            assert _same(ctx.posegraph_edge_report(dr, edges, poses), got)
    # the solved poses as a device pointer: the same numbers
    dev = torch.from_numpy(solved).to("cuda:0")
    got_d = ctx.posegraph_edge_report(dr, edges, dev)
    _check_report(orc, dr, edges, solved, got_d, "%s / solved, device pointer" % graph)
    assert _same(got_d, got)
    # the objective at the solve's own result is the solve's final error
    print("%s: sums3[2] %.17g, stats4 final error %.17g" % (graph, got[2][2], stats[2]))
    assert abs(got[2][2] - stats[2]) <= 1e-9 * abs(stats[2])


@pytest.mark.parametrize("n,ne", [(1, 0), (2, 0), (250, 5), (256, 0), (250, 7), (300, 213)])
def test_report_workgroup_and_wavefront_boundaries(ctx, orc, n, ne):
    """total + ne = 1, 2, 255, 256, 257, 513 factors: one thread, part of a wavefront, one short of a workgroup, exactly one, one
    more (the closures straddle the workgroups), two and a thread; with and without closures; a chain of ONE pose (the prior alone)"""
    assert n + ne in (1, 2, 255, 256, 257, 513)
    rng = np.random.default_rng(100 + n + ne)
    dr = np.zeros((n, 6)); dr[:, 3] = 0.05 * np.arange(n); dr[:, 2] = 0.01 * np.sin(np.arange(n) / 30.0); dr[:, 5] = rng.uniform(-0.2, 0.2, n)
    ends = [tuple(rng.choice(n, 2, replace=False)) for _ in range(ne)] if ne else []
    edges = np.concatenate([_edge(orc, dr, int(a), int(b), rng.uniform(-0.3, 0.3)) for a, b in ends]) if ne else np.zeros(0, orc.LCEDGE_DTYPE)
    at = dr.copy(); at[:, 3:] += rng.normal(0, 1e-3, (n, 3)); at[:, :3] += rng.normal(0, 1e-5, (n, 3))      # off the measurements: no residual is zero
    poses = R.dr_poses(orc, at)
    got = ctx.posegraph_edge_report(dr, edges, poses)
    assert got[0].shape == (ne,) and got[1].shape == (ne, 6)
    _check_report(orc, dr, edges, poses, got, "%d poses + %d closures" % (n, ne))
    assert got[2][0] > 0 and (ne == 0) == (got[2][1] == 0)
    assert _same(ctx.posegraph_edge_report(dr, edges, poses), got)


def test_report_error_exits_leave_the_context_usable(orc):
    from diasss_amd import capi
    from tests.test_gpu_configs import _lawnmower_graph
    dr, _, edges = _lawnmower_graph(6, 400, 150, seed=5)
    poses = R.dr_poses(orc, dr)
    c = capi.Context(max_frames=2)
    first = c.posegraph_edge_report(dr, edges, poses)
    for kind in ("range", "var0", "varnan", "relnan"):
        bad = edges.copy()
        k = len(bad) // 2
        if kind == "range": bad["b"][k] = len(dr) + 5
        elif kind == "var0": bad["var"][k, 3] = 0.0
        elif kind == "varnan": bad["var"][k, 1] = np.nan
        else: bad["rel"][k, 4] = np.inf
        with pytest.raises(capi.DsssError) as ei:
            c.posegraph_edge_report(dr, bad, poses)
        assert ei.value.code == -2, kind                                    # DSSS_E_ARG
        with pytest.raises(capi.DsssError) as ei:
            c.posegraph_solve_gated(dr, bad)
        assert ei.value.code == -2, kind
        assert _same(c.posegraph_edge_report(dr, edges, poses), first), kind
    for g in ((0.0, 10.0, 8), (float("nan"), 10.0, 8), (22.458, 1.0, 8), (22.458, 10.0, 0)):      # gate not above 0, decade not above 1, no solve
        with pytest.raises(capi.DsssError) as ei:
            c.posegraph_solve_gated(dr, edges, capi.PGGateParams(g[0], g[1], g[2], 0))
        assert ei.value.code == -2, g
    assert _same(c.posegraph_edge_report(dr, edges, poses), first)
    c.close()


def test_gated_solve_trivial_forms(ctx, orc):
    """one solve allowed, or a gate nothing exceeds: the plain solve's bits, every edge kept, one solve"""
    from diasss_amd import capi
    dr, edges, _ = R.corrupted_graph((4, 300, 60, 7), 0.20)
    ref, sref = ctx.posegraph_solve_edges(dr, edges)
    for g in (capi.PGGateParams(R.GATE, R.DECADE, 1, 0), capi.PGGateParams(1e300, R.DECADE, R.MAX_SOLVES, 0)):
        poses, stats, keep, chi2, ns = ctx.posegraph_solve_gated(dr, edges, g)
        assert (poses == ref).all() and (np.asarray(stats) == np.asarray(sref)).all()
        assert keep.all() and ns == 1
        assert _same([chi2], [ctx.posegraph_edge_report(dr, edges, ref)[0]])
    # no closures at all: the chain alone, one solve
    poses, stats, keep, chi2, ns = ctx.posegraph_solve_gated(dr, edges[:0])
    ref0, _ = ctx.posegraph_solve_edges(dr, edges[:0])
    assert (poses == ref0).all() and ns == 1 and len(keep) == 0 and len(chi2) == 0


@pytest.mark.parametrize("case", range(4))
def test_gated_solve_against_the_rule_on_the_oracle(ctx, orc, case):
    args, frac, solves, nbad, ndrop, nclean = R.GATE_GRAPHS[case]
    dr, edges, bad = R.corrupted_graph(args, frac)
    o_poses, o_keep, o_solves, margin = R.oracle_gate(orc, dr, edges)
    assert margin > 0.01                                                    # ON THE ORACLE: no kept edge within 1 % of a threshold, so 1e-6 in the poses flips nothing
    poses, stats, keep, chi2, ns = ctx.posegraph_solve_gated(dr, edges)
    print("graph %s frac %.2f: device %d solves, kept %d of %d; oracle %d solves, kept %d, margin %.1f %%; max |pose - oracle| %.3g"
          % (args, frac, ns, keep.sum(), len(edges), o_solves, o_keep.sum(), 100 * margin, np.abs(poses - o_poses).max()))
    assert ns == o_solves == solves
    assert (keep == o_keep).all()
    assert np.abs(poses - o_poses).max() < 1e-6                             # orc.pg_solve on the kept edges
    xi, sg = R.edge_residuals(orc, edges, poses)                            # ALL edges, dropped ones included, at the returned trajectory
    dc = np.abs(chi2 - ((xi / sg) ** 2).sum(axis=1)) / R.chi2_bound(xi, sg)
    print("   max |chi2 - witness| = %.3g of its bound; chi2 kept max %.4g, dropped min %.4g" % (dc.max(), chi2[keep].max(), chi2[~keep].min()))
    assert dc.max() <= 1.0
    assert not (keep & bad).any()                                           # no corrupted edge kept
    assert (~keep & ~bad).sum() <= 0.05 * nclean                            # at most 5 % of the clean edges dropped
    # the last solve is the plain solve of the kept edges, bit for bit
    p2, s2 = ctx.posegraph_solve_edges(dr, np.ascontiguousarray(edges[keep]))
    assert (p2 == poses).all() and (np.asarray(s2) == np.asarray(stats)).all()

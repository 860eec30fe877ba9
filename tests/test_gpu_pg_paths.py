"""The pose-graph LM on the device (dsss_pg.hip: lm_loop / trial) against the oracle's own LM, PATH FOR PATH, on the cases of
tests/pg_paths_ref.py: rejected trials followed by another factorisation at a larger lambda, every exit of the loop taken in the middle of a
run, every field of dsss_pg_params moved, and graphs whose elimination is nothing like a lawnmower survey's.  Every case qualifies on the oracle
alone (tests/test_pg_paths_cpu.py: no decision near its threshold or on rounding, three linear solvers on one path within a tenth of the bars
here), so nothing is allowed to differ: iterations, trials, final lambda, err0, err, poses; and every solve is run twice for its bits."""
import numpy as np
import pytest

from tests import pg_paths_ref as P
from tests.test_gpu_pg_online import _objective_floor

pytestmark = pytest.mark.gpu

WORST = {"dpose": 0.0}


@pytest.fixture(scope="module")
def ctx():
    from diasss_amd import capi
    c = capi.Context(max_frames=2)
    yield c
    c.close()


def _device(ctx, dr, e, p, **override):
    """one dsss_posegraph_solve_edges with the oracle's parameters p on the context -> (poses, stats4, trials); the defaults are put back"""
    _, _, _, pg = ctx.default_params()
    for k, _t in pg._fields_:
        setattr(pg, k, override.get(k, getattr(p, k)))
    ctx.set_params(pg=pg)
    try:
        X, st = ctx.posegraph_solve_edges(dr, e)
        return X, np.asarray(st).copy(), ctx.posegraph_schedule()[1]
    finally:
        ctx.set_params(pg=ctx.default_params()[3])


def _compare(orc, ctx, name, label=None, twice=True):
    dr, e, p, Xr, sr, _trace, path, ntrials = P.reference(orc, name)
    X, st, trials = _device(ctx, dr, e, p)
    dpose = float(np.abs(X - Xr).max())
    WORST["dpose"] = max(WORST["dpose"], dpose)
    print("%-22s %s iterations %d | %d, trials %d | %d, lambda %.6g | %.6g, err0 %.12e | %.12e, err %.9e | %.9e, max |dpose| %.3e (largest so far %.3e)"
          % (label or name, P.path_string(path), st[0], sr[0], trials, ntrials, st[3], sr[3], st[1], sr[1], st[2], sr[2], dpose, WORST["dpose"]))
    assert st[0] == sr[0]
    assert trials == ntrials
    assert np.isclose(st[3], sr[3], rtol=1e-12, atol=0)
    assert np.isclose(st[1], sr[1], rtol=1e-12, atol=0)
    assert np.isclose(st[2], sr[2], rtol=P.OBJ_BAR, atol=_objective_floor(len(dr)))
    assert dpose < P.POSE_BAR
    if twice:
        X2, st2, trials2 = _device(ctx, dr, e, p)
        assert X2.tobytes() == X.tobytes() and st2.tobytes() == st.tobytes() and trials2 == trials
    return X, st, trials


@pytest.mark.parametrize("name", list(P.LM_CASES))
def test_lm_path(orc, ctx, name):
    X, st, trials = _compare(orc, ctx, name)
    if name in ("all_rejected_lammax", "factor_fails"):
        dr, e, p = P.build(orc, name)
        X0, st0, trials0 = _device(ctx, dr, e, p, max_iters=0)                   # nothing accepted: the start values, bit for bit
        assert trials0 == 0 and st0[0] == 0 and X0.tobytes() == X.tobytes() and st0[1] == st[1] == st[2]


def test_clean_solve_after_the_rejected_runs_has_the_bits_of_a_fresh_context(orc, ctx):
    """no flag, lambda or fail word survives a rejected run: the plain lawnmower solve on the context that ran every LM-path case (the two that
    end on failed factorisations and on lambda_max once more right before it) equals the one of a context that ran nothing else"""
    from diasss_amd import capi
    for name in ("factor_fails", "interleaved"):
        _device(ctx, *P.build(orc, name))
    dr, e, p = P._clean(orc)
    X, st, trials = _device(ctx, dr, e, p)
    fresh = capi.Context(max_frames=2)
    try:
        Xf, stf, trialsf = _device(fresh, dr, e, p)
    finally:
        fresh.close()
    assert X.tobytes() == Xf.tobytes() and st.tobytes() == stf.tobytes() and trials == trialsf
    Xr, sr = orc.pg_solve(dr, e, p)
    assert st[0] == sr[0] and np.abs(X - Xr).max() < P.POSE_BAR


@pytest.mark.parametrize("name", ["reject_then_accept", "interleaved", "factor_fails"])
def test_rejected_branch_with_three_partitions(orc, ctx, name):
    """the interface fronts and the reduced scalars through the rejected branch: three partitions on the one rank"""
    dr, e, p, Xr, sr, _trace, path, ntrials = P.reference(orc, name)
    ctx.set_pg_partitions(3)
    try:
        X, st, trials = _device(ctx, dr, e, p)
    finally:
        ctx.set_pg_partitions(0)
    dpose = float(np.abs(X - Xr).max())
    print("%-22s 3 partitions: iterations %d | %d, trials %d | %d, lambda %.6g | %.6g, max |dpose| %.3e" % (name, st[0], sr[0], trials, ntrials, st[3], sr[3], dpose))
    assert st[0] == sr[0] and trials == ntrials and dpose < P.POSE_BAR


@pytest.mark.parametrize("name", [n for n in P.TOPOLOGY_CASES if n != "tiny_1"])
def test_topology(orc, ctx, name):
    _compare(orc, ctx, name)
    if name in ("random_pairs", "clique_48"):
        # the schedule the device ran, not the host twin's forecast: per level, panel steps and the scalar rows below its tallest panel
        lv = ctx.posegraph_schedule()[0]
        print("%-22s levels (panel steps, widest panel, rows below the tallest, interface): %s" % (name, lv.tolist()))
        if name == "random_pairs":
            assert lv[:, 2].max() > P.PG_BWD_SPLIT                              # pg_front_bwd_part_kernel ran
            assert P.level_tiles_at_least(lv[:, 2].max()) > P.PG_RSU32_MAX_TILES    # a level left the 32 x 32 quarters
            # ... and the fused kernel altogether: the front runs trsm2 + syrk, then rsu<64>, then rsu<32> as it shrinks
            assert P.level_tiles_at_least(lv[:, 2].max()) > P.PG_RSU_MAX_TILES
        else:
            assert lv[:, 0].sum() > 2 and lv[:, 1].max() == 96                  # more than two 96-column panel steps


def test_one_pose_is_refused_before_anything_runs(orc, ctx):
    """include/dsss.h: total < 2 is DSSS_E_ARG; the context goes on working"""
    from diasss_amd import capi
    dr, e, p = P.build(orc, "tiny_1")
    with pytest.raises(capi.DsssError) as ei:
        ctx.posegraph_solve_edges(dr, e)
    assert ei.value.code == -2                                                   # DSSS_E_ARG
    _compare(orc, ctx, "tiny_2", twice=False)

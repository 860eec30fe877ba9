"""SINGLE steps of the pose-graph LM on the device against the refined oracle of tests/pg_step_ref.py: the LM is stopped after one and after two
accepted steps (max_iters on both sides) and the poses are compared there, at a bar that follows from the spread of the oracle's own f64
solvers (1e-14 .. 1e-7, most cases 1e-11) instead of the 1e-6 a converged run is held to.  A converged run repairs a slightly wrong linear solve
in its next step and hides it (tests/test_pg_step_cpu.py shows a solve wrong by 1e-4 passing every converged comparison); a single step cannot.

Step 1 is the EARLY trial: the chain part and the bins are launched under the analysis (early_trial, pre_chain, pre_bins).  Step 2 is the first
ordinary trial().  Partitions switch the early bins off and run the interface fronts; a trial after refused trials re-uploads lambda, recomputes the
chain part and does not pre-run the bins; DSSS_PG_BINS=serial and DSSS_PG_BIN_COST=1e12 run the other form of the bins and one bin for the graph.

Every combination qualifies on the oracle alone (tests/test_pg_step_cpu.py); the bar is 32 max(s, floor) but for the one case that
pg_step_ref.MARGIN_OF names with its evidence.  Asserted for each: iterations, trials, lambda, err0; the reported
err is the objective AT the returned poses; max |X - X_ref| <= bar; a second solve returns the same bytes."""
import numpy as np
import pytest

from tests import pg_step_ref as S
from tests import pg_paths_ref as P
from tests.test_gpu_pg_paths import _device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from diasss_amd import capi
    c = capi.Context(max_frames=2)
    yield c
    c.close()


def _step(orc, ctx, combo, label=""):
    name, steps, params = combo
    kw = dict(params)
    ref = S.reference(orc, name, steps, **kw)
    s = S.spread(orc, name, steps, **kw)
    bar = S.bar(orc, name, steps, **kw)
    X, st, trials = _device(ctx, ref.dr, ref.e, ref.p)
    dist = float(np.abs(X - ref.X).max())
    err_at = orc.pg_error_at(ref.dr, ref.e, X)
    print("%-32s %-22s %-13s step %-9.3g s %-9.3g bar %-9.3g device %-9.3g = %.3g s = %.3g bar; iterations %d | %d, trials %d | %d, lambda %g | %g, err %.15e at its poses %.15e"
          % (S.combo_id(combo), label, ref.path, ref.step, s, bar, dist, dist / s if s else np.inf, dist / bar, st[0], ref.stats[0], trials, ref.ntrials, st[3], ref.stats[3], st[2], err_at))
    assert st[0] == ref.stats[0] == steps
    assert trials == ref.ntrials
    assert np.isclose(st[3], ref.stats[3], rtol=1e-12, atol=0)
    assert np.isclose(st[1], ref.stats[1], rtol=1e-12, atol=0)
    assert np.isclose(st[2], err_at, rtol=1e-11, atol=0)
    assert dist <= bar
    X2, st2, trials2 = _device(ctx, ref.dr, ref.e, ref.p)
    assert X2.tobytes() == X.tobytes() and st2.tobytes() == st.tobytes() and trials2 == trials
    return X, st


@pytest.mark.parametrize("parts", [0, 3])
@pytest.mark.parametrize("combo", S.TOPOLOGY_COMBOS, ids=S.combo_id)
def test_topology_step(orc, ctx, combo, parts):
    name = combo[0]
    n = len(S.reference(orc, *combo[:2]).dr)
    label = "%d partitions" % parts
    if parts > max(1, n // 4):
        label += " (clamped to %d: n / 4)" % max(1, n // 4)
    ctx.set_pg_partitions(parts)
    try:
        _step(orc, ctx, combo, label)
        lv = ctx.posegraph_schedule()[0]
    finally:
        ctx.set_pg_partitions(0)
    if parts == 0 and name in ("random_pairs", "clique_48"):
        # the schedule the device ran (tests/test_gpu_pg_paths.py, test_topology): the step went through the kernels the case is there for
        if name == "random_pairs":
            assert lv[:, 2].max() > P.PG_BWD_SPLIT                              # pg_front_bwd_part_kernel ran
            assert P.level_tiles_at_least(lv[:, 2].max()) > P.PG_RSU32_MAX_TILES    # a level left the 32 x 32 quarters
            assert P.level_tiles_at_least(lv[:, 2].max()) > P.PG_RSU_MAX_TILES      # trsm2 + syrk, then rsu<64>, then rsu<32> as the front shrinks
        else:
            assert lv[:, 0].sum() > 2 and lv[:, 1].max() == 96                  # more than two 96-column panel steps


@pytest.mark.parametrize("combo", S.DAMPING_COMBOS, ids=S.combo_id)
def test_damping_step(orc, ctx, combo):
    """lambda0 = 1e-12 is the undamped Gauss-Newton system, where a wrong off-diagonal term shows most; 1e3 lets the diagonal dominate"""
    _step(orc, ctx, combo)


@pytest.mark.parametrize("combo", S.REFUSED_COMBOS, ids=S.combo_id)
def test_step_after_refused_trials(orc, ctx, combo):
    _step(orc, ctx, combo)


@pytest.mark.parametrize("combo", S.SERIAL_COMBOS, ids=S.combo_id)
def test_serial_bins_step(orc, ctx, monkeypatch, combo):
    """the serial kernel, which the pipelined one is held to bit for bit (tests/test_gpu_pg_bins.py), is itself held to the oracle"""
    monkeypatch.setenv("DSSS_PG_BINS", "serial")
    _step(orc, ctx, combo, "serial bins")


@pytest.mark.parametrize("form", ["default", "serial"])
@pytest.mark.parametrize("combo", S.ONE_BIN_COMBOS, ids=S.combo_id)
def test_one_bin_step(orc, ctx, monkeypatch, combo, form):
    """the whole graph as ONE bin: columns with more sources than a staged chunk (band) and than three (hub)"""
    monkeypatch.setenv("DSSS_PG_BIN_COST", repr(1e12))
    if form == "serial":
        monkeypatch.setenv("DSSS_PG_BINS", "serial")
    _step(orc, ctx, combo, "one bin, " + form)

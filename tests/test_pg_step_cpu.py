"""tests/pg_step_ref.py on the oracle alone: every combination tests/test_gpu_pg_step.py runs has to qualify, chain_seams has the gaps it is
built for, and the SENSITIVITY test: a linear solve that is wrong by 1e-4 relative in one separator passes everything a converged run is
held to (tests/test_gpu_pg_paths.py) and misses the one-step bar by more than a factor 100.  That gap is what the one-step comparison closes;
the test keeps it from reopening unnoticed (a bar that grew, a reference that lost its refinement)."""
import numpy as np
import pytest

from tests import pg_paths_ref as P
from tests import pg_step_ref as S


@pytest.fixture(scope="module")
def table(orc):
    out = {}
    print()
    for c in S.COMBOS + list(S.REFUSED_BY_RULE_C):
        name, steps, params = c
        q = out[c] = S.qualify(orc, name, steps, **dict(params))
        print("%-32s %-3s %-13s step %-9.3g s %-9.3g floor %-9.3g bar %-9.3g references agree to %-9.3g rounding margin %-9.3g %s"
              % (S.combo_id(c), "ok" if q["ok"] else "NO", q["path"], q["step"], q["s"], q["floor"], q["bar"], q["agree"], q["margin"], "; ".join(q["why"])))
    return out


def test_every_combination_of_the_gpu_file_qualifies(table):
    used = set(S.TOPOLOGY_COMBOS + S.DAMPING_COMBOS + S.REFUSED_COMBOS + S.SERIAL_COMBOS + S.ONE_BIN_COMBOS)
    assert used == set(S.COMBOS)                                                 # the serial and one-bin runs reuse topology combinations
    bad = {S.combo_id(c): table[c]["why"] for c in S.COMBOS if not table[c]["ok"]}
    assert not bad, bad
    for c in S.COMBOS:
        assert table[c]["iters"] == c[1] and table[c]["path"].count("A") == c[1] and table[c]["path"][-1] == "A"
        assert table[c]["bar"] == S.margin(c[0], c[1], **dict(c[2])) * max(table[c]["s"], table[c]["floor"])
    assert set(S.MARGIN_OF) <= set(S.COMBOS) and len(S.MARGIN_OF) == 1           # one raised margin, and rules (d), (e) hold with it (above)


def test_the_combinations_left_out_are_the_ones_rule_c_refuses(table):
    """every topology at one and at two steps, but for the two that rule (c) -- and rule (c) alone -- refuses"""
    every = {(name, steps, ()) for name in S.TOPOLOGIES for steps in (1, 2)}
    assert every - set(S.TOPOLOGY_COMBOS) == set(S.REFUSED_BY_RULE_C)
    for c in S.REFUSED_BY_RULE_C:
        q = table[c]
        assert not q["ok"] and all(w.startswith("(c)") for w in q["why"]), (c, q["why"])
        assert q["agree"] <= 2 * q["floor"]                                      # ... by less than 8 eps max |X|


def test_refused_trials_come_before_the_compared_step(table):
    assert table[("reject_then_accept", 1, ())]["path"] == "RRRRRRRA"
    assert table[("interleaved", 2, ())]["path"] == "ARRRRRRRRRRA"
    assert table[("accept_then_reject", 2, ())]["path"] == "ARRRRRRRRRA"


def test_reference_is_cached_and_starts_where_the_lm_starts(orc):
    r1, r2 = S.reference(orc, "band", 1), S.reference(orc, "band", 2)
    assert S.reference(orc, "band", 1) is r1
    assert r1.X0.tobytes() == r2.X0.tobytes() == S.reference(orc, "band", 0).X.tobytes()
    assert r1.step == float(np.abs(r1.X - r1.X0).max()) and r2.step == float(np.abs(r2.X - r1.X).max())
    assert r1.p.max_iters == 1 and r2.p.max_iters == 2 and r1.stats[0] == 1 and r2.stats[0] == 2
    r = S.reference(orc, "band", 1, lambda0=1e3)
    assert r.p.lambda0 == 1e3 and r.X.tobytes() != r1.X.tobytes() and r.X0.tobytes() == r1.X0.tobytes()
    assert S.bar(orc, "band", 1) == S.MARGIN * max(S.spread(orc, "band", 1), S.floor(orc, "band", 1))


def test_chain_seams_has_the_gaps_it_is_built_for(orc):
    dr, e, p = S.build(orc, "chain_seams", 1)
    assert len(dr) == 1380 and len(e) == 12 and (e["a"] < e["b"]).all()
    m = S.seam_separators()
    assert not (m % S.CHUNK == 0).any()
    assert sorted(np.unique(np.concatenate([e["a"], e["b"]])).tolist()) == m.tolist()
    prof = S.seam_profile(dr, e)
    print("chain_seams gaps (length, inserted separators):", prof)
    assert [g for g, _k in prof] == [S.SEAM_LEAD] + list(S.SEAM_GAPS[1:]) + [len(dr) - 1 - int(m[-1])]
    run = S.RUN * S.CHUNK
    assert any(k >= 1 for _g, k in prof)                                         # a gap that receives a chunk end as an extra separator
    assert any(k == 0 and run - S.CHUNK < g <= run + S.CHUNK for g, k in prof)   # ... and one within a chunk of that length that does not
    assert {g for g, k in prof if k} == {272, 273} and S._reduced(dr, e)[0] == len(m) + 2 + 2
    for g in (1, 2, S.CHUNK - 1, S.CHUNK, S.CHUNK + 1, run - 1, run, run + 1):
        assert g in [x for x, _k in prof]


# ---------------------------------------------------------------- the sensitivity test
FAULT = 1e-4


def _faulty(ns, x):
    """the 6-vector of separator ns // 2 of the reduced solution, scaled by 1 + FAULT"""
    x = x.copy()
    x[6 * (ns // 2):6 * (ns // 2) + 6] *= 1.0 + FAULT
    return x


@pytest.mark.parametrize("name", ["clique", "hub", "band", "chain_seams"])
def test_a_faulty_linear_solve_passes_the_converged_run_and_misses_the_one_step_bar(orc, name):
    dr, e, p = S.CASES[name](orc)
    Xc, sc, _tc, pathc, ntc = orc.pg_solve_path(dr, e, p, solver="sparse")
    Xf, sf, _tf, pathf, ntf = orc.pg_solve_path(dr, e, p, solver="sparse", reduced_post=_faulty)
    converged = float(np.abs(Xf - Xc).max())
    ref = S.reference(orc, name, 1)
    X1 = orc.pg_solve_path(ref.dr, ref.e, ref.p, solver="sparse", reduced_post=_faulty)[0]
    one_step, bar = float(np.abs(X1 - ref.X).max()), S.bar(orc, name, 1)
    print("%-12s fault %g: converged run %s | %s, iterations %d | %d, lambda %g | %g, max |dpose| %.3g, objective %.3g relative; one step %.3g against a bar of %.3g (x %.3g)"
          % (name, FAULT, P.path_string(pathf), P.path_string(pathc), sf[0], sc[0], sf[3], sc[3], converged, abs(sf[2] - sc[2]) / sc[2], one_step, bar, one_step / bar))
    # what the converged comparisons see: nothing
    assert P.path_string(pathf) == P.path_string(pathc) and ntf == ntc and sf[0] == sc[0] and sf[3] == sc[3]
    assert converged <= P.POSE_BAR / 10
    assert abs(sf[2] - sc[2]) <= P.OBJ_BAR / 10 * sc[2]
    # what one step sees
    assert one_step > 100 * bar


def test_the_hook_unused_changes_nothing(orc):
    """reduced_post = None is the binding as it was; the identity as the hook gives the same bytes and is called once per reduced solve"""
    dr, e, p = S.build(orc, "band", 2)
    calls = []

    def identity(ns, x):
        calls.append(ns)
        return x
    for fr in (0, 2):
        del calls[:]
        a = orc.pg_solve_path(dr, e, p, solver="sparse", full_refine=fr)
        b = orc.pg_solve_path(dr, e, p, solver="sparse", full_refine=fr, reduced_post=identity)
        assert all(u.tobytes() == v.tobytes() for u, v in zip(a[:4], b[:4])) and a[4] == b[4]
        assert len(calls) == a[4] * (1 + fr) and len(set(calls)) == 1
    X, st = orc.pg_solve(dr, e, p, solver="sparse")
    assert X.tobytes() == orc.pg_solve_path(dr, e, p, solver="sparse")[0].tobytes()
    with pytest.raises(AssertionError):
        orc.pg_solve(dr, e, p, solver="envelope", reduced_post=identity)         # the envelope Cholesky never leaves the C file

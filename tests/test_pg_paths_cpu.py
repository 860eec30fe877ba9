"""The cases of tests/pg_paths_ref.py on the oracle alone: before the device is compared on them (tests/test_gpu_pg_paths.py) every case
has to qualify -- no decision near its threshold, no decision on rounding, three linear solvers on one path -- and has to take the exit it
is named for, read from the record of EVERY trial (orc_pg_solve_path).  Changing a seed, an angle or a variance there fails here first."""
import re

import numpy as np
import pytest

from tests import pg_paths_ref as P


@pytest.fixture(scope="module")
def table(orc):
    """qualify() of every case, once; printed as the table of paths, exits and margins"""
    out = {name: P.qualify(orc, name) for name in P.CASES if name != "tiny_1"}
    print()
    for name, q in out.items():
        print("%-22s %-5s trials %2d iters %2d lambda %-8.3g exit %-17s rounding margin %-9.3g solvers: poses %.1e objective %.1e  %s %s"
              % (name, "ok" if q["ok"] else "NO", q["ntrials"], q["iters"], q["lam"], q["exit"], q["margin"], q["spread_pose"], q["spread_obj"], q["path"],
                 "; ".join(q["why"])))
    return out


def test_every_case_qualifies(table):
    bad = {n: q["why"] for n, q in table.items() if not q["ok"]}
    assert not bad, bad
    assert set(table) == set(P.CASES) - {"tiny_1"}                              # (one pose: no trial to qualify; the device refuses it)


def test_lm_cases_take_the_paths_they_are_named_for(orc, table):
    t = table
    def alternations(s):
        s = re.sub("[NF]", "R", s)
        return sum(1 for a, b in zip(s, s[1:]) if a != b)
    assert re.match("R{3,}A", t["reject_then_accept"]["path"])
    q = t["accept_then_reject"]                                                 # accepts, each followed by rejections only, the last run of them to lambda_max:
    assert re.fullmatch("(A+R{3,}){1,2}", q["path"]) and q["exit"] == "lambda_max" and alternations(q["path"]) < 4 <= alternations(t["interleaved"]["path"])
    assert q["iters"] == q["path"].count("A") > 0
    assert alternations(t["interleaved"]["path"]) >= 4
    assert t["all_rejected_lammax"]["iters"] == 0 and t["all_rejected_lammax"]["exit"] == "lambda_max" and set(t["all_rejected_lammax"]["path"]) == {"R"}
    q = t["stop_after_reject"]
    assert q["exit"] == "stop_after_reject" and q["iters"] > 0 and q["path"].endswith("AR") and q["lam"] < P.build(orc, "stop_after_reject")[2].lambda_max
    for name, field, value in (("lambda0_1e-12", "lambda0", 1e-12), ("lambda0_1e8", "lambda0", 1e8), ("lambda_factor_2", "lambda_factor", 2.0),
                               ("lambda_factor_100", "lambda_factor", 100.0), ("lambda_max_1e-3", "lambda_max", 1e-3), ("min_fidelity_0.5", "min_fidelity", 0.5),
                               ("min_fidelity_0.9", "min_fidelity", 0.9), ("max_iters_1", "max_iters", 1), ("max_iters_2", "max_iters", 2)):
        assert getattr(P.build(orc, name)[2], field) == value
    # the parameters change the path: the final lambda is lambda0 * factor^(rejections - accepts) as long as no exit cuts it short
    for name in ("lambda0_1e-12", "lambda0_1e8", "lambda_factor_2", "lambda_factor_100"):
        p = P.build(orc, name)[2]; s = t[name]["path"]
        assert np.isclose(t[name]["lam"], p.lambda0 * p.lambda_factor ** (s.count("R") - s.count("A")), rtol=1e-9), name
    assert t["lambda0_1e8"]["iters"] >= 10
    assert "R" in t["lambda_factor_2"]["path"] and "R" in t["lambda_factor_100"]["path"]
    assert t["lambda_factor_2"]["path"].count("R") > t["reject_then_accept"]["path"].count("R") > t["lambda_factor_100"]["path"].count("R")
    assert t["lambda_max_1e-3"]["path"] == "RR" and t["lambda_max_1e-3"]["exit"] == "lambda_max"
    assert t["max_iters_1"]["exit"] == "max_iters" and t["max_iters_2"]["exit"] == "max_iters" and (t["max_iters_1"]["iters"], t["max_iters_2"]["iters"]) == (1, 2)
    assert t["abs_tol_early"]["exit"] == "abs_tol"
    assert set(t["factor_fails"]["path"]) == {"F"} and t["factor_fails"]["iters"] == 0 and t["factor_fails"]["exit"] == "lambda_max"


def test_parameters_turn_a_plain_run_into_another(orc, table):
    """min_fidelity 0.5 / 0.9 reject a trial the default accepts; max_iters and abs_tol stop a descent that goes on without them"""
    dr, e, p = P.build(orc, "min_fidelity_0.5")
    plain = orc.pg_solve_path(dr, e, P._params(orc, add_noise=0))
    s = P.path_string(plain[3])
    first = s.index("A")
    assert 1e-3 < plain[3][first, 2] < 0.25 and plain[1][0] > 0                 # accepted by the default, far below both thresholds
    for name in ("min_fidelity_0.5", "min_fidelity_0.9"):
        assert table[name]["path"] == "R" * len(table[name]["path"]) and len(table[name]["path"]) > first
    dr, e, p = P.build(orc, "abs_tol_early")
    full = orc.pg_solve_path(dr, e, P._params(orc))
    assert int(full[1][0]) == table["abs_tol_early"]["iters"] + 1 == table["max_iters_2"]["iters"] + 2


def test_path_entry_point_returns_the_plain_results(orc):
    """orc_pg_solve_path runs the loop of orc_pg_solve_init and orc_pg_solve: same bytes out, the decided trials of the path are the trace,
    and the count is the length of the path"""
    for name in ("interleaved", "reject_then_accept", "factor_fails", "max_iters_2", "tiny_3", "ends"):
        dr, e, p = P.build(orc, name)
        for solver in ("envelope", "sparse"):
            X0, st0 = orc.pg_solve(dr, e, p, solver=solver)
            X1, st1, tr1 = orc.pg_solve_init(dr, e, p, solver=solver)
            X2, st2, tr2, path, nt = orc.pg_solve_path(dr, e, p, solver=solver)
            assert X0.tobytes() == X1.tobytes() == X2.tobytes() and st0.tobytes() == st1.tobytes() == st2.tobytes() and tr1.tobytes() == tr2.tobytes()
            assert nt == len(path)
            decided = path[path[:, 5] == orc.PG_TRIAL_DECIDED]
            assert decided[:, :5].tobytes() == tr2.tobytes()
            assert np.isnan(path[path[:, 5] != orc.PG_TRIAL_DECIDED][:, 1:3]).all()
            assert int(path[:, 4].sum()) == int(st2[0])
    dr, e, p = P.build(orc, "interleaved")                                      # a short path buffer still counts every trial
    assert orc.pg_solve_path(dr, e, p, path_cap=5)[4] == 44


def test_host_twin_reports_the_intended_fronts(orc):
    """the analysis (host twin, no GPU) of the reduced graphs: random_pairs has a front tall enough for pg_front_bwd_part_kernel and for a
    level above PG_RSU32_MAX_TILES at the smallest size on the grid; the 40-pose clique goes to the binned subtrees, clique_48 is one front
    of four panels; the hub and the band for the record"""
    st = {name: P.twin_stats(*P.build(orc, name)[:2]) for name in ("random_pairs", "clique", "clique_48", "hub", "band", "wild_variances")}
    for name, s in st.items():
        print("%-16s nnzL %6d fronts %3d panels %3d levels %3d binned columns %4d largest front %4d block rows" % (name, s[0], s[1], s[2], s[3], s[6], s[7]))
    assert st["random_pairs"][7] >= P.FRONT_ROWS_FOR_BWD_SPLIT > P.FRONT_ROWS_FOR_RSU32
    # ... and for a level above PG_RSU_MAX_TILES: separate row solve and update first, then the fused kernel at 64 x 64, then its quarters
    assert P.level_tiles_at_least(6 * st["random_pairs"][7] - 96) > P.PG_RSU_MAX_TILES
    n, ne = P.RANDOM_PAIRS
    smaller = P._random_pairs(orc, n - 50, int(0.75 * (n - 50)))
    assert P.twin_stats(*smaller[:2])[7] < P.FRONT_ROWS_FOR_BWD_SPLIT           # ... and one step down the grid it is not
    assert st["clique"][7] < 33 and st["clique"][6] >= 28                       # 40 poses: binned, no front wider than two panels (16 block columns each)
    assert st["clique_48"][1] == 1 and st["clique_48"][7] >= 48 and st["clique_48"][2] >= 3      # 48 poses: one front, more than two 96-column panels
    assert st["band"][1] >= 2 and st["hub"][6] >= 290                           # the star is all leaves


def test_case_shapes(orc):
    dr, e, _ = P.build(orc, "hub");            assert len(e) == 300 and len(np.unique(e["a"])) + len(np.unique(e["b"])) >= 300 and ((e["a"] == 600) | (e["b"] == 600)).all()
    dr, e, _ = P.build(orc, "clique");         assert len(e) == 780
    dr, e, _ = P.build(orc, "band");           assert len(e) == sum(min(4, max(0, len(dr) - 2 - a)) for a in range(len(dr))) and ((e["b"] - e["a"] >= 2) & (e["b"] - e["a"] <= 5)).all()
    dr, e, _ = P.build(orc, "ends");           n = len(dr); assert sorted(zip(e["a"].tolist(), e["b"].tolist())) == sorted([(0, n - 1), (0, 1), (n - 1, n - 2), (1, n - 1)])
    dr, e, _ = P.build(orc, "wild_variances"); assert len(e) == 200 and len(set(zip(e["a"].tolist(), e["b"].tolist()))) == 200 and e["var"].min() < 1e-9 and e["var"].max() > 10
    for n in (1, 2, 3, 7):
        dr, e, p = P.build(orc, "tiny_%d" % n); assert len(dr) == n and p.add_noise == 0 and len(e) == (n > 1)
    dr, e, p = P.build(orc, "factor_fails")
    assert (e["var"] > 0).all() and np.isfinite(e["var"]).all() and np.isfinite(1.0 / np.sqrt(e["var"])).all() and 1.0 / e["var"].min() > np.finfo(np.float64).max / 40.0 ** 2

// diasss_amd/host/lm_rule_check.cpp -- truth table of the LM decisions in csrc/dsss_lm.h (host side; the kernels compile the same text).
// The rows and their expected columns are in lm_rule_table.h, written by hand from the rule as oracle/orc_lc.c states it (its lines 208-236):
// nothing there is computed by the header under test.  The device probe (dev_probe.hip) walks the same rows on the GPU.
// Stand-alone, built with the host sanitizers; needs no GPU and no libdsss.
#include "lm_rule_table.h"
#include <cstdio>

static int bad = 0;
static void expect(bool got, bool want, const char* what, int row)
{
    if (got != want) { std::printf("FAIL %s, row %d: got %d, expected %d\n", what, row, (int)got, (int)want); ++bad; }
}

int main()
{
    const lm_rule R = lm_gtsam_defaults();
    expect(R.relTol == 1e-5 && R.absTol == 1e-5 && R.lamMax == 1e5 && R.minFid == 1e-3 && R.factor == 10.0 && R.maxIter == 100, true, "GTSAM defaults", 0);

    for (int i = 0; i < LM_VERDICT_ROWS; ++i) {
        const lm_verdict_row V = lm_table_verdict(i);
        const lm_verdict v = lm_judge(lm_table_rule(V.rule), V.oldLin, V.newLin, V.err, V.newErr);
        expect(lm_descends(V.oldLin, V.newLin), V.descends, "lm_descends", i);
        expect(v.success, V.success, "success", i); expect(v.stop, V.stop, "stop", i);
    }
    for (int i = 0; i < LM_LAMBDA_ROWS; ++i) {
        const lm_lambda_row S = lm_table_lambda(i);
        const lm_lambda_got g = lm_table_lambda_run(S);
        expect(g.early == 0, true, "no refusal before the last gives up", i);
        expect(g.gave_up, S.gives_up, "gives up", i);
        if (S.next >= 0) expect(g.next == S.next, true, "the next lambda", i);
    }
    for (int i = 0; i < LM_CONTINUE_ROWS; ++i) {
        const lm_continue_row C = lm_table_continue(i);
        expect(lm_continue(lm_table_rule(C.rule), C.iters, C.cur, C.err), C.go, "lm_continue", i);
    }

    if (bad) { std::printf("lm_rule_check: %d failures\n", bad); return 1; }
    std::printf("lm_rule_check: ok\n");
    return 0;
}

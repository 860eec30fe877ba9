// diasss_amd/host/lm_rule_check.cpp -- truth table of the LM decisions in csrc/dsss_lm.h (host side; the kernels compile the same text).
// The expected column is written by hand from the rule as oracle/orc_lc.c states it (its lines 208-236): nothing here is computed by the header.
// Stand-alone, built with the host sanitizers; needs no GPU and no libdsss.
#include "../csrc/dsss_lm.h"
#include <cstdio>
#include <limits>

static int bad = 0;
static void expect(bool got, bool want, const char* what, int row)
{
    if (got != want) { std::printf("FAIL %s, row %d: got %d, expected %d\n", what, row, (int)got, (int)want); ++bad; }
}

int main()
{
    const lm_rule R = lm_gtsam_defaults();
    const double eps = 2.220446049250313e-16;               // 2^-52: 1 - eps and 1 - 2 eps are doubles, and 1 - (1 - eps) == eps exactly
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double p17 = 1.0 / 131072, p16 = 1.0 / 65536, p20 = 1.0 / 1048576;      // 7.6e-6 < relTol * 1 = 1e-5 < 1.5e-5; all exact
    expect(R.relTol == 1e-5 && R.absTol == 1e-5 && R.lamMax == 1e5 && R.minFid == 1e-3 && R.factor == 10.0 && R.maxIter == 100, true, "GTSAM defaults", 0);

    // ---- the verdict: linChange = oldLin - newLin; nothing unless linChange >= 0; success = linChange > eps * oldLin && costChange / linChange > minFid;
    //      stop = |costChange| < relTol * err, costChange = err - newErr
    const struct { double oldLin, newLin, err, newErr; bool descends, success, stop; } V[] = {
        { 1, 2, 1, 0.5,                0, 0, 0 },      //  0 linChange negative: nothing, however good the cost
        { 1, 1, 1, 0.5,                1, 0, 0 },      //  1 linChange zero: not above eps * oldLin
        { 1, 1, 1, 1,                  1, 0, 1 },      //  2 linChange zero, cost unchanged: stop without success
        { 1, 1 - eps, 1, 0,            1, 0, 0 },      //  3 linChange exactly eps * oldLin: `>` is strict
        { 1, 1 - 2 * eps, 1, 0,        1, 1, 0 },      //  4 just above it: fidelity 1 / (2 eps)
        { 2, 1, 1e-3, 0,               1, 0, 0 },      //  5 fidelity exactly minFid: `>` is strict
        { 2, 1, 0.0005, 0,             1, 0, 0 },      //  6 fidelity below
        { 2, 1, 0.002, 0,              1, 1, 0 },      //  7 fidelity above
        { 2, 1, 1, 2,                  1, 0, 0 },      //  8 the cost rises: negative fidelity
        { 2, 1, 1, 1 - p17,            1, 0, 1 },      //  9 |costChange| = 2^-17 < 1e-5: stop; fidelity 7.6e-6
        { 2, 1, 1, 1 - p16,            1, 0, 0 },      // 10 |costChange| = 2^-16 > 1e-5: no stop
        { 1, 1 - p20, 1, 1 - p17,      1, 1, 1 },      // 11 fidelity 8 and a small cost change: success and stop
        { 1, 0.5, 0, 0,                1, 0, 0 },      // 12 err == 0: fidelity 0, and 0 < relTol * 0 is false
        { 2, 1, 1, nan,                1, 0, 0 },      // 13 newErr NaN: every comparison false
        { 2, 1, 1, inf,                1, 0, 0 },      // 14 newErr infinite
        { 1, nan, 1, 0.5,              0, 0, 0 },      // 15 linear error NaN: linChange >= 0 is false
    };
    for (int i = 0; i < (int)(sizeof V / sizeof V[0]); ++i) {
        const lm_verdict v = lm_judge(R, V[i].oldLin, V[i].newLin, V[i].err, V[i].newErr);
        expect(lm_descends(V[i].oldLin, V[i].newLin), V[i].descends, "lm_descends", i);
        expect(v.success, V[i].success, "success", i); expect(v.stop, V[i].stop, "stop", i);
    }

    // ---- the lambda schedule: lambda *= factor, give up when lambda >= lamMax; lambda /= factor after an accepted step
    double lam = 1e4;
    expect(lm_refused(R, &lam), true, "lambda reaches lamMax exactly", 0); expect(lam == 1e5, true, "1e4 * 10", 0);
    lam = 1e3;
    expect(lm_refused(R, &lam), false, "one step below lamMax", 1); expect(lam == 1e4, true, "1e3 * 10", 1);
    lam = 1e-5;                                             // the start value: the tenth refusal in a row is the one that gives up (orc_lc.c's trace: failures come in tens)
    for (int k = 1; k <= 10; ++k) expect(lm_refused(R, &lam), k == 10, "refusals from 1e-5", k);
    lam = 1e-5; lm_accepted(R, &lam);
    expect(lam == 1e-5 / 10, true, "lambda /= 10", 0);
    const lm_rule Q = { 1e-3, 1e-2, 8.0, 0.25, 2.0, 3 };    // other constants (the pose-graph LM fills them from its parameters)
    lam = 4; expect(lm_refused(Q, &lam), true, "factor 2, lamMax 8", 0); expect(lam == 8, true, "4 * 2", 0);
    lam = 4; lm_accepted(Q, &lam); expect(lam == 2, true, "4 / 2", 0);
    expect(lm_judge(Q, 2, 1, 0.25, 0).success, false, "minFid 0.25, at", 0); expect(lm_judge(Q, 2, 1, 0.5, 0).success, true, "minFid 0.25, above", 1);

    // ---- the outer condition: iters < maxIter && !(err <= 0 || (cur - err) / cur <= relTol || cur - err <= absTol) && isfinite(cur)
    const struct { int iters; double cur, err; bool go; } C[] = {
        { 99, 2, 1,                    1 },             //  0 maxIter - 1
        { 100, 2, 1,                   0 },             //  1 maxIter
        { 5, 1, 0,                     0 },             //  2 err == 0
        { 5, 1, 1 - p17,               0 },             //  3 relative decrease 7.6e-6 <= relTol
        { 5, 1, 1 - p16,               1 },             //  4 relative and absolute decrease 1.5e-5: both above
        { 5, 1e-3, 0.5e-3,             1 },             //  5 relative 0.5, absolute 5e-4
        { 5, 1e-5, 0.5e-5,             0 },             //  6 relative 0.5, absolute 5e-6 <= absTol
        { 5, 1, 2,                     0 },             //  7 no decrease (a search that stopped without success leaves cur == err)
        { 5, 1, 1,                     0 },             //  8 the same, exactly
        { 5, inf, 1,                   0 },             //  9 cur infinite: inf / inf is NaN, the tests pass, isfinite does not
        { 5, nan, nan,                 0 },             // 10 cur NaN
        { 5, 1, nan,                   1 },             // 11 err NaN under a finite cur: no comparison holds, the loop goes on
    };
    for (int i = 0; i < (int)(sizeof C / sizeof C[0]); ++i) expect(lm_continue(R, C[i].iters, C[i].cur, C[i].err), C[i].go, "lm_continue", i);
    expect(lm_continue(Q, 2, 2, 1), true, "maxIter 3, iters 2", 0); expect(lm_continue(Q, 3, 2, 1), false, "maxIter 3, iters 3", 1);

    if (bad) { std::printf("lm_rule_check: %d failures\n", bad); return 1; }
    std::printf("lm_rule_check: ok\n");
    return 0;
}

// diasss_amd/host/lm_rule_table.h -- the truth table of the LM decisions in csrc/dsss_lm.h, for the host program under the host sanitizers
// (lm_rule_check.cpp) and for the device probe (dev_probe.hip, function id 19): both walk the same rows.
// The expected columns are written by hand from the rule as oracle/orc_lc.c states it (its lines 208-236): nothing here is computed by dsss_lm.h.
// The rows live in functions, not in namespace-scope arrays, so that the same text compiles for the host and for the device.
#pragma once
#include "../csrc/dsss_lm.h"

#define LMT_EPS 2.220446049250313e-16               // 2^-52: 1 - eps and 1 - 2 eps are doubles, and 1 - (1 - eps) == eps exactly
#define LMT_INF __builtin_inf()
#define LMT_NAN __builtin_nan("")
#define LMT_P17 (1.0 / 131072)                      // 7.6e-6 < relTol * 1 = 1e-5 < 1.5e-5 = LMT_P16; all exact
#define LMT_P16 (1.0 / 65536)
#define LMT_P20 (1.0 / 1048576)

// rule 0: GTSAM's defaults; rule 1: other constants (the pose-graph LM fills them from its parameters)
PDEV lm_rule lm_table_rule(int which) { if (which == 0) return lm_gtsam_defaults(); return { 1e-3, 1e-2, 8.0, 0.25, 2.0, 3 }; }

// ---- the verdict: linChange = oldLin - newLin; nothing unless linChange >= 0; success = linChange > eps * oldLin && costChange / linChange > minFid;
//      stop = |costChange| < relTol * err, costChange = err - newErr
struct lm_verdict_row { int rule; double oldLin, newLin, err, newErr; bool descends, success, stop; };
enum { LM_VERDICT_ROWS = 18 };
PDEV lm_verdict_row lm_table_verdict(int i)
{
    const lm_verdict_row V[LM_VERDICT_ROWS] = {
        { 0, 1, 2, 1, 0.5,                          0, 0, 0 },      //  0 linChange negative: nothing, however good the cost
        { 0, 1, 1, 1, 0.5,                          1, 0, 0 },      //  1 linChange zero: not above eps * oldLin
        { 0, 1, 1, 1, 1,                            1, 0, 1 },      //  2 linChange zero, cost unchanged: stop without success
        { 0, 1, 1 - LMT_EPS, 1, 0,                  1, 0, 0 },      //  3 linChange exactly eps * oldLin: `>` is strict
        { 0, 1, 1 - 2 * LMT_EPS, 1, 0,              1, 1, 0 },      //  4 just above it: fidelity 1 / (2 eps)
        { 0, 2, 1, 1e-3, 0,                         1, 0, 0 },      //  5 fidelity exactly minFid: `>` is strict
        { 0, 2, 1, 0.0005, 0,                       1, 0, 0 },      //  6 fidelity below
        { 0, 2, 1, 0.002, 0,                        1, 1, 0 },      //  7 fidelity above
        { 0, 2, 1, 1, 2,                            1, 0, 0 },      //  8 the cost rises: negative fidelity
        { 0, 2, 1, 1, 1 - LMT_P17,                  1, 0, 1 },      //  9 |costChange| = 2^-17 < 1e-5: stop; fidelity 7.6e-6
        { 0, 2, 1, 1, 1 - LMT_P16,                  1, 0, 0 },      // 10 |costChange| = 2^-16 > 1e-5: no stop
        { 0, 1, 1 - LMT_P20, 1, 1 - LMT_P17,        1, 1, 1 },      // 11 fidelity 8 and a small cost change: success and stop
        { 0, 1, 0.5, 0, 0,                          1, 0, 0 },      // 12 err == 0: fidelity 0, and 0 < relTol * 0 is false
        { 0, 2, 1, 1, LMT_NAN,                      1, 0, 0 },      // 13 newErr NaN: every comparison false
        { 0, 2, 1, 1, LMT_INF,                      1, 0, 0 },      // 14 newErr infinite
        { 0, 1, LMT_NAN, 1, 0.5,                    0, 0, 0 },      // 15 linear error NaN: linChange >= 0 is false
        { 1, 2, 1, 0.25, 0,                         1, 0, 0 },      // 16 minFid 0.25, at
        { 1, 2, 1, 0.5, 0,                          1, 1, 0 },      // 17 minFid 0.25, above (|costChange| = 0.5 is not below relTol * err = 5e-4)
    };
    return V[i];
}

// ---- the lambda schedule: lambda *= factor, give up when lambda >= lamMax; lambda /= factor after an accepted step.
// A row refuses `refusals` times in a row from lambda (0: one accepted step instead); only the LAST refusal may give up, and does if `gives_up`.
// next: the lambda afterwards, or a negative number where the row does not state it.
struct lm_lambda_row { int rule; double lambda; int refusals; bool gives_up; double next; };
enum { LM_LAMBDA_ROWS = 6 };
PDEV lm_lambda_row lm_table_lambda(int i)
{
    const lm_lambda_row S[LM_LAMBDA_ROWS] = {
        { 0, 1e4, 1,        1, 1e5 },               //  0 lambda reaches lamMax exactly
        { 0, 1e3, 1,        0, 1e4 },               //  1 one step below lamMax
        { 0, 1e-5, 10,      1, -1 },                //  2 the start value: the tenth refusal in a row is the one that gives up (orc_lc.c's trace: failures come in tens)
        { 0, 1e-5, 0,       0, 1e-5 / 10 },         //  3 lambda /= 10
        { 1, 4, 1,          1, 8 },                 //  4 factor 2, lamMax 8
        { 1, 4, 0,          0, 2 },                 //  5 4 / 2
    };
    return S[i];
}
struct lm_lambda_got { int early; bool gave_up; double next; };      // early: refusals before the last one that gave up
PDEV lm_lambda_got lm_table_lambda_run(const lm_lambda_row& s)
{
    const lm_rule R = lm_table_rule(s.rule);
    lm_lambda_got g = { 0, false, s.lambda };
    if (s.refusals == 0) { lm_accepted(R, &g.next); return g; }
    for (int k = 1; k <= s.refusals; ++k) {
        const bool up = lm_refused(R, &g.next);
        if (k < s.refusals) g.early += up; else g.gave_up = up;
    }
    return g;
}

// ---- the outer condition: iters < maxIter && !(err <= 0 || (cur - err) / cur <= relTol || cur - err <= absTol) && isfinite(cur)
struct lm_continue_row { int rule; int iters; double cur, err; bool go; };
enum { LM_CONTINUE_ROWS = 14 };
PDEV lm_continue_row lm_table_continue(int i)
{
    const lm_continue_row C[LM_CONTINUE_ROWS] = {
        { 0, 99, 2, 1,                    1 },             //  0 maxIter - 1
        { 0, 100, 2, 1,                   0 },             //  1 maxIter
        { 0, 5, 1, 0,                     0 },             //  2 err == 0
        { 0, 5, 1, 1 - LMT_P17,           0 },             //  3 relative decrease 7.6e-6 <= relTol
        { 0, 5, 1, 1 - LMT_P16,           1 },             //  4 relative and absolute decrease 1.5e-5: both above
        { 0, 5, 1e-3, 0.5e-3,             1 },             //  5 relative 0.5, absolute 5e-4
        { 0, 5, 1e-5, 0.5e-5,             0 },             //  6 relative 0.5, absolute 5e-6 <= absTol
        { 0, 5, 1, 2,                     0 },             //  7 no decrease (a search that stopped without success leaves cur == err)
        { 0, 5, 1, 1,                     0 },             //  8 the same, exactly
        { 0, 5, LMT_INF, 1,               0 },             //  9 cur infinite: inf / inf is NaN, the tests pass, isfinite does not
        { 0, 5, LMT_NAN, LMT_NAN,         0 },             // 10 cur NaN
        { 0, 5, 1, LMT_NAN,               1 },             // 11 err NaN under a finite cur: no comparison holds, the loop goes on
        { 1, 2, 2, 1,                     1 },             // 12 maxIter 3, iters 2
        { 1, 3, 2, 1,                     0 },             // 13 maxIter 3, iters 3
    };
    return C[i];
}

// diasss_amd/csrc/dsss_lm.h -- the DECISIONS of GTSAM 4.2's LevenbergMarquardtOptimizer (diagonalDamping off, errorTol 0),
// written once for the three LM loops of the library: lc_kernel (16 lanes and LDS per problem), tri_kernel (a thread's registers) and
// pg_solve::lm_loop (a whole device).  Only the decisions are shared -- each loop keeps its own linear algebra and its own state.
// Every expression keeps the operands, order and comparisons of oracle/orc_lc.c (the independent copy); built with -ffp-contract=off.
#pragma once
#include "dsss_pose.h"

struct lm_rule { double relTol, absTol, lamMax, minFid, factor; int maxIter; };
PDEV lm_rule lm_gtsam_defaults() { return { 1e-5, 1e-5, 1e5, 1e-3, 10.0, 100 }; }      // LevenbergMarquardtParams()

struct lm_verdict { bool success, stop; };      // success: take the trial point; stop (without success): leave the lambda search

// tryLambda's gate, stated here and nowhere else: the linear model does not rise at the step.  Only then is newErr needed -- the kernels ask before
// they evaluate it -- and lm_judge asks again, so a caller that has newErr anyway (the pose graph) calls lm_judge alone.
PDEV bool lm_descends(double oldLin, double newLin) { return oldLin - newLin >= 0; }
// LevenbergMarquardtOptimizer::tryLambda on a step that solved: fidelity of the model, and the relative cost change that ends the search
PDEV lm_verdict lm_judge(const lm_rule& R, double oldLin, double newLin, double err, double newErr)
{
    lm_verdict v = { false, false };
    if (lm_descends(oldLin, newLin)) {
        const double linChange = oldLin - newLin, costChange = err - newErr;
        if (linChange > 2.220446049250313e-16 * oldLin) v.success = (costChange / linChange) > R.minFid;
        if (fabs(costChange) < R.relTol * err) v.stop = true;
    }
    return v;
}
PDEV void lm_accepted(const lm_rule& R, double* lambda) { *lambda /= R.factor; }
// a refused trial that did not stop: the next lambda; true = it reached lamMax, give up this iteration
PDEV bool lm_refused(const lm_rule& R, double* lambda) { *lambda *= R.factor; return *lambda >= R.lamMax; }
// NonlinearOptimizer::defaultOptimize's loop condition after an iteration that went from error cur to err
PDEV bool lm_continue(const lm_rule& R, int iters, double cur, double err)
{
    return iters < R.maxIter && !((err <= 0) || ((cur - err) / cur <= R.relTol) || ((cur - err) <= R.absTol)) && std::isfinite(cur);
}

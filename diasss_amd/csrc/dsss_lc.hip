// diasss_amd/csrc/dsss_lc.hip -- batched loop-closure measurements: one 15-DoF Levenberg-Marquardt problem per
// matched keypoint pair.  Restates Optimizer::LoopClosingTFs, graph_option = 0
// (/root/reference/src/core/optimizer.cpp:641-982): graph {Prior(X1, 1e-6), Between(X1, X2; DR odometry, adaptive
// sigmas :778), SssPoint(L1, X1), SssPoint(L1, X2)} (:773-786), GTSAM LM with default parameters (:815-822), marginal
// covariance of X2 (:956-959), score = ini/final - 2 (:853-896).  GTSAM semantics per SURVEY.md A.2/A.3 and
// oracle/orc_lc.c.  f64 VALU: 15 x 15 systems are far too small for MFMA; 16 lanes per problem.
#include "dsss_internal.h"
#include "dsss_pose.h"
#include "dsss_lm.h"
#include <algorithm>

#define MR 16
#define MD 15

struct mini_prob {
    pose_t prior, odo;
    double sig_prior[6], sig_odo[6], sig_s[2], sig_t[2];
    double slant_s, slant_t;
};
struct mini_val { double L[3]; pose_t X1, X2; };

// ---- 16 lanes per problem, four problems per wavefront.  The 16 x 15 Jacobian and the 15 x 15 systems live in LDS with one row per lane; every sum
// keeps the element-wise order of oracle/orc_lc.c (k ascending): the one-thread version's bits, with serial chains of O(15^2) instead of O(15^3).
#define LG 16                  // lanes per problem
#define LS 16                  // LDS row stride (doubles)
// The problem's constants and its current / trial values live in LDS too (the same 100 doubles on every lane: in registers they held the kernel at one
// wavefront per SIMD).  H and its Cholesky factor share one 15 x 16 array: H keeps its lower triangle ([i][j], j <= i), the factor goes into the other
// half transposed and shifted by a column (L(i, k), k <= i, at [k][i + 1]) -- H survives the retries of a trial with a larger lambda, and 4.9 KB per
// problem let eight workgroups share a compute unit's LDS (two wavefronts per SIMD).
#define LIDX(i, k) ((k) * LS + (i) + 1)
struct lc_lds { double J[MR * LS]; double H[MD * LS]; double r[MR]; mini_prob m; mini_val v, nv; };

// The pose algebra (two Logmaps with acos / sin / tan, two sss factors: a few hundred dependent f64 operations, 75 % of the kernel's cycles) comes in
// PAIRS of the same code on different data -- prior / between, source / target sss factor, retraction of X1 / X2, the two DR poses of the set-up --
// so lanes 0..7 of the group run the first of a pair and lanes 8..15 the second, and the results cross by one shuffle each.
__device__ inline void lc_bcast_pose(const pose_t& mine, int src, pose_t* out)
{
#pragma unroll
    for (int k = 0; k < 9; ++k) out->R[k] = __shfl(mine.R[k], src, LG);
#pragma unroll
    for (int k = 0; k < 3; ++k) out->t[k] = __shfl(mine.t[k], src, LG);
}
__device__ inline void lc_select_pose(bool second, const pose_t& a, const pose_t& b, pose_t* out)
{
#pragma unroll
    for (int k = 0; k < 9; ++k) out->R[k] = second ? b.R[k] : a.R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) out->t[k] = second ? b.t[k] : a.t[k];
}
// whitened residual r and Jacobian J.  With J: both go to LDS (lane `lane` clears row `lane` of J, lanes 0 and 8 write the entries of their
// halves and their halves of r).  Without J (error evaluation): r in registers on every lane.
__device__ static void mini_lin(const mini_prob& m, const mini_val& v, double* r, double* J, int lane)
{
    const bool hb = (lane & 8) != 0;                       // second half of the group: between factor, target's sss factor
    const bool wr = J && (lane & 7) == 0;
    if (J) {
#pragma unroll
        for (int c2 = 0; c2 < LS; ++c2) J[lane * LS + c2] = 0.0;
        __builtin_amdgcn_wave_barrier();
    }
    // first half:  PriorFactor   e = Logmap(prior^-1 X1), H = I
    // second half: BetweenFactor e = Logmap(meas^-1 h), h = X1^-1 X2, H1 = -Ad(h^-1), H2 = I
    pose_t t1, t2, E; double xi[6], rr[6];
    const pose_t* P = hb ? &v.X1 : &m.prior;               // (lane-dependent LDS addresses: one load per element)
    const pose_t* Q = hb ? &v.X2 : &v.X1;
    pose_between(P, Q, &t1);
    pose_between(&m.odo, &t1, &t2);                        // (unused by the first half)
    lc_select_pose(hb, t1, t2, &E);
    pose_log(&E, xi);
#pragma unroll
    for (int i = 0; i < 6; ++i) { const double sg = hb ? m.sig_odo[i] : m.sig_prior[i]; rr[i] = xi[i] / sg; }
    if (!J) {
#pragma unroll
        for (int i = 0; i < 6; ++i) { r[i] = __shfl(rr[i], 0, LG); r[6 + i] = __shfl(rr[i], 8, LG); }
    } else if (wr) {                                       // the linearisation keeps its residual in LDS (r = the group's S.r): sixteen registers less across the solve
#pragma unroll
        for (int i = 0; i < 6; ++i) r[(hb ? 6 : 0) + i] = rr[i];
    }
    if (J) {
        pose_t hi; double Ad[36];
        pose_inverse(&t1, &hi);                            // t1 = h on the second half
        pose_adjoint(&hi, Ad);
        if (wr && !hb) {
#pragma unroll
            for (int i = 0; i < 6; ++i) J[i * LS + 3 + i] = 1.0 / m.sig_prior[i];
        }
        if (wr && hb) {
#pragma unroll
            for (int i = 0; i < 6; ++i) {
#pragma unroll
                for (int j = 0; j < 6; ++j) J[(6 + i) * LS + 3 + j] = -Ad[6 * i + j] / m.sig_odo[i];
                J[(6 + i) * LS + 9 + i] = 1.0 / m.sig_odo[i];
            }
        }
    }
    // first half: SssPoint(L1, X1), second half: SssPoint(L1, X2)
    double ee[2], H1[6], H2[12], r2[2];
    const pose_t* X = hb ? &v.X2 : &v.X1;
    const double slant = hb ? m.slant_t : m.slant_s;
    const double sg0 = hb ? m.sig_t[0] : m.sig_s[0], sg1 = hb ? m.sig_t[1] : m.sig_s[1];
    sss_factor(v.L, X, slant, 0.0, ee, J ? H1 : nullptr, H2);
    r2[0] = ee[0] / sg0; r2[1] = ee[1] / sg1;
    if (!J) {
#pragma unroll
        for (int i = 0; i < 2; ++i) { r[12 + i] = __shfl(r2[i], 0, LG); r[14 + i] = __shfl(r2[i], 8, LG); }
    }
    if (wr) {
        const int row0 = hb ? 14 : 12, col0 = hb ? 9 : 3;
        r[row0] = r2[0]; r[row0 + 1] = r2[1];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const double sg = i ? sg1 : sg0;
#pragma unroll
            for (int j = 0; j < 3; ++j) J[(row0 + i) * LS + j] = H1[3 * i + j] / sg;
#pragma unroll
            for (int j = 0; j < 6; ++j) J[(row0 + i) * LS + col0 + j] = H2[6 * i + j] / sg;
        }
    }
    if (J) __builtin_amdgcn_wave_barrier();
}
// Out of line on purpose: inlined at its two call sites it costs lc_kernel 42 VGPRs and 25 spills.  mini_lin stays with the inliner, which takes it into
// mini_err and calls it from the kernel: forced out of line as well, mini_err would call it and the scratch grows from 64 to 208 B per lane.
__device__ static __noinline__ double mini_err(const mini_prob& m, const mini_val& v, int lane)
{
    double r[MR];
    mini_lin(m, v, r, nullptr, lane);
    double s = 0;
#pragma unroll
    for (int i = 0; i < MR; ++i) s += r[i] * r[i];
    return 0.5 * s;
}
// lane a < 15: row a of H = J^T J up to the diagonal, and g[a] = (J^T r)[a]
__device__ static double normal_eq(const double* J, const double* r, double* H, int lane)
{
    double g = 0;
    if (lane < MD) {
        double ca[MR];
#pragma unroll
        for (int k = 0; k < MR; ++k) ca[k] = J[k * LS + lane];
#pragma unroll
        for (int k = 0; k < MR; ++k) g += ca[k] * r[k];
        for (int b2 = 0; b2 < MD; ++b2) {
            double t = 0;
#pragma unroll
            for (int k = 0; k < MR; ++k) t += ca[k] * J[k * LS + b2];
            if (b2 <= lane) H[lane * LS + b2] = t;
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    __builtin_amdgcn_wave_barrier();
    return g;
}
// lower Cholesky of A = H + lambda I into L (LDS, the LIDX half of the array H lives in): lane i owns row i in registers; returns 0 on success (uniform
// over the group).  Column j: lanes i >= j subtract sum_k L(i,k) L(j,k), k ascending, exactly as the sequential form.
__device__ static int chol15(const double* H, double lambda, double* L, int lane)
{
    double row[MD];
    const int li = lane < MD ? lane : MD - 1;               // lane 15 shadows row 14 and never writes
#pragma unroll
    for (int j = 0; j < MD; ++j) row[j] = j <= li ? H[li * LS + j] + (j == li ? lambda : 0.0) : 0.0;      // (the entries right of the diagonal are never used)
    int bad = 0;
#pragma unroll
    for (int j = 0; j < MD; ++j) {
        double sacc = row[j];
#pragma unroll
        for (int k = 0; k < MD; ++k) if (k < j) sacc -= row[k] * L[LIDX(j, k)];
        const double dj = __shfl(sacc, j, LG);              // pivot before the square root, from the diagonal lane
        if (!(dj > 0) || !isfinite(dj)) { bad = 1; break; }
        const double dq = sqrt(dj);
        row[j] = li == j ? dq : sacc / dq;
        if (lane < MD && li >= j) L[LIDX(li, j)] = row[j];
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_sched_barrier(0);
    }
    return bad;
}
// b <- (L L^T)^-1 b, b in registers of every lane (same values on every lane of the group), L read from LDS
__device__ static void chol15_solve(const double* L, double* b)
{
#pragma unroll
    for (int i = 0; i < MD; ++i) {
        double sacc = b[i];
#pragma unroll
        for (int k = 0; k < MD; ++k) if (k < i) sacc -= L[LIDX(i, k)] * b[k];
        b[i] = sacc / L[LIDX(i, i)];
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int i = MD - 1; i >= 0; --i) {
        double sacc = b[i];
#pragma unroll
        for (int k = 0; k < MD; ++k) if (k > i) sacc -= L[LIDX(k, i)] * b[k];
        b[i] = sacc / L[LIDX(i, i)];
        __builtin_amdgcn_sched_barrier(0);
    }
}

// ------------------------------------------------------------------ what lc_kernel and tri_kernel share
// the pi-yaw compensation of one side (optimizer.cpp:650,697-703) from its flag bit; rebuilt where needed, not kept in registers across an LM
__device__ inline void lc_comp_pose(bool on, pose_t* C)
{
    const double flipv[3] = { 0, 0, DSSS_PI_REF };
    pose_identity(C); if (on) so3_exp(flipv, C->R);
}
// sigmas of an SssPointFactor (:685): sigma_r = 0.1, slant * alpha_bw with alpha_bw = 0.1 degrees
__device__ inline void lc_sss_sigmas(double slant, double* sig) { sig[0] = 0.1; sig[1] = slant * (0.1 * DSSS_PI_REF / 180); }
// landmark start (:789-795): midpoint of the two geo samples, mean of the two pings' depths below their altitudes
__device__ inline void lc_landmark_start(const double* geo_s, const double* geo_t, double z_s, double alt_s, double z_t, double alt_t, double* L)
{
    L[0] = (geo_s[0] + geo_t[0]) / 2; L[1] = (geo_s[1] + geo_t[1]) / 2; L[2] = ((z_s - alt_s) + (z_t - alt_t)) / 2;
}

// ------------------------------------------------------------------ lc_kernel, stage by stage (each inlined into the kernel)
// the context's per-frame device tables, indexed by frame slot
struct lc_tables { const double* const* __restrict__ alt; const double* const* __restrict__ gr; const double* const* __restrict__ pose; const int* __restrict__ cols; };
static lc_tables lc_tables_of(const dsss_ctx* c) { const int F = c->max_frames; return { c->d_ptrs, c->d_ptrs + F, c->d_ptrs + 2 * F, c->cols_dev }; }

// set-up (:685-795): DR poses with the compensation, sigmas and the landmark start into LDS (S.m, S.v); geo[4]: the two points' geo samples
__device__ inline void lc_setup(lc_lds& S, const lc_tables& T, const double* kp, int fs, int ft, int flip, int lane, double* geo)
{
    const double PI = DSSS_PI_REF;
    const double* pose_s = T.pose[fs]; const double* pose_t_ = T.pose[ft];
    const int id_s = (int)kp[0], id_t = (int)kp[3];
    const bool hb = (lane & 8) != 0;                       // lanes 0..7: the source ping's pose and geo sample, lanes 8..15: the target's
    mini_prob m;                                            // built in registers
    m.slant_s = kp[2]; m.slant_t = kp[5]; lc_sss_sigmas(kp[2], m.sig_s); lc_sss_sigmas(kp[5], m.sig_t);
    pose_t Tp_s, Tp_t, Tp_st;
    {
        pose_t Pm, Cm, Tm;
        pose_from_rodrigues(hb ? pose_t_ + (size_t)id_t * 6 : pose_s + (size_t)id_s * 6, &Pm);
        lc_comp_pose(flip & (hb ? 2 : 1), &Cm);
        pose_compose(&Pm, &Cm, &Tm);
        lc_bcast_pose(Tm, 0, &Tp_s); lc_bcast_pose(Tm, 8, &Tp_t);
    }
    pose_between(&Tp_s, &Tp_t, &Tp_st);
    for (int k = 0; k < 6; ++k) m.sig_prior[k] = 0.000001;
    m.sig_odo[0] = 0.1 * PI / 180; m.sig_odo[1] = 0.1 * PI / 180; m.sig_odo[2] = 0.5 * PI / 180;          // :778
    m.sig_odo[3] = fabs(Tp_st.t[0] * 2); m.sig_odo[4] = fabs(Tp_st.t[1] / 10); m.sig_odo[5] = 0.1;
    for (int k = 3; k < 5; ++k) if (m.sig_odo[k] < 1e-9) m.sig_odo[k] = 1e-9;
    m.prior = Tp_s; m.odo = Tp_st;
    double gx, gy;
    dsss_geo_at(hb ? pose_t_ : pose_s, hb ? T.gr[ft] : T.gr[fs], hb ? T.cols[ft] : T.cols[fs], hb ? id_t : id_s, hb ? (int)kp[4] : (int)kp[1], &gx, &gy);
    geo[0] = __shfl(gx, 0, LG); geo[1] = __shfl(gy, 0, LG); geo[2] = __shfl(gx, 8, LG); geo[3] = __shfl(gy, 8, LG);
    mini_val v;
    lc_landmark_start(geo, geo + 2, pose_s[(size_t)id_s * 6 + 5], T.alt[fs][id_s], pose_t_[(size_t)id_t * 6 + 5], T.alt[ft][id_t], v.L);
    v.X1 = Tp_s; v.X2 = Tp_t;
    if (lane == 0) { S.m = m; S.v = v; }
    __builtin_amdgcn_wave_barrier();                        // the group's lanes sit in one wavefront: its LDS operations execute in program order
}
// one trial: solve (H + lambda I) d = -g, linear error at d, retraction into S.nv, error there.  Failed Cholesky, rising linear model: refused, no stop
__device__ inline lm_verdict lc_trial(lc_lds& S, const lm_rule& R, double g_mine, double lambda, double oldLin, double err, int lane, double* newErr)
{
    const lm_verdict refused = { false, false };
    if (chol15(S.H, lambda, S.H, lane) != 0) return refused;
    double d[MD];
#pragma unroll
    for (int a = 0; a < MD; ++a) d[a] = -__shfl(g_mine, a, LG);
    chol15_solve(S.H, d);
    double sk = S.r[lane];                                  // lane k: row k of J d + r
#pragma unroll
    for (int a = 0; a < MD; ++a) sk += S.J[lane * LS + a] * d[a];
    double newLin = 0;
#pragma unroll
    for (int k = 0; k < MR; ++k) { const double t = __shfl(sk, k, LG); newLin += t * t; }
    newLin *= 0.5;
    if (!lm_descends(oldLin, newLin)) return refused;
    {   // the trial values go to LDS (S.nv); the registers that held them are free again afterwards
        const bool hb = (lane & 8) != 0;                    // lanes 0..7 retract X1, lanes 8..15 X2
        pose_t Xn; double dx[6];
        const pose_t* X = hb ? &S.v.X2 : &S.v.X1;
#pragma unroll
        for (int a = 0; a < 6; ++a) dx[a] = hb ? d[9 + a] : d[3 + a];
        pose_retract(X, dx, &Xn);
        if (lane == 0) { for (int a = 0; a < 3; ++a) S.nv.L[a] = S.v.L[a] + d[a]; S.nv.X1 = Xn; }
        if (lane == 8) S.nv.X2 = Xn;
        __builtin_amdgcn_wave_barrier();
    }
    *newErr = mini_err(S.m, S.nv, lane);
    return lm_judge(R, oldLin, newLin, err, *newErr);
}
// v = nv, element-wise by the lanes of the group (27 doubles)
__device__ inline void lc_take_trial(lc_lds& S, int lane)
{
    const double* src = reinterpret_cast<const double*>(&S.nv); double* dst = reinterpret_cast<double*>(&S.v);
    const double e0 = src[lane], e1 = lane + LG < (int)(sizeof(mini_val) / sizeof(double)) ? src[lane + LG] : 0.0;
    __builtin_amdgcn_wave_barrier();
    dst[lane] = e0; if (lane + LG < (int)(sizeof(mini_val) / sizeof(double))) dst[lane + LG] = e1;
    __builtin_amdgcn_wave_barrier();
}
// LevenbergMarquardtOptimizer::optimize, default params (:815-822), on S.v; *err_io: the error at S.v; returns the accepted steps
__device__ inline int lc_lm(lc_lds& S, int lane, double* err_io)
{
    const lm_rule R = lm_gtsam_defaults();
    double lambda = 1e-5, err = *err_io, cur;
    int iters = 0;
    if (err > 0) do {
        cur = err;
        mini_lin(S.m, S.v, S.r, S.J, lane);
        const double g_mine = normal_eq(S.J, S.r, S.H, lane);
        double oldLin = 0;
#pragma unroll
        for (int k = 0; k < MR; ++k) oldLin += S.r[k] * S.r[k];
        oldLin *= 0.5;
        for (;;) {
            double newErr = 0;
            const lm_verdict v = lc_trial(S, R, g_mine, lambda, oldLin, err, lane, &newErr);
            if (v.success) { lc_take_trial(S, lane); err = newErr; lm_accepted(R, &lambda); ++iters; break; }
            if (v.stop || lm_refused(R, &lambda)) break;
        }
    } while (lm_continue(R, iters, cur, err));
    *err_io = err; return iters;
}
// eval_1 (:853-896): *new_pose = X2 without its compensation; score = ini / final - 2, the source sample's distance to the target's before and after
__device__ inline double lc_score(const lc_lds& S, const double* kp, const double* gr_t, int Mt, int flip, const double* geo, pose_t* new_pose)
{
    const double PI = DSSS_PI_REF;
    pose_t cq, cti;
    lc_comp_pose(flip & 2, &cq); pose_inverse(&cq, &cti);
    pose_compose(&S.v.X2, &cti, new_pose);
    const double x_o = geo[0] - geo[2], y_o = geo[1] - geo[3], ini = sqrt(x_o * x_o + y_o * y_o);
    double rpy[3]; pose_rpy(new_pose, rpy);
    const bool port = kp[4] < Mt / 2;
    const int gi = port ? Mt / 2 - (int)kp[4] : (int)kp[4] - Mt / 2;
    const double bearing = port ? rpy[2] + PI / 2 - PI : rpy[2] - PI / 2 - PI;
    const double lx = new_pose->t[0] + gr_t[gi] * cos(bearing), ly = new_pose->t[1] + gr_t[gi] * sin(bearing);
    const double x_n = geo[0] - lx, y_n = geo[1] - ly;
    return ini / sqrt(x_n * x_n + y_n * y_n) - 2;
}
// Marginals(graph, result).marginalCovariance(X2).diagonal() (:956-959): lane c < 6 solves for unit vector 9 + c; NaN where H at S.v does not factor
__device__ inline void lc_marginal_var(lc_lds& S, int lane, double* var)
{
    mini_lin(S.m, S.v, S.r, S.J, lane);
    (void)normal_eq(S.J, S.r, S.H, lane);
    double var_mine = NAN;
    if (chol15(S.H, 0.0, S.H, lane) == 0) {
        double d[MD];
#pragma unroll
        for (int a = 0; a < MD; ++a) d[a] = (a == 9 + lane) ? 1.0 : 0.0;
        chol15_solve(S.H, d);
        var_mine = 0;
#pragma unroll
        for (int a = 9; a < MD; ++a) if (a == 9 + lane) var_mine = d[a];
    }
#pragma unroll
    for (int c2 = 0; c2 < 6; ++c2) var[c2] = __shfl(var_mine, c2, LG);
}
// the measurement (:958): new_pose relative to the source's DR pose without its compensation (S.m.prior = Tp_s)
__device__ inline void lc_rel_pose(const lc_lds& S, int flip, const pose_t& new_pose, double* rel12)
{
    pose_t cq, csi, src, rel;
    lc_comp_pose(flip & 1, &cq); pose_inverse(&cq, &csi);
    pose_compose(&S.m.prior, &csi, &src); pose_between(&src, &new_pose, &rel);
    for (int a = 0; a < 9; ++a) rel12[a] = rel.R[a];
    for (int a = 0; a < 3; ++a) rel12[9 + a] = rel.t[a];
}

// kp7: n x 7, kp7_flip: the sticky compensation flags of every row (bit 0 source, bit 1 target; made by the matcher or by lc_sticky_flags).
// The frames of row i: slots act_s / act_t[kp7_pair[i]], or single_s / single_t for every row when kp7_pair is null.
__global__ __launch_bounds__(64, 2) void lc_kernel(const double* __restrict__ kp7, int n, const int* __restrict__ kp7_pair, const uint8_t* __restrict__ kp7_flip,
                                                const int* __restrict__ act_s, const int* __restrict__ act_t, int single_s, int single_t, lc_tables T, dsss_lc* __restrict__ out)
{
    __shared__ lc_lds s_all[64 / LG];
    const int grp = threadIdx.x / LG, lane = threadIdx.x % LG;
    const int i = blockIdx.x * (64 / LG) + grp;
    if (i >= n) return;                                     // whole groups leave together
    lc_lds& S = s_all[grp];
    const double* kp = kp7 + (size_t)i * 7;
    const int fs = kp7_pair ? act_s[kp7_pair[i]] : single_s, ft = kp7_pair ? act_t[kp7_pair[i]] : single_t;
    const int flip = kp7_flip[i];
    double geo[4]; dsss_lc o;
    lc_setup(S, T, kp, fs, ft, flip, lane, geo);                              // :685-795
    o.pad_ = 0; o.err0 = o.err1 = mini_err(S.m, S.v, lane);
    o.iters = lc_lm(S, lane, &o.err1);                                        // :815-822
    pose_t new_pose;
    o.score = lc_score(S, kp, T.gr[ft], T.cols[ft], flip, geo, &new_pose);    // :853-896
    lc_marginal_var(S, lane, o.var);                                          // :956-959
    lc_rel_pose(S, flip, new_pose, o.rel);                                    // :958
    if (lane == 0) out[i] = o;
}

// ------------------------------------------------------------------ a21 / a23: landmark triangulation
// LMTriaFactor (LMtriangulatefactor.cpp:10-27: residual and 2x3 Jacobian = those of SssPointFactor with the pose held
// fixed) inside Optimizer::TriangulateOneLandmark (optimizer.cpp:984-1021): 3-DoF GTSAM LM on the landmark, point prior
// (10, 10, |xy baseline| / 100).  Call site :907-921 (eval_2): DR poses with the sticky yaw compensation, landmark
// initialised as in :789-795; the four consistency figures printed there are returned next to the point.
// One thread per problem: 7 x 3 Jacobian and a 3 x 3 system in registers; same operation order as oracle/orc_lc.c.
struct tri_frame { const double* pose; const double* alt; const double* gr; int M; };      // device tables of one frame (unused, null, in the explicit-poses form)
struct tri_prob { pose_t Tp_s, Tp_t; double slant_s, slant_t, sig_s[2], sig_t[2], sig_p[3], ini[3]; };

// set-up: poses and start point -- the caller's (q, a row of the n x 27 form) or the DR poses with the compensation -- and the sigmas
__device__ inline void tri_setup(tri_prob& P, const double* kp, const tri_frame& s, const tri_frame& t, int flip, const double* q)
{
    if (q) {                                                        // TriangulateOneLandmark with the caller's poses and start point
        for (int k = 0; k < 9; ++k) { P.Tp_s.R[k] = q[k]; P.Tp_t.R[k] = q[12 + k]; }
        for (int k = 0; k < 3; ++k) { P.Tp_s.t[k] = q[9 + k]; P.Tp_t.t[k] = q[21 + k]; P.ini[k] = q[24 + k]; }
    } else {
        const int id_s = (int)kp[0], id_t = (int)kp[3];
        pose_t cps_s, cps_t, Ps, Pt;
        lc_comp_pose(flip & 1, &cps_s); lc_comp_pose(flip & 2, &cps_t);
        pose_from_rodrigues(s.pose + (size_t)id_s * 6, &Ps); pose_from_rodrigues(t.pose + (size_t)id_t * 6, &Pt);
        pose_compose(&Ps, &cps_s, &P.Tp_s); pose_compose(&Pt, &cps_t, &P.Tp_t);
        double geo_s[2], geo_t[2];
        dsss_geo_at(s.pose, s.gr, s.M, id_s, (int)kp[1], &geo_s[0], &geo_s[1]);
        dsss_geo_at(t.pose, t.gr, t.M, id_t, (int)kp[4], &geo_t[0], &geo_t[1]);
        lc_landmark_start(geo_s, geo_t, s.pose[(size_t)id_s * 6 + 5], s.alt[id_s], t.pose[(size_t)id_t * 6 + 5], t.alt[id_t], P.ini);
    }
    P.slant_s = kp[2]; P.slant_t = kp[5]; lc_sss_sigmas(kp[2], P.sig_s); lc_sss_sigmas(kp[5], P.sig_t);
    const double dx = P.Tp_s.t[0] - P.Tp_t.t[0], dy = P.Tp_s.t[1] - P.Tp_t.t[1];
    P.sig_p[0] = 10.0; P.sig_p[1] = 10.0; P.sig_p[2] = sqrt(dx * dx + dy * dy) / 100;
    if (P.sig_p[2] < 1e-9) P.sig_p[2] = 1e-9;
}
__device__ static void tri_lin(const tri_prob& P, const double* p, double* r, double* J)
{
    double ee[2], H1[6], H2[12];
    sss_factor(p, &P.Tp_s, P.slant_s, 0.0, ee, J ? H1 : nullptr, H2);
    for (int i = 0; i < 2; ++i) { r[i] = ee[i] / P.sig_s[i]; if (J) for (int j = 0; j < 3; ++j) J[i * 3 + j] = H1[3 * i + j] / P.sig_s[i]; }
    sss_factor(p, &P.Tp_t, P.slant_t, 0.0, ee, J ? H1 : nullptr, H2);
    for (int i = 0; i < 2; ++i) { r[2 + i] = ee[i] / P.sig_t[i]; if (J) for (int j = 0; j < 3; ++j) J[(2 + i) * 3 + j] = H1[3 * i + j] / P.sig_t[i]; }
    for (int i = 0; i < 3; ++i) { r[4 + i] = (p[i] - P.ini[i]) / P.sig_p[i]; if (J) for (int j = 0; j < 3; ++j) J[(4 + i) * 3 + j] = (i == j) ? 1.0 / P.sig_p[i] : 0.0; }
}
__device__ static double tri_err(const tri_prob& P, const double* p)
{
    double rr[7], t = 0;
    tri_lin(P, p, rr, nullptr); for (int k = 0; k < 7; ++k) t += rr[k] * rr[k];
    return 0.5 * t;
}
__device__ static int tri_chol3(double* A)
{
    for (int j = 0; j < 3; ++j) {
        double d = A[j * 3 + j];
        for (int k = 0; k < j; ++k) d -= A[j * 3 + k] * A[j * 3 + k];
        if (!(d > 0) || !isfinite(d)) return -1;
        d = sqrt(d); A[j * 3 + j] = d;
        for (int i = j + 1; i < 3; ++i) { double t = A[i * 3 + j]; for (int k = 0; k < j; ++k) t -= A[i * 3 + k] * A[j * 3 + k]; A[i * 3 + j] = t / d; }
    }
    return 0;
}
// the 3-DoF LM on the landmark p (optimizer.cpp:1003-1010), GTSAM defaults
__device__ inline void tri_lm(const tri_prob& P, double* p)
{
    const lm_rule R = lm_gtsam_defaults();
    double lambda = 1e-5, err = tri_err(P, p), cur;
    int iters = 0;
    if (err > 0) do {
        cur = err;
        double r[7], J[21], H[9], g[3];
        tri_lin(P, p, r, J);
        for (int a = 0; a < 3; ++a) {
            double t = 0; for (int k = 0; k < 7; ++k) t += J[k * 3 + a] * r[k];
            g[a] = t;
            for (int b = 0; b < 3; ++b) { double u = 0; for (int k = 0; k < 7; ++k) u += J[k * 3 + a] * J[k * 3 + b]; H[a * 3 + b] = u; }
        }
        double oldLin = 0; for (int k = 0; k < 7; ++k) oldLin += r[k] * r[k];
        oldLin *= 0.5;
        for (;;) {                                                  // one trial per pass; a failed Cholesky and a rising linear model are refused, no stop
            double A[9], d[3], np_[3] = { 0, 0, 0 }, newErr = 0, newLin = 0;
            lm_verdict v = { false, false };
            for (int a = 0; a < 9; ++a) A[a] = H[a];
            for (int a = 0; a < 3; ++a) { A[a * 3 + a] += lambda; d[a] = -g[a]; }
            if (tri_chol3(A) == 0) {
                for (int a = 0; a < 3; ++a) { double t = d[a]; for (int k = 0; k < a; ++k) t -= A[a * 3 + k] * d[k]; d[a] = t / A[a * 3 + a]; }
                for (int a = 2; a >= 0; --a) { double t = d[a]; for (int k = a + 1; k < 3; ++k) t -= A[k * 3 + a] * d[k]; d[a] = t / A[a * 3 + a]; }
                for (int k = 0; k < 7; ++k) { double t = r[k]; for (int a = 0; a < 3; ++a) t += J[k * 3 + a] * d[a]; newLin += t * t; }
                newLin *= 0.5;
                if (lm_descends(oldLin, newLin)) {
                    for (int a = 0; a < 3; ++a) np_[a] = p[a] + d[a];
                    newErr = tri_err(P, np_);
                    v = lm_judge(R, oldLin, newLin, err, newErr);
                }
            }
            if (v.success) { for (int a = 0; a < 3; ++a) p[a] = np_[a]; err = newErr; lm_accepted(R, &lambda); ++iters; break; }
            if (v.stop || lm_refused(R, &lambda)) break;
        }
    } while (lm_continue(R, iters, cur, err));
}
// flips: the rows' sticky flags (lc_sticky_flags), null only with explicit27 (n x 27: the caller's poses and start points)
__global__ __launch_bounds__(64) void tri_kernel(const double* __restrict__ kp7, int n, const uint8_t* __restrict__ flips, tri_frame fs, tri_frame ft,
                                                 const double* __restrict__ explicit27, double* __restrict__ out7)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const double* kp = kp7 + (size_t)i * 7;
    tri_prob P;
    tri_setup(P, kp, fs, ft, flips ? flips[i] : 0, explicit27 ? explicit27 + (size_t)i * 27 : nullptr);      // :907-915, :789-795
    double p[3] = { P.ini[0], P.ini[1], P.ini[2] };
    tri_lm(P, p);                                                                                            // :984-1021
    double* o = out7 + (size_t)i * 7;                               // the point and the four consistency figures (:916-921)
    o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
    double e[2];
    sss_factor(p, &P.Tp_s, P.slant_s, 0.0, e, nullptr, nullptr); o[3] = fabs(e[0]); o[4] = fabs(e[1]);
    sss_factor(p, &P.Tp_t, P.slant_t, 0.0, e, nullptr, nullptr); o[5] = fabs(e[0]); o[6] = fabs(e[1]);
}

// ------------------------------------------------------------------ host side
// caller-supplied kp7 rows: pings and bins index altitude / ground-range tables on the device, so they are range-checked on the host first
// (GetKpsPairs never emits |bin - M/2| < 20, optimizer.cpp:602-609; bin - M/2 == M/2 is the one-past-the-end read).  pair < 0: no pair to name.
static int check_kp7_rows(dsss_ctx* c, const dsss_frame& fs, const dsss_frame& ft, const double* rows, int n, int pair)
{
    for (int i = 0; i < n; ++i) {
        const double* k = rows + (size_t)i * 7;
        if (k[0] >= 0 && k[0] < fs.N && k[3] >= 0 && k[3] < ft.N && k[1] >= 1 && k[1] < fs.M && k[4] >= 1 && k[4] < ft.M) continue;
        char who[32] = ""; if (pair >= 0) snprintf(who, sizeof who, "pair %d ", pair);
        DSSS_FAIL(c, DSSS_E_ARG, "%skp7 row %d: ping/bin outside the frames (%g,%g | %g,%g)", who, i, k[0], k[1], k[3], k[4]);
    }
    return DSSS_OK;
}
// sticky yaw compensation flags of ONE LoopClosingTFs call (optimizer.cpp:650,697-703): prefix OR over its n checked rows, bit 0 source, bit 1 target
static void lc_sticky_flags(const dsss_frame& fs, const dsss_frame& ft, const double* rows, int n, uint8_t* flip)
{
    uint8_t f = 0;
    for (int i = 0; i < n; ++i) {
        const double* k = rows + (size_t)i * 7;
        if (dsss_yaw_flips(fs.h_geo[(size_t)(int)k[0] * 6 + 2])) f |= 1;
        if (dsss_yaw_flips(ft.h_geo[(size_t)(int)k[3] * 6 + 2])) f |= 2;
        flip[i] = f;
    }
}
// dsss_lc_solve and dsss_triangulate before anything reaches the device: frames, host copy of the rows (kp7 may be a device pointer), range check, flags
static int lc_one_list(dsss_ctx* c, int id_s, int id_t, const double* kp7, int n, std::vector<double>* h, std::vector<uint8_t>* flip)
{
    if (id_s < 0 || id_s >= c->max_frames || id_t < 0 || id_t >= c->max_frames) DSSS_FAIL(c, DSSS_E_ARG, "frame id out of range");
    const dsss_frame &fs = c->frames[id_s], &ft = c->frames[id_t];
    if (!fs.has_geom || !ft.has_geom) DSSS_FAIL(c, DSSS_E_STATE, "frames need dsss_frame_set first");
    if (!fs.h_geo || !ft.h_geo) DSSS_FAIL(c, DSSS_E_STATE, "host copy of the DR poses missing");
    if (n == 0) return DSSS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    h->resize((size_t)n * 7); flip->resize(n);
    HIPCHK(c, hipMemcpy(h->data(), kp7, h->size() * sizeof(double), hipMemcpyDefault));
    if (const int rc = check_kp7_rows(c, fs, ft, h->data(), n, -1)) return rc;
    lc_sticky_flags(fs, ft, h->data(), n, flip->data());
    return DSSS_OK;
}
// queues lc_kernel over n > 0 rows on the context's stream; the pointer tables are up (dsss_mt_upload_ptr_tables)
static int lc_launch(dsss_ctx* c, const double* kp7, int n, const int* kp7_pair, const uint8_t* kp7_flip, const int* act_s, const int* act_t, int single_s, int single_t,
                     dsss_lc* out)
{
    dsss_scope sc(c, DSSS_K_LC);
    hipLaunchKernelGGL(lc_kernel, dim3((n + 3) / 4), dim3(64), 0, c->stream, kp7, n, kp7_pair, kp7_flip, act_s, act_t, single_s, single_t, lc_tables_of(c), out);
    HIPCHK(c, hipGetLastError());
    return DSSS_OK;
}
// the two triangulation calls: rows and flags (or explicit poses) up into ONE buffer of this call, freed on every way out; tri_kernel; results down
static int tri_run(dsss_ctx* c, const double* kp7, int n, const uint8_t* h_flip, const tri_frame& fs, const tri_frame& ft, const double* in27, double* out7)
{
    const size_t nd = (size_t)n * (7 + 7 + (in27 ? 27 : 0));
    dsss_buf d("triangulation rows, inputs and results");
    if (const int rc = d.reserve(c, nd * sizeof(double) + (h_flip ? (size_t)n : 0))) return rc;
    double* d_kp7 = d.as<double>(); double* d_out = d_kp7 + (size_t)n * 7; double* d_in = in27 ? d_out + (size_t)n * 7 : nullptr;
    uint8_t* d_flip = h_flip ? reinterpret_cast<uint8_t*>(d_kp7 + nd) : nullptr;
    HIPCHK(c, hipMemcpyAsync(d_kp7, kp7, (size_t)n * 7 * sizeof(double), hipMemcpyDefault, c->stream));
    if (d_in) HIPCHK(c, hipMemcpyAsync(d_in, in27, (size_t)n * 27 * sizeof(double), hipMemcpyDefault, c->stream));
    if (d_flip) HIPCHK(c, hipMemcpyAsync(d_flip, h_flip, (size_t)n, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(tri_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, (const double*)d_kp7, n, (const uint8_t*)d_flip, fs, ft, (const double*)d_in, d_out);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out7, d_out, (size_t)n * 7 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DSSS_OK;
}
static tri_frame tri_frame_of(const dsss_frame& f) { return { f.pose6, f.alt, f.gr, f.M }; }

extern "C" {

int dsss_lc_solve_all(dsss_ctx* c)
{
    if (!c) return DSSS_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const int n = c->total_kp7;
    c->has_lc = false;
    if (const int rc = c->lcs.reserve(c, (size_t)n * sizeof(dsss_lc), ((size_t)n + 1024) * sizeof(dsss_lc))) return rc;
    if (n > 0)
        if (const int rc = lc_launch(c, c->kp7, n, c->kp7_pair, c->kp7_flip, c->act_s, c->act_t, 0, 0, c->lcs.as<dsss_lc>())) return rc;
    c->has_lc = true; ++c->lc_gen;      // an LC result set exists once its launch is queued (none for an empty one)
    return DSSS_OK;
}

int dsss_lc_get(dsss_ctx* c, int pair, dsss_lc* out, int cap, int* nout)
{
    if (!c) return DSSS_E_ARG;
    if (pair < 0 || pair >= c->npairs) DSSS_FAIL(c, DSSS_E_ARG, "pair %d out of range", pair);
    if (!c->has_lc) DSSS_FAIL(c, DSSS_E_STATE, "dsss_lc_solve_all has not run");
    const int a = c->pair_active[pair];
    const int n = a < 0 ? 0 : c->h_kp7_off[a + 1] - c->h_kp7_off[a];
    if (nout) *nout = n;
    if (n == 0 || !out) return DSSS_OK;
    if (cap < n) DSSS_FAIL(c, DSSS_E_CAPACITY, "caller capacity %d < %d", cap, n);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->lcs.as<dsss_lc>() + c->h_kp7_off[a], (size_t)n * sizeof(dsss_lc), hipMemcpyDeviceToHost));
    return DSSS_OK;
}

// LoopClosingTFs for the kp7 lists of MANY pairs given by the caller (what the host mirror's TrajOptimizationAll builds
// with GetKpsPairs from corres_kps or, with USE_ANNO = 1, from anno_kps: optimizer.cpp:35-97): one upload, one launch.
// The results stay on the device exactly as after dsss_match_pairs + dsss_lc_solve_all, so dsss_lc_get,
// dsss_posegraph_select and dsss_posegraph_solve work on them (pair order = the caller's order = the reference's loop order).
int dsss_lc_solve_pairs(dsss_ctx* c, const int* src_ids, const int* tgt_ids, int npairs, const double* kp7, const int* pair_off)
{
    if (!c || npairs < 0 || (npairs > 0 && (!src_ids || !tgt_ids || !pair_off))) return DSSS_E_ARG;
    dsss_mt_clear_results(c);            // whatever fails from here on leaves an EMPTY result set (include/dsss.h)
    HIPCHK(c, hipSetDevice(c->device));
    const int n = npairs > 0 ? pair_off[npairs] : 0;
    if (n < 0 || (n > 0 && !kp7)) return DSSS_E_ARG;
    for (int p = 0; p < npairs; ++p) {
        const int s = src_ids[p], t = tgt_ids[p];
        if (s < 0 || s >= c->max_frames || t < 0 || t >= c->max_frames || s == t) DSSS_FAIL(c, DSSS_E_ARG, "pair %d: bad frame ids (%d,%d)", p, s, t);
        if (!c->frames[s].has_geom || !c->frames[t].has_geom) DSSS_FAIL(c, DSSS_E_STATE, "pair %d: frames need dsss_frame_set first", p);
        if (pair_off[p + 1] < pair_off[p] || pair_off[0] != 0) DSSS_FAIL(c, DSSS_E_ARG, "pair_off does not start at 0 or is not ascending at pair %d", p);
    }
    int rc = dsss_sync_bboxes(c); if (rc) return rc;
    if ((rc = dsss_mt_upload_ptr_tables(c))) return rc;
    std::vector<double> h((size_t)n * 7);
    if (n > 0) HIPCHK(c, hipMemcpy(h.data(), kp7, h.size() * sizeof(double), hipMemcpyDefault));
    std::vector<int> h_pair(n); std::vector<uint8_t> h_flip(n);
    for (int p = 0; p < npairs && n > 0; ++p) {                    // the flags are sticky within one LoopClosingTFs call: per pair
        const dsss_frame &fs = c->frames[src_ids[p]], &ft = c->frames[tgt_ids[p]];
        const int o = pair_off[p], np = pair_off[p + 1] - o;
        if (!fs.h_geo || !ft.h_geo) DSSS_FAIL(c, DSSS_E_STATE, "pair %d: host copy of the DR poses missing", p);
        if ((rc = check_kp7_rows(c, fs, ft, h.data() + (size_t)o * 7, np, p))) return rc;
        lc_sticky_flags(fs, ft, h.data() + (size_t)o * 7, np, h_flip.data() + o);
        std::fill(h_pair.begin() + o, h_pair.begin() + o + np, p);
    }
    if (n > 0) {
        HIPCHK(c, hipStreamSynchronize(c->stream));                // queued kernels may still read the buffers written below
        if ((rc = dsss_mt_reserve_pair_index(c, npairs)) || (rc = dsss_mt_reserve_rows(c, n))) return rc;      // (no correspondences: the matcher's own per-pair buffers are not touched)
        HIPCHK(c, hipMemcpy(c->act_s, src_ids, npairs * sizeof(int), hipMemcpyHostToDevice)); HIPCHK(c, hipMemcpy(c->act_t, tgt_ids, npairs * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->kp7_off, pair_off, (npairs + 1) * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->kp7, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->kp7_pair, h_pair.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice)); HIPCHK(c, hipMemcpy(c->kp7_flip, h_flip.data(), (size_t)n, hipMemcpyHostToDevice));
    }
    // publish: every listed pair is "active", in the caller's order, with no matcher rows and no correspondences (corres_valid stays false)
    c->npairs = c->nactive = npairs; c->total_kp7 = n;
    c->pair_s.assign(src_ids, src_ids + npairs); c->pair_t.assign(tgt_ids, tgt_ids + npairs);
    c->pair_active.resize(npairs); for (int p = 0; p < npairs; ++p) c->pair_active[p] = p;
    c->h_row_off.assign(npairs + 1, 0); if (npairs > 0) c->h_kp7_off.assign(pair_off, pair_off + npairs + 1);
    return dsss_lc_solve_all(c);
}

int dsss_lc_solve(dsss_ctx* c, int id_s, int id_t, const double* kp7, int n, dsss_lc* out)
{
    if (!c || n < 0 || (n > 0 && (!kp7 || !out))) return DSSS_E_ARG;
    std::vector<double> h; std::vector<uint8_t> flip;
    int rc = lc_one_list(c, id_s, id_t, kp7, n, &h, &flip); if (rc || n == 0) return rc;
    if ((rc = dsss_sync_bboxes(c))) return rc;                 // also publishes the frames' N and M to the device tables
    if ((rc = dsss_mt_upload_ptr_tables(c))) return rc;
    dsss_buf d_kp7("dsss_lc_solve kp7"), d_flip("dsss_lc_solve flags"), d_out("dsss_lc_solve results");      // of this call: freed on every way out of it
    if ((rc = d_kp7.reserve(c, h.size() * sizeof(double))) || (rc = d_flip.reserve(c, flip.size())) || (rc = d_out.reserve(c, (size_t)n * sizeof(dsss_lc)))) return rc;
    HIPCHK(c, hipMemcpyAsync(d_kp7.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_flip.p, flip.data(), flip.size(), hipMemcpyHostToDevice, c->stream));
    if ((rc = lc_launch(c, d_kp7.as<double>(), n, nullptr, d_flip.as<uint8_t>(), nullptr, nullptr, id_s, id_t, d_out.as<dsss_lc>()))) return rc;
    HIPCHK(c, hipMemcpyAsync(out, d_out.p, (size_t)n * sizeof(dsss_lc), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DSSS_OK;
}

// Optimizer::TriangulateOneLandmark for every row of the caller's kp7 list of one pair (optimizer.h:56-59, call site
// optimizer.cpp:907-921).  out7_host: n x 7 = [x y z | |range_s err| |plane_s| |range_t err| |plane_t|].
int dsss_triangulate(dsss_ctx* c, int id_s, int id_t, const double* kp7, int n, double* out7)
{
    if (!c || n < 0 || (n > 0 && (!kp7 || !out7))) return DSSS_E_ARG;
    std::vector<double> h; std::vector<uint8_t> flip;
    const int rc = lc_one_list(c, id_s, id_t, kp7, n, &h, &flip); if (rc || n == 0) return rc;
    return tri_run(c, h.data(), n, flip.data(), tri_frame_of(c->frames[id_s]), tri_frame_of(c->frames[id_t]), nullptr, out7);
}

// the same with the caller's own poses: Optimizer::TriangulateOneLandmark(kps_pair, Ts_s, Ts_t, Tp_s, Tp_t, lm_ini) with
// Ts = identity (frame.cpp:38-39).  in27: n x [Tp_s R(9) t(3) | Tp_t R(9) t(3) | lm_ini(3)]; only kp7[2], kp7[5] (slant ranges) are read.
int dsss_triangulate_poses(dsss_ctx* c, const double* kp7, const double* in27, int n, double* out7)
{
    if (!c || n < 0 || (n > 0 && (!kp7 || !in27 || !out7))) return DSSS_E_ARG;
    if (n == 0) return DSSS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    return tri_run(c, kp7, n, nullptr, tri_frame{}, tri_frame{}, in27, out7);
}

} // extern "C"

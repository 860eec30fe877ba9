// diasss_amd/csrc/dsss_pg_report.hip -- what the factors of a pose graph say about a trajectory, and a solve that listens (no
// reference counterpart: TrajOptimizationAll hands every selected loop closure to the optimiser and never looks back, optimizer.cpp:203-258).
//     dsss_posegraph_edge_report   every factor of the graph dsss_posegraph_solve_edges builds, evaluated at ANY trajectory: per
//                                  loop closure the whitened residual and its chi-square, and the objective split into the chain's
//                                  share and the loop closures'
//     dsss_posegraph_solve_gated   solve, report, drop the worst decade of the inconsistent closures, solve again -- around the
//                                  UNCHANGED dsss_posegraph_solve_edges (the solver and its kernels are not touched by the gate)
// The factors are factor_eval's (dsss_pg_dev.h), the measurements pg_init_kernel's: the numbers here are the solve's own.
#include "dsss_pg_kernels.h"
#include "dsss_pg_dev.h"
#include <algorithm>
#include <limits>

// One thread per factor k < n + ne (k < n: prior / odometry, n + e: loop closure e), as pg_linearize_kernel<false>: a gather of two 96-byte
// poses and ~400 dependent f64 operations per thread, the residual in registers (factor_eval<false> writes no Jacobian).  The squared
// norms of a workgroup go through the fixed tree of block_sum256 into TWO partials per workgroup -- chain factors and loop closures
// apart -- which pg_final_sum_kernel adds in block order: no atomics, the same bits every call.
__global__ __launch_bounds__(256) void pg_report_kernel(int n, int ne, const pose_t* __restrict__ X, const pose_t* __restrict__ meas, pg_weights W,
                                                        const int* __restrict__ ea, const int* __restrict__ eb, const pose_t* __restrict__ emeas,
                                                        const double* __restrict__ ew, double* __restrict__ r6, double* __restrict__ chi2,
                                                        double* __restrict__ part_chain, double* __restrict__ part_lc)
{
    __shared__ double s_w[4];
    const int k = blockIdx.x * 256 + threadIdx.x;
    double e2 = 0;
    if (k < n + ne) {
        double rr[6], J[36];
        factor_eval<false>(k, n, X, meas, W, ea, eb, emeas, ew, rr, J);
#pragma unroll
        for (int a = 0; a < 6; ++a) e2 += rr[a] * rr[a];
        if (k >= n) {
            const size_t e = (size_t)(k - n);
#pragma unroll
            for (int a = 0; a < 6; ++a) r6[e * 6 + a] = rr[a];
            chi2[e] = e2;
        }
    }
    const double sc = block_sum256(k < n ? e2 : 0.0, s_w);
    const double sl = block_sum256(k < n ? 0.0 : e2, s_w);
    if (threadIdx.x == 0) { part_chain[blockIdx.x] = sc; part_lc[blockIdx.x] = sl; }
}

namespace {

// the checks of dsss_posegraph_solve_edges on one edge (pg_solve::plan, upload_dr)
int pgr_check_edges(dsss_ctx* c, const dsss_lc_edge* edges, int ne, int n)
{
    for (int e = 0; e < ne; ++e) {
        const dsss_lc_edge& E = edges[e];
        if (E.a < 0 || E.a >= n || E.b < 0 || E.b >= n || E.a == E.b) DSSS_FAIL(c, DSSS_E_ARG, "LC edge %d out of range", e);
        for (int k = 0; k < 6; ++k) if (!(E.var[k] > 0) || !std::isfinite(E.var[k])) DSSS_FAIL(c, DSSS_E_ARG, "LC edge %d: variance %d is not finite and positive", e, k);
        for (int k = 0; k < 12; ++k) if (!std::isfinite(E.rel[k])) DSSS_FAIL(c, DSSS_E_ARG, "LC edge %d: relative pose is not finite", e);
    }
    return DSSS_OK;
}

// the report proper.  dr6 and poses12: host or device; edges: HOST, already checked.
int pgr_run(dsss_ctx* c, const double* dr6, int n, const dsss_lc_edge* edges, int ne, const double* poses12,
            double* chi2_host, double* r6_host, double* sums3_host)
{
    const hipStream_t st = c->stream;
    const int nf = n + ne, nblk = (nf + 255) / 256;
    // device layout: X | DR poses (pg_init_kernel's second output, not read) | meas | emeas | dr6 | ew | r6 | chi2 | partials | sums | ea | eb
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_X = 0, o_D = o_X + up((size_t)n * sizeof(pose_t)), o_M = o_D + up((size_t)n * sizeof(pose_t)),
                 o_EM = o_M + up((size_t)n * sizeof(pose_t)), o_dr = o_EM + up((size_t)ne * sizeof(pose_t)),
                 o_ew = o_dr + up((size_t)n * 6 * sizeof(double)), o_r = o_ew + up((size_t)ne * 6 * sizeof(double)),
                 o_c = o_r + up((size_t)ne * 6 * sizeof(double)), o_p = o_c + up((size_t)ne * sizeof(double)),
                 o_s = o_p + up((size_t)2 * nblk * sizeof(double)), o_a = o_s + up(2 * sizeof(double)),
                 o_b = o_a + up((size_t)ne * sizeof(int)), total = o_b + up((size_t)ne * sizeof(int));
    if (const int rc = c->pgr_buf.reserve(c, total, total + total / 4)) return rc;      // the context keeps the report's device scratch between calls
    char* B = c->pgr_buf.as<char>();
    pose_t *d_X = (pose_t*)(B + o_X), *d_D = (pose_t*)(B + o_D), *d_M = (pose_t*)(B + o_M), *d_EM = (pose_t*)(B + o_EM);
    double *d_dr = (double*)(B + o_dr), *d_ew = (double*)(B + o_ew), *d_r = (double*)(B + o_r), *d_c = (double*)(B + o_c),
           *d_p = (double*)(B + o_p), *d_s = (double*)(B + o_s);
    int *d_a = (int*)(B + o_a), *d_b = (int*)(B + o_b);

    pg_weights W;                                                        // the solve's (pg_solve::plan; optimizer.cpp:24,28)
    { const double PI = DSSS_PI_REF, wgt1 = 0.001, wgt2 = 10;
      const double so[6] = { wgt1 * PI / 180, wgt1 * PI / 180, 0.1 * wgt1 * wgt2 * PI / 180, wgt1 * wgt2, wgt1 * wgt2, wgt1 };
      for (int k = 0; k < 6; ++k) { W.prior[k] = 1.0 / 0.000001; W.odo[k] = 1.0 / so[k]; } }
    std::vector<int> ea(ne), eb(ne); std::vector<pose_t> emeas(ne); std::vector<double> ew((size_t)ne * 6);
    for (int e = 0; e < ne; ++e) {
        ea[e] = edges[e].a; eb[e] = edges[e].b;
        for (int k = 0; k < 9; ++k) emeas[e].R[k] = edges[e].rel[k];
        for (int k = 0; k < 3; ++k) emeas[e].t[k] = edges[e].rel[9 + k];
        for (int k = 0; k < 6; ++k) ew[(size_t)e * 6 + k] = 1.0 / std::sqrt(edges[e].var[k]);
    }
    HIPCHK(c, hipMemcpyAsync(d_dr, dr6, (size_t)n * 6 * sizeof(double), hipMemcpyDefault, st));
    HIPCHK(c, hipMemcpyAsync(d_X, poses12, (size_t)n * sizeof(pose_t), hipMemcpyDefault, st));      // pose_t is 12 contiguous doubles (R row-major, t)
    if (ne) {
        HIPCHK(c, hipMemcpyAsync(d_a, ea.data(), (size_t)ne * sizeof(int), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(d_b, eb.data(), (size_t)ne * sizeof(int), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(d_EM, emeas.data(), (size_t)ne * sizeof(pose_t), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(d_ew, ew.data(), (size_t)ne * 6 * sizeof(double), hipMemcpyHostToDevice, st));
    }
    hipLaunchKernelGGL(pg_init_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, d_dr, (const double*)nullptr, 0, d_D, d_M);
    hipLaunchKernelGGL(pg_report_kernel, dim3(nblk), dim3(256), 0, st, n, ne, d_X, d_M, W, d_a, d_b, d_EM, d_ew, d_r, d_c, d_p, d_p + nblk);
    hipLaunchKernelGGL(pg_final_sum_kernel, dim3(1), dim3(256), 0, st, d_p, nblk, 0.5, d_s);
    hipLaunchKernelGGL(pg_final_sum_kernel, dim3(1), dim3(256), 0, st, d_p + nblk, nblk, 0.5, d_s + 1);
    HIPCHK(c, hipGetLastError());
    double s2[2] = { 0, 0 };
    if (ne && chi2_host) HIPCHK(c, hipMemcpyAsync(chi2_host, d_c, (size_t)ne * sizeof(double), hipMemcpyDeviceToHost, st));
    if (ne && r6_host) HIPCHK(c, hipMemcpyAsync(r6_host, d_r, (size_t)ne * 6 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(s2, d_s, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));      // (also: the host vectors above were read by the uploads)
    if (sums3_host) { sums3_host[0] = s2[0]; sums3_host[1] = s2[1]; sums3_host[2] = s2[0] + s2[1]; }
    return DSSS_OK;
}

} // namespace

extern "C" {

int dsss_posegraph_edge_report(dsss_ctx* c, const double* dr6, int total, const dsss_lc_edge* edges, int ne,
                               const double* poses12, double* chi2_host, double* r6_host, double* sums3_host)
{
    if (!c || !dr6 || !poses12 || total <= 0 || ne < 0 || (ne > 0 && (!edges || !chi2_host))) return DSSS_E_ARG;
    if ((long long)total + ne > std::numeric_limits<int>::max() - 256) return DSSS_E_ARG;
    if (dsss_comm_world(c) > 1) DSSS_FAIL(c, DSSS_E_STATE, "dsss_posegraph_edge_report is single rank");
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<dsss_lc_edge> h_e(ne);
    if (ne) HIPCHK(c, hipMemcpy(h_e.data(), edges, (size_t)ne * sizeof(dsss_lc_edge), hipMemcpyDefault));
    if (const int rc = pgr_check_edges(c, h_e.data(), ne, total)) return rc;
    return pgr_run(c, dr6, total, h_e.data(), ne, poses12, chi2_host, r6_host, sums3_host);
}

void dsss_pg_gate_params_default(dsss_pg_gate_params* p)
{
    if (!p) return;
    p->gate = 22.458;            // chi-square, 6 degrees of freedom, p = 0.999
    p->decade = 10.0; p->max_solves = 8; p->pad_ = 0;
}

// All edges start kept.  Solve the kept edges (compacted in their original order); report them at the result, m = their largest chi2
// (a non-finite one counts as +inf); m <= gate or the last allowed solve: done; otherwise every kept edge with chi2 > max(gate, m / decade)
// goes and the rest is solved again.  The worst decade first: an outlier inflates the residuals of the good edges around it, so
// they are judged only once it has gone.  No sorting, no ties to break: the same mask every run.
int dsss_posegraph_solve_gated(dsss_ctx* c, const double* dr6, int total, const dsss_lc_edge* edges, int ne,
                               const dsss_pg_gate_params* gp, double* poses12_host, double* stats4_host,
                               uint8_t* keep_host, double* chi2_host, int* n_solves_host)
{
    if (!c || !dr6 || total <= 0 || ne < 0 || (ne > 0 && (!edges || !keep_host)) || !poses12_host || !n_solves_host) return DSSS_E_ARG;
    dsss_pg_gate_params G;
    if (gp) G = *gp; else dsss_pg_gate_params_default(&G);
    if (!(G.gate > 0) || !(G.decade > 1) || G.max_solves < 1) DSSS_FAIL(c, DSSS_E_ARG, "gate must be > 0, decade > 1, max_solves >= 1");
    if (dsss_comm_world(c) > 1) DSSS_FAIL(c, DSSS_E_STATE, "dsss_posegraph_solve_gated is single rank");
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<double> h_dr((size_t)total * 6);
    HIPCHK(c, hipMemcpy(h_dr.data(), dr6, h_dr.size() * sizeof(double), hipMemcpyDefault));
    std::vector<dsss_lc_edge> h_e(ne);
    if (ne) HIPCHK(c, hipMemcpy(h_e.data(), edges, (size_t)ne * sizeof(dsss_lc_edge), hipMemcpyDefault));
    if (const int rc = pgr_check_edges(c, h_e.data(), ne, total)) return rc;
    std::vector<uint8_t> keep(ne, 1);
    std::vector<dsss_lc_edge> kept; kept.reserve(ne);
    std::vector<int> kidx; kidx.reserve(ne);
    std::vector<double> chi2(ne);
    const double INF = std::numeric_limits<double>::infinity();
    int solves = 0;
    for (;;) {
        kept.clear(); kidx.clear();
        for (int e = 0; e < ne; ++e) if (keep[e]) { kept.push_back(h_e[e]); kidx.push_back(e); }
        const int nk = (int)kept.size();
        if (const int rc = dsss_posegraph_solve_edges(c, h_dr.data(), total, kept.data(), nk, poses12_host, stats4_host)) return rc;
        ++solves;
        if (solves >= G.max_solves || nk == 0) break;
        if (const int rc = pgr_run(c, h_dr.data(), total, kept.data(), nk, poses12_host, chi2.data(), nullptr, nullptr)) return rc;
        double m = 0;
        for (int k = 0; k < nk; ++k) { if (!std::isfinite(chi2[k])) chi2[k] = INF; m = std::max(m, chi2[k]); }
        if (m <= G.gate) break;
        const double thr = std::max(G.gate, m / G.decade);
        int dropped = 0;
        for (int k = 0; k < nk; ++k) if (chi2[k] > thr) { keep[kidx[k]] = 0; ++dropped; }
        if (!dropped) break;      // (m = +inf only: the threshold is +inf too, and the same solve again would say the same)
    }
    if (ne) std::copy(keep.begin(), keep.end(), keep_host);
    *n_solves_host = solves;
    if (ne && chi2_host) return pgr_run(c, h_dr.data(), total, h_e.data(), ne, poses12_host, chi2_host, nullptr, nullptr);
    return DSSS_OK;
}

} // extern "C"

// diasss_amd/csrc/dsss_pg_dev.h -- device helpers the pose-graph kernels share: small dense algebra (6 x 6 row-major), the factors of the
// graph and the fixed block sum (one definition for the solve, dsss_pg_chain.hip, and the report, dsss_pg_report.hip)
#pragma once
#include <hip/hip_runtime.h>
#include "dsss_pg_kernels.h"
#include "dsss_wave.h"

// ------------------------------------------------------------------ small dense helpers (6x6 row-major)
// 6 x 6 Cholesky with the reciprocal of a correctly rounded square root (one sqrt and one division per pivot), ri[j] = 1 / L[j][j]: for the bins, whose 17 k columns
// carry the whole dynamic range of the chain condensation -- with rsqrt here two elimination orders of the C3 graph end 1.6e-6 apart, with
// this 3e-7 (test_config_C4_full_size_8_partitions_and_2_ranks)
__device__ inline int chol6_recip(double* A, double* ri)
{
    int bad = 0;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = A[j * 6 + j];
#pragma unroll
        for (int k = 0; k < 6; ++k) if (k < j) d -= A[j * 6 + k] * A[j * 6 + k];
        if (!(d > 0) || !isfinite(d)) { bad = 1; d = 1.0; }
        const double sq = sqrt(d), r = 1.0 / sq;
        A[j * 6 + j] = sq; ri[j] = r;
#pragma unroll
        for (int i = 0; i < 6; ++i) if (i > j) {
            double s = A[i * 6 + j];
#pragma unroll
            for (int k = 0; k < 6; ++k) if (k < j) s -= A[i * 6 + k] * A[j * 6 + k];
            A[i * 6 + j] = s * r;
        }
    }
    return bad;
}
// the same with 1 / L[j][j] left ON the diagonal (what the solves multiply by): no separate reciprocal array, twelve registers less
__device__ inline int chol6_rdiag(double* A)
{
    int bad = 0;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = A[j * 6 + j];
#pragma unroll
        for (int k = 0; k < 6; ++k) if (k < j) d -= A[j * 6 + k] * A[j * 6 + k];
        if (!(d > 0) || !isfinite(d)) { bad = 1; d = 1.0; }
        const double r = rsqrt(d);
        A[j * 6 + j] = r;
#pragma unroll
        for (int i = 0; i < 6; ++i) if (i > j) {
            double s = A[i * 6 + j];
#pragma unroll
            for (int k = 0; k < 6; ++k) if (k < j) s -= A[i * 6 + k] * A[j * 6 + k];
            A[i * 6 + j] = s * r;
        }
    }
    return bad;
}

// ------------------------------------------------------------------ factors
// factor k < n: k == 0 prior on X0 (measurement DR0), else Between(X_{k-1}, X_k); factor n + e: LC edge e.
// r = whitened residual, Ji = whitened Jacobian wrt the first pose (-W Ad(h^-1)); the Jacobian wrt the second
// pose is W itself (BetweenFactor with GTSAM_SLOW_BUT_CORRECT_BETWEENFACTOR off, PriorFactor H = I).
// WJ is a template parameter and the arrays are indexed by unrolled loops only: r and Ji stay in registers (with a run-time `Ji != nullptr` the
// compiler kept the 36 + 2 doubles in 304 bytes of private memory per thread -- 125 MB of scratch traffic per launch at C3, the reason the
// kernel wrote 243 MB for 138 MB of residuals and Jacobians).  Same operations in the same order: same bits.
template <bool WJ>
__device__ __forceinline__ void factor_eval(int k, int n, const pose_t* X, const pose_t* meas, const pg_weights& W,
                                            const int* ea, const int* eb, const pose_t* emeas, const double* ew,
                                            double (&r)[6], double (&Ji)[36])
{
    double xi[6];
    if (k == 0) {
        pose_t d;
        pose_between(&meas[0], &X[0], &d);
        pose_log(&d, xi);
#pragma unroll
        for (int a = 0; a < 6; ++a) r[a] = xi[a] * W.prior[a];
        if (WJ) {
#pragma unroll
            for (int a = 0; a < 36; ++a) Ji[a] = 0.0;
        }
        return;
    }
    int i, j; const pose_t* m; double w[6];
    if (k < n) {
        i = k - 1; j = k; m = &meas[k];
#pragma unroll
        for (int a = 0; a < 6; ++a) w[a] = W.odo[a];
    } else {
        const int e = k - n; i = ea[e]; j = eb[e]; m = &emeas[e];
#pragma unroll
        for (int a = 0; a < 6; ++a) w[a] = ew[(size_t)e * 6 + a];
    }
    pose_t h, er;
    pose_between(&X[i], &X[j], &h);
    pose_between(m, &h, &er);
    pose_log(&er, xi);
#pragma unroll
    for (int a = 0; a < 6; ++a) r[a] = xi[a] * w[a];
    if (WJ) {
        pose_t hi; double Ad[36];
        pose_inverse(&h, &hi);
        pose_adjoint(&hi, Ad);
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = 0; b < 6; ++b) Ji[a * 6 + b] = -Ad[a * 6 + b] * w[a];
    }
}

// deterministic block sum: wave shuffle tree then the 4 wave sums in order
__device__ inline double block_sum256(double v, double* s_w)
{
    v = dsss_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

// diasss_amd/csrc/dsss_pg_init.hip -- what the pose-graph solve needs around the chain and the factorisation: initial values (the noise of
// optimizer.cpp:150-160, DR poses, measurements), the ordered compaction of flagged items (accepted normal pairs, loop-closure edges),
// the gathers of DR rows and poses, the separators' coordinates and the trajectory rows (optimizer.cpp:1164-1214).  -ffp-contract=off.
#include "dsss_pg_kernels.h"
#include "dsss_pg_dev.h"

// ------------------------------------------------------------------ initial values on the device
// std::default_random_engine (minstd_rand0, seed 1) + std::normal_distribution<double> (libstdc++ Marsaglia polar,
// optimizer.cpp:30-31,154-158) without the sequential dependency: polar attempt a always consumes engine outputs
// 4a+1 .. 4a+4 (two generate_canonical calls of two engine calls each), so every attempt is evaluated independently
// after an O(log a) jump-ahead of the LCG; accepted attempts are compacted in order and each yields (y*mult, x*mult).
__device__ inline unsigned long long minstd_pow(unsigned long long e)
{
    unsigned long long r = 1, b = 16807ULL;
    const unsigned long long m = 2147483647ULL;
    while (e) { if (e & 1) r = (r * b) % m; b = (b * b) % m; e >>= 1; }
    return r;
}
__global__ __launch_bounds__(256) void pg_rng_attempts_kernel(long long nattempts, double* __restrict__ pairs, int* __restrict__ flags)
{
    const long long a0 = ((long long)blockIdx.x * 256 + threadIdx.x) * RNG_PER_THREAD;
    if (a0 >= nattempts) return;
    const unsigned long long m = 2147483647ULL;
    unsigned long long x = minstd_pow((unsigned long long)(4 * a0));        // state after 4*a0 engine calls (seed 1)
    const double R = 2147483646.0;
    for (int k = 0; k < RNG_PER_THREAD && a0 + k < nattempts; ++k) {
        double cn[2];
        for (int q = 0; q < 2; ++q) {
            x = (x * 16807ULL) % m; const double e1 = (double)(x - 1);
            x = (x * 16807ULL) % m; const double e2 = (double)(x - 1);
            double can = (e1 + e2 * R) / (R * R);
            if (can >= 1.0) can = 0.99999999999999988897769753748;   // nextafter(1, 0)
            cn[q] = can;
        }
        const double u = 2.0 * cn[0] - 1.0, v = 2.0 * cn[1] - 1.0, r2 = u * u + v * v;
        const bool ok = !(r2 > 1.0 || r2 == 0.0);
        double mult = 0;
        if (ok) mult = sqrt(-2 * log(r2) / r2);
        pairs[2 * (a0 + k)] = v * mult; pairs[2 * (a0 + k) + 1] = u * mult;
        flags[a0 + k] = ok ? 1 : 0;
    }
}
// exclusive scan of flags in three steps (block sums, scan of block sums by one block, compaction)
__global__ __launch_bounds__(256) void pg_flag_blocksum_kernel(const int* __restrict__ flags, long long n, int* __restrict__ bsum)
{
    __shared__ int s_w[4];
    const long long i0 = (long long)blockIdx.x * 4096;
    int acc = 0;
    for (int k = threadIdx.x; k < 4096; k += 256) if (i0 + k < n) acc += flags[i0 + k];
    acc = dsss_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) bsum[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}
__global__ __launch_bounds__(256) void pg_flag_scan_kernel(int* __restrict__ bsum, int nb, int* __restrict__ total)
{
    if (threadIdx.x == 0) { int run = 0; for (int i = 0; i < nb; ++i) { const int v = bsum[i]; bsum[i] = run; run += v; } *total = run; }
}
// the compaction of one block of 4096 flags, shared by the two kernels below: store(i, pos) for every set flag i, pos = its rank among
// the set flags of the whole list (bsum[] holds the ranks at the block starts).  The rank so far is carried in a register.
template <typename STORE>
__device__ inline void pg_compact_block(const int* __restrict__ flags, long long n, const int* __restrict__ bsum, STORE store)
{
    __shared__ int s_w[4];
    const long long i0 = (long long)blockIdx.x * 4096;
    int run = bsum[blockIdx.x];
    for (int c = 0; c < 4096; c += 256) {
        const long long i = i0 + c + threadIdx.x;
        const int f = (i < n) ? flags[i] : 0;
        int tot;
        const int pos = run + dsss_block_scan_excl<4, int>(f, &tot, s_w);
        if (f) store(i, pos);
        run += tot;
    }
}
__global__ __launch_bounds__(256) void pg_flag_compact_kernel(const int* __restrict__ flags, const double* __restrict__ pairs, long long n,
                                                              const int* __restrict__ bsum, long long need_pairs, double* __restrict__ normals)
{
    pg_compact_block(flags, n, bsum, [&](long long i, int pos) {
        if (pos < need_pairs) { normals[2 * (size_t)pos] = pairs[2 * i]; normals[2 * (size_t)pos + 1] = pairs[2 * i + 1]; }
    });
}
// edges in ascending target pose id (the reference's loop order), ordered compaction over blocks of 4096 poses
__global__ __launch_bounds__(256) void lc_edge_compact_kernel(const int* __restrict__ flags, const int* __restrict__ bsum, const unsigned long long* __restrict__ slot,
                                                              int total, const int* __restrict__ kp7_off, const double* __restrict__ kp7,
                                                              const dsss_lc* __restrict__ lcs, const int* __restrict__ act_s, const int* __restrict__ frame_off,
                                                              int cap, dsss_lc_edge* __restrict__ edges, int2* __restrict__ ab)
{
    pg_compact_block(flags, total, bsum, [&](long long g, int pos) {
        if (pos >= cap) return;
        const unsigned long long key = slot[g];
        const int p = (int)(key >> 32) - 1, k = (int)(0xffffffffu - (unsigned)(key & 0xffffffffu));
        const int i = kp7_off[p] + k;
        dsss_lc_edge ed;
        ed.a = frame_off[act_s[p]] + (int)kp7[(size_t)i * 7 + 0];
        ed.b = (int)g;
        for (int q = 0; q < 12; ++q) ed.rel[q] = lcs[i].rel[q];
        for (int q = 0; q < 6; ++q) ed.var[q] = lcs[i].var[q];
        edges[pos] = ed;
        if (ab) ab[pos] = make_int2(ed.a, ed.b);
    });
}
// DR rows of the frames (device copies kept by dsss_frame_set) into one array, frame after frame
__global__ __launch_bounds__(256) void pg_gather_dr_kernel(const unsigned long long* __restrict__ fptr, const int* __restrict__ foff, double* __restrict__ out)
{
    const int f = blockIdx.y;
    const double* __restrict__ src = reinterpret_cast<const double*>(fptr[f]);
    const size_t n6 = (size_t)(foff[f + 1] - foff[f]) * 6;
    double* __restrict__ dst = out + (size_t)foff[f] * 6;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n6; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}
// poses picked out of a trajectory by index (the frozen end points of a window update)
__global__ __launch_bounds__(256) void pg_gather_pose_kernel(int n, const int* __restrict__ idx, const pose_t* __restrict__ X, pose_t* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = X[idx[i]];
}
// x, y of the separator poses (the coordinates the nested dissection bisects)
__global__ __launch_bounds__(256) void pg_sep_xy_kernel(int ns, const int* __restrict__ sep_pose, const double* __restrict__ dr6, double* __restrict__ xy)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= ns) return;
    xy[2 * k] = dr6[(size_t)sep_pose[k] * 6 + 3]; xy[2 * k + 1] = dr6[(size_t)sep_pose[k] * 6 + 4];
}
// DR poses, odometry measurements and initial estimate (optimizer.cpp:150-200)
__global__ __launch_bounds__(256) void pg_init_kernel(int n, const double* __restrict__ dr6, const double* __restrict__ normals, int add_noise,
                                                      pose_t* __restrict__ X, pose_t* __restrict__ meas)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double PI = DSSS_PI_REF;
    pose_t cur, prev, m;
    pose_from_rodrigues(dr6 + (size_t)i * 6, &cur);
    if (i == 0) m = cur;
    else { pose_from_rodrigues(dr6 + (size_t)(i - 1) * 6, &prev); pose_between(&prev, &cur, &m); }
    meas[i] = m;
    if (add_noise) {
        const double* z = normals + (size_t)i * 6;
        const double noise_xyz = 0.5, noise_rpy = 0.5 * PI / 180;
        const double w[3] = { z[0] * noise_rpy, z[1] * noise_rpy, z[2] * noise_rpy };
        pose_t N, o;
        so3_exp(w, N.R);
        N.t[0] = z[3] * noise_xyz; N.t[1] = z[4] * noise_xyz; N.t[2] = z[5] * noise_xyz;
        pose_compose(&cur, &N, &o);
        X[i] = o;
    } else X[i] = cur;
}

// trajectory rows "r p y x y z" of SaveTrajactoryAll (optimizer.cpp:1199-1203), computed where the poses live
__global__ __launch_bounds__(256) void pg_rpy_kernel(int n, const pose_t* __restrict__ X, double* __restrict__ rpy6)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const pose_t T = X[i];
    double rpy[3];
    pose_rpy(&T, rpy);
    double* o = rpy6 + (size_t)i * 6;
    o[0] = rpy[0]; o[1] = rpy[1]; o[2] = rpy[2]; o[3] = T.t[0]; o[4] = T.t[1]; o[5] = T.t[2];
}


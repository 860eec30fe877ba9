// diasss_amd/csrc/dsss_pg_chain.hip -- the pose CHAIN of the batch LM (dsss_pg.hip): factors and their linearisation, per-pose Hessian
// blocks, the two-level condensation of the chain onto the separators and its back-substitution, the scatter of the reduced system into
// the factor / the fronts' value array, and what the ranks pack for the all-reduce.  (Initial values, the compactions and the
// trajectory rows: dsss_pg_init.hip.)  Everything here runs at -ffp-contract=off: the order of the source is the order of the result, and a
// sum that several kernels must form alike is ONE function below -- pg_jtj_row / pg_jtr (a factor's share of a pose's block row and
// gradient) and pg_condensed (a node's block and gradient after its two segments are condensed).
#include "dsss_pg_kernels.h"
#include "dsss_pg_dev.h"
// (the factors themselves -- factor_eval -- and the fixed block sum live in dsss_pg_dev.h: the report kernel of dsss_pg_report.hip evaluates the same ones)
// Ownership with several ranks (dsss_comm.hip): a rank owns the poses [mp0, mp1); chain factor k belongs to the owner of pose k,
// LC edge (a, b) to the owner of its HIGHER pose eo = max(a, b) -- the rule the analysis builds the interface on (dsss_pg_sym.cpp:
// "a factor belongs to the rank of its higher pose and adds to the diagonal block of the lower one").  The pipeline's own edges
// have a < b, so eo = b there; dsss_posegraph_solve_edges also takes a > b.  Every kernel below skips what the rank does not
// own; with one rank [mp0, mp1) is everything.  A SEGMENT of a level of the condensation (pg_level) belongs to the owner of its
// first interior node, in that level's indices.
__device__ __forceinline__ bool pg_owns(int p, int lo, int hi) { return p >= lo && p < hi; }
__device__ inline bool pg_owned_factor(int k, int n, const int* __restrict__ eo, int mp0, int mp1) { return pg_owns(k < n ? k : eo[k - n], mp0, mp1); }
__device__ __forceinline__ bool pg_owned_segment(const pg_level& lv, int s) { return pg_owns(lv.ends[s] + 1, lv.lo, lv.hi); }
template <bool WJ>        // WJ: residuals AND Jacobians (r, Ji both given); otherwise the error alone (r, Ji null)
__global__ __launch_bounds__(256) void pg_linearize_kernel(int n, int ne, const pose_t* __restrict__ X, const pose_t* __restrict__ meas,
                                                           pg_weights W, const int* __restrict__ ea, const int* __restrict__ eb, const int* __restrict__ eo,
                                                           const pose_t* __restrict__ emeas, const double* __restrict__ ew,
                                                           double* __restrict__ r, double* __restrict__ Ji, double* __restrict__ partial, int mp0, int mp1)
{
    __shared__ double s_w[4];
    // (round 4) A thread's 36 Jacobian entries are 288 contiguous bytes and the threads of a wavefront lie 288 bytes apart: stored
    // directly, every store instruction touched 64 cache lines for 8 bytes each.  The 64 Jacobians of a wavefront are ONE contiguous
    // 18 KB range: they go through the wavefront's own slice of LDS (half a Jacobian at a time, rows padded to 19) and leave as whole lines.
    __shared__ double s_j[4][64 * 19];
    const int k = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double e2 = 0;
    const bool own = k < n + ne && pg_owned_factor(k, n, eo, mp0, mp1);
    double rr[6], J[36];
    if (own) {
        factor_eval<WJ>(k, n, X, meas, W, ea, eb, emeas, ew, rr, J);
#pragma unroll
        for (int a = 0; a < 6; ++a) { e2 += rr[a] * rr[a]; if (WJ) r[(size_t)k * 6 + a] = rr[a]; }
    }
    if (WJ) {
        const unsigned long long owned = __ballot(own);
        const size_t k0 = (size_t)(blockIdx.x * 256 + wv * 64);   // first factor of this wavefront
        double* __restrict__ sj = s_j[wv];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (own) {
#pragma unroll
                for (int a = 0; a < 18; ++a) sj[lane * 19 + a] = J[18 * h + a];
            }
            __builtin_amdgcn_wave_barrier();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int i = 0; i < 18; ++i) {
                const int e = i * 64 + lane, f = e / 18, a = e - 18 * f;
                if ((owned >> f) & 1ull) Ji[(k0 + f) * 36 + 18 * h + a] = sj[f * 19 + a];
            }
            __builtin_amdgcn_wave_barrier();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
    }
    const double s = block_sum256(e2, s_w);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

template __global__ void pg_linearize_kernel<false>(int, int, const pose_t* __restrict__, const pose_t* __restrict__, pg_weights, const int* __restrict__, const int* __restrict__, const int* __restrict__, const pose_t* __restrict__, const double* __restrict__, double* __restrict__, double* __restrict__, double* __restrict__, int, int);
template __global__ void pg_linearize_kernel<true>(int, int, const pose_t* __restrict__, const pose_t* __restrict__, pg_weights, const int* __restrict__, const int* __restrict__, const int* __restrict__, const pose_t* __restrict__, const double* __restrict__, double* __restrict__, double* __restrict__, double* __restrict__, int, int);

__global__ __launch_bounds__(256) void pg_final_sum_kernel(const double* __restrict__ partial, int n, double scale, double* __restrict__ out)
{
    __shared__ double s_w[4];
    double acc = 0;
    for (int i = threadIdx.x; i < n; i += 256) acc += partial[i];
    const double s = block_sum256(acc, s_w);
    if (threadIdx.x == 0) *out = s * scale;
}

// A factor's share of the block row of its FIRST variable, from its Jacobian J (6 x 6 row-major): ja = column a of J, sb = row a of
// J^T J, every entry summed over q ascending; then (J^T r)[a].  pg_assemble_kernel (ends of the level-1 chain, loop closures) and
// pg_seg_from_j (interior poses) form the blocks of the pose chain with these, so they are the same sums in the same order.
__device__ __forceinline__ void pg_jtj_row(const double* J, int a, double* ja, double* sb)
{
#pragma unroll
    for (int q = 0; q < 6; ++q) ja[q] = J[q * 6 + a];
#pragma unroll
    for (int q = 0; q < 6; ++q)
#pragma unroll
        for (int b = 0; b < 6; ++b) sb[b] += ja[q] * J[q * 6 + b];
}
__device__ __forceinline__ double pg_jtr(const double* ja, const double* rr)
{
    double s = 0;
#pragma unroll
    for (int q = 0; q < 6; ++q) s += ja[q] * rr[q];
    return s;
}
// per-pose Hessian blocks: D (diagonal), C = H(i, i+1), g = J^T r, of the np poses of `plist` -- the ends of the level-1 chain, whose
// D, C, g the chain kernels read; the interior poses of the segments carry chain factors alone, and pg_segment_kernel<true> /
// pg_backsub_kernel<true> form their blocks from the Jacobians themselves.  LC contributions are summed over the pose's incidence
// list in a fixed order (no atomics).  SIX LANES PER POSE: lane a builds row a of D and C and g[a] (one thread per pose held 2 x 36
// accumulators + a Jacobian: 280 registers, one wavefront per SIMD); the six lanes read the same Jacobian, which the memory pipeline
// broadcasts.  Every entry is summed in the order of the one-thread form.
__global__ __launch_bounds__(6 * PG_ASM_POSES) void pg_assemble_kernel(int n, pg_weights W, const double* __restrict__ r, const double* __restrict__ Ji,
                                                          const int* __restrict__ adj_ptr, const int* __restrict__ adj_edge,
                                                          const double* __restrict__ ew, const double* __restrict__ lambda_ptr,
                                                          double* __restrict__ D, double* __restrict__ C, double* __restrict__ g,
                                                          const int* __restrict__ eo, int mp0, int mp1, const int* __restrict__ plist, int np)
{
    const int slot = blockIdx.x * PG_ASM_POSES + threadIdx.x / 6, a = threadIdx.x % 6;
    if (slot >= np) return;
    const int i = plist[slot];
    double Dd[6] = { 0, 0, 0, 0, 0, 0 }, Cc[6] = { 0, 0, 0, 0, 0, 0 }, gg = 0;
    const bool own_i = pg_owns(i, mp0, mp1), own_next = pg_owns(i + 1, mp0, mp1);
    // factor i with this pose as the second variable (Jacobian W)
    const double* w2 = i == 0 ? W.prior : W.odo;
    if (own_i) {
        const double wa = w2[a];
#pragma unroll
        for (int b = 0; b < 6; ++b) if (b == a) Dd[b] += wa * wa;
        gg += wa * r[(size_t)i * 6 + a];
    }
    if (i + 1 < n && own_next) {   // factor i+1 with this pose as the first variable
        double ja[6], sb[6] = { 0, 0, 0, 0, 0, 0 };
        pg_jtj_row(Ji + (size_t)(i + 1) * 36, a, ja, sb);
#pragma unroll
        for (int b = 0; b < 6; ++b) { Dd[b] += sb[b]; Cc[b] = ja[b] * W.odo[b]; }       // C = Ji^T W
        gg += pg_jtr(ja, r + (size_t)(i + 1) * 6);
    }
    for (int p = adj_ptr[i]; p < adj_ptr[i + 1]; ++p) {
        const int code = adj_edge[p], e = code >> 1, second = code & 1;
        if (!pg_owns(eo[e], mp0, mp1)) continue;               // the edge belongs to another rank
        const double* rr = r + (size_t)(n + e) * 6;
        if (second) {
            const double wa = ew[(size_t)e * 6 + a];
#pragma unroll
            for (int b = 0; b < 6; ++b) if (b == a) Dd[b] += wa * wa;
            gg += wa * rr[a];
        } else {
            double ja[6], sb[6] = { 0, 0, 0, 0, 0, 0 };
            pg_jtj_row(Ji + (size_t)(n + e) * 36, a, ja, sb);
#pragma unroll
            for (int b = 0; b < 6; ++b) Dd[b] += sb[b];
            gg += pg_jtr(ja, rr);
        }
    }
    const double lambda = *lambda_ptr;
    if (own_i) {                                               // the damping of a pose is added once, by its owner
#pragma unroll
        for (int b = 0; b < 6; ++b) if (b == a) Dd[b] += lambda;
    }
    g[(size_t)i * 6 + a] = gg;
#pragma unroll
    for (int b = 0; b < 6; ++b) { D[(size_t)i * 36 + a * 6 + b] = Dd[b]; C[(size_t)i * 36 + a * 6 + b] = Cc[b]; }
}

// Schur complement of the interior of segment s (poses L+1 .. R-1) onto its end points L, R (block Thomas recursion).
// Stores the Cholesky factor of every eliminated pivot (Dl), the fill block E_i = H(L, i) and the updated gradient for the
// back-substitution; outputs the end-point corrections.  Per pose the thirteen right-hand sides of D_i^-1 [E_i^T | C_i | g_i] are spread
// over the lanes of a group (each factorises the 6 x 6 pivot itself: cheaper than broadcasting the factor), and the products with E_i
// and C_i^T that follow are column-parallel as well.  One thread per segment took 24 us per pose (3 000 dependent f64 operations, 512
// registers and scratch).  Global memory is touched at ONE point of a step, its top: the blocks of the next step are requested there and
// consumed at the top of the next step, and the records of the back-substitution (E_i, g_i, and the factor of the PREVIOUS step, parked
// in LDS) are stored there, so the one wait on the memory counter per step finds everything a whole step old (dependent loads inside
// the step cost 8 000 of its 12 500 cycles).  E, D, G are double-buffered in LDS.  Rounds 2 - 4 ran SIXTEEN lanes per segment, one
// right-hand side each: ~540 vector instructions per step
struct pg_seg_lds { double E[2][36], D[2][36], G[2][6], C[36], L[36], Rv[6], Wo[6]; };      // 240 doubles (x 32 groups = 61 440 B)
// the lanes of a group sit in one wavefront, whose LDS operations execute in program order: waiting for the LDS queue
// (not for the global stores in flight -- a fence would) and keeping the compiler from moving memory operations across is enough
#define PG_COMPILER_FENCE() asm volatile("" ::: "memory")
#define PG_GROUP_SYNC() do { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_wave_barrier(); } while (0)
// -- the 6 x 6 factor (150, the same on every lane), one pair of triangular solves (42) and two products (72) --
// for FOUR segments, thirteen of sixteen lanes busy and half of the second product thrown away.  EIGHT lanes per segment (round 5; eight
// segments per wavefront): lane c < 6 carries TWO right-hand
// sides -- row c of E_i (its E y accumulates column c of DL) and column c of C_i (its E y is column c of E_(i+1), its C^T y column c of the
// next pivot) -- lane 6 the gradient, lane 7 only helps to move blocks: the factor is computed once per EIGHT segments, the two solves of a
// lane are independent chains (the kernel is bound by dependent f64 latency at two wavefronts per SIMD), and a step is ~520 instructions
// for eight segments (124 -> 103 us per launch at C3).  Every right-hand side sees the arithmetic of the sixteen-lane kernel in the same
// order: the records are the same bits.
#define PG_SEG_LANES 8
// FROMJ (round 5, pass 1 on the pose chain): the blocks of the INTERIOR poses are not read but formed here -- an interior pose p carries
// the chain factors p and p + 1 and nothing else (every loop-closure pose is a separator), so with J = the Jacobian of factor p + 1
//     D_p = diag(w^2) + J^T J + lambda I,   C_p = J^T diag(w),   g_p = w r_p + J^T r_(p+1)
// in the order of operations of pg_assemble_kernel (which then runs on the 48 k ends of the level-1 chain instead of all 400 k poses: it
// wrote 230 MB per trial that this kernel read back).  The Jacobian of the NEXT pose is requested at the top of a step, parked in LDS at
// the step's end (in the slot of C_i, which is free by then) and turned into the lane's column of D, its entries of C and its component
// of g there; D_p is symmetric bit for bit (the products commute, the sums run over the same index), so column c is row c.
// D, C, g are read at the segment's LEFT END only (C_L couples it to the first interior pose).
template <bool FROMJ>
__device__ __forceinline__ void pg_seg_from_j(const double* __restrict__ Jl, const double* __restrict__ Rn, double rp, const double* __restrict__ Wl, double wa, double lambda,
                                              int c, double* __restrict__ nC, double* __restrict__ pre, double& gpre)
{
    if constexpr (FROMJ) {
#pragma unroll
        for (int u = 0; u < 5; ++u) { const int a = c + PG_SEG_LANES * u; if (a < 36) { const int row = a / 6, col = a - 6 * row; nC[u] = Jl[col * 6 + row] * Wl[col]; } }
        if (c < 6) {
            double ja[6], sb[6] = { 0, 0, 0, 0, 0, 0 };
            pg_jtj_row(Jl, c, ja, sb);
#pragma unroll
            for (int b = 0; b < 6; ++b) { double d = b == c ? 0.0 + wa * wa : 0.0; d += sb[b]; if (b == c) d += lambda; pre[b] = d; }
            const double gg = 0.0 + wa * rp;
            gpre = gg + pg_jtr(ja, Rn);
        }
    }
}
template <bool FROMJ>
__global__ __launch_bounds__(256, 2) void pg_segment_kernel(pg_level lv, int* __restrict__ fail, const double* __restrict__ rf, const double* __restrict__ Jf,
                                                            pg_weights W, const double* __restrict__ lambda_ptr)
{
    const double* __restrict__ D = lv.D; const double* __restrict__ C = lv.C; const double* __restrict__ g = lv.g;
    double* __restrict__ E = lv.E; double* __restrict__ Dl = lv.Dl; double* __restrict__ gi = lv.gi;
    double* __restrict__ segDL = lv.segDL; double* __restrict__ segDR = lv.segDR; double* __restrict__ segGL = lv.segGL;
    double* __restrict__ segGR = lv.segGR; double* __restrict__ segS = lv.segS;
    __shared__ pg_seg_lds sh_all[256 / PG_SEG_LANES];
    const int grp = threadIdx.x / PG_SEG_LANES, c = threadIdx.x % PG_SEG_LANES;
    const int slot = blockIdx.x * (256 / PG_SEG_LANES) + grp;
    if (slot >= lv.nseg) return;                                // whole groups leave together
    const int s = lv.order[slot];                               // descending length: the eight segments of a wavefront run the same number of steps
    pg_seg_lds& sh = sh_all[grp];
    const int L = lv.ends[s], R = lv.ends[s + 1];
    if (!pg_owned_segment(lv, s)) return;
    if (R == L + 1) {
        for (int a = c; a < 36; a += PG_SEG_LANES) { segDL[(size_t)s * 36 + a] = 0; segDR[(size_t)s * 36 + a] = 0; segS[(size_t)s * 36 + a] = C[(size_t)L * 36 + a]; }
        if (c < 6) { segGL[(size_t)s * 6 + c] = 0; segGR[(size_t)s * 6 + c] = 0; }
        return;
    }
    double lambda = 0.0, rp = 0.0, rn = 0.0, jn[5] = { 0, 0, 0, 0, 0 }, gpre = 0.0, wa = 0.0;      // FROMJ: r_p[c], r_(p+1)[c], the lane's share of the next Jacobian, its component of g, its weight
    if constexpr (FROMJ) {
        lambda = *lambda_ptr;
        wa = c == 0 ? W.odo[0] : c == 1 ? W.odo[1] : c == 2 ? W.odo[2] : c == 3 ? W.odo[3] : c == 4 ? W.odo[4] : W.odo[5];      // (a lane-dependent index would put the argument into scratch)
        if (c < 6) sh.Wo[c] = wa;
        for (int a = c; a < 36; a += PG_SEG_LANES) { sh.E[0][a] = C[(size_t)L * 36 + a]; sh.C[a] = Jf[(size_t)(L + 2) * 36 + a]; }
        if (c < 6) { rp = rf[(size_t)(L + 1) * 6 + c]; rn = rf[(size_t)(L + 2) * 6 + c]; sh.Rv[c] = rn; }
    } else {
        for (int a = c; a < 36; a += PG_SEG_LANES) { sh.E[0][a] = C[(size_t)L * 36 + a]; sh.D[0][a] = D[(size_t)(L + 1) * 36 + a]; }
        if (c < 6) sh.G[0][c] = g[(size_t)(L + 1) * 6 + c];
    }
    // acc[]: column c of DL on lanes 0..5, GL on lane 6.  pre[]: the prefetched column c of D_(i+1) on lanes 0..5, g_(i+1) on lane 6 -- added
    // to the next step's pivot / gradient at its top (one load sequence for both kinds of lane: two divergent ones that write the same registers are serialised by a full wait).  nC: the lane's
    // share of C_(i+1).
    double nC[5], acc[6] = { 0, 0, 0, 0, 0, 0 }, pre[6] = { 0, 0, 0, 0, 0, 0 };
    const bool has_role = c < 7, is_col = c < 6;
    const int pre_stride = is_col ? 6 : 1;
    const double* pre_src = is_col ? D + c : g;
    const int pre_lds = is_col ? (int)(&sh.D[0][0] - &sh.E[0][0]) + c : (int)(&sh.G[0][0] - &sh.E[0][0]);     // offsets from sh.E[0] in doubles
    const int pre_flip = is_col ? 36 : 6;
    int cb = 0;
    if constexpr (FROMJ) {                                      // the first interior pose: D, g into LDS, its C into nC
#pragma unroll
        for (int u = 0; u < 5; ++u) nC[u] = 0.0;
        PG_GROUP_SYNC();
        double d0[6] = { 0, 0, 0, 0, 0, 0 };
        pg_seg_from_j<true>(sh.C, sh.Rv, rp, sh.Wo, wa, lambda, c, nC, d0, gpre);
        if (c < 6) {
#pragma unroll
            for (int a = 0; a < 6; ++a) sh.D[0][a * 6 + c] = d0[a];
            sh.G[0][c] = gpre;
            rp = rn;
        }
        gpre = 0.0;
        PG_GROUP_SYNC();
    } else {
#pragma unroll
        for (int u = 0; u < 5; ++u) { const int a = c + PG_SEG_LANES * u; nC[u] = a < 36 ? C[(size_t)(L + 1) * 36 + a] : 0.0; }
    }
    for (int i = L + 1; i < R; ++i) {
        const bool last = (i + 1 == R);
        double* __restrict__ Ec = sh.E[cb]; double* __restrict__ Dc = sh.D[cb]; double* __restrict__ Gc = sh.G[cb];
        double* __restrict__ En = sh.E[cb ^ 1]; double* __restrict__ Dn = sh.D[cb ^ 1]; double* __restrict__ Gn = sh.G[cb ^ 1];
#pragma unroll
        for (int u = 0; u < 5; ++u) { const int a = c + PG_SEG_LANES * u; if (a < 36) sh.C[a] = nC[u]; }
        if constexpr (FROMJ) {
            if (is_col) {                                        // completes the entries the last step left in D and G: column c of D_i, component c of g_i
#pragma unroll
                for (int a = 0; a < 6; ++a) Dc[a * 6 + c] += pre[a];
                Gc[c] += gpre;
            }
            if (!last) {                                         // the Jacobian of factor i + 2 and r_(i+2): pose i + 1's blocks, formed at the end of this step
#pragma unroll
                for (int u = 0; u < 5; ++u) { const int a = c + PG_SEG_LANES * u; if (a < 36) jn[u] = Jf[(size_t)(i + 2) * 36 + a]; }
                if (is_col) rn = rf[(size_t)(i + 2) * 6 + c];
            }
        } else {
        if (has_role) {                                          // completes the entries the last step left in D and G
            double* dst = &sh.E[0][0] + pre_lds + cb * pre_flip;
#pragma unroll
            for (int a = 0; a < 6; ++a) dst[a * pre_stride] += pre[a];
        }
        if (!last) {
#pragma unroll
            for (int u = 0; u < 5; ++u) { const int a = c + PG_SEG_LANES * u; if (a < 36) nC[u] = C[(size_t)(i + 1) * 36 + a]; }
            if (has_role) {
                const double* src = pre_src + (size_t)(i + 1) * (is_col ? 36 : 6);
#pragma unroll
                for (int a = 0; a < 6; ++a) pre[a] = src[a * pre_stride];
            }
        } else if (has_role) {
#pragma unroll
            for (int a = 0; a < 6; ++a) pre[a] = 0.0;
        }
        }
        if (i > L + 1) for (int a = c; a < 36; a += PG_SEG_LANES) Dl[(size_t)(i - 1) * 36 + a] = sh.L[a];
        PG_GROUP_SYNC();
        for (int a = c; a < 36; a += PG_SEG_LANES) E[(size_t)i * 36 + a] = Ec[a];
        if (c < 6) gi[(size_t)i * 6 + c] = Gc[c];
        double Li[36];                                           // the factor with 1 / L_jj on its diagonal
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b2 = 0; b2 < 6; ++b2) Li[a * 6 + b2] = b2 <= a ? Dc[a * 6 + b2] : 0.0;
        if (chol6_rdiag(Li)) { *fail = 1; return; }              // every lane of the group sees the same pivot: they leave together
        if (c == 0) {
#pragma unroll
            for (int a = 0; a < 36; ++a) sh.L[a] = Li[a];
        }
        PG_COMPILER_FENCE();
        // right-hand sides of this lane: yA = row c of E (lanes 0..5) or the gradient (lanes 6, 7); yB = column c of C (lanes 0..5; the
        // gradient again on the others, unused)
        double yA[6], yB[6];
        {
            const double* ya = is_col ? Ec + c * 6 : Gc;
            const double* yb = is_col ? sh.C + c : Gc;
            const int bstr = is_col ? 6 : 1;
#pragma unroll
            for (int q = 0; q < 6; ++q) { yA[q] = ya[q]; yB[q] = yb[q * bstr]; }
        }
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            double t = yA[a], u = yB[a];
            for (int k = 0; k < a; ++k) { t -= Li[a * 6 + k] * yA[k]; u -= Li[a * 6 + k] * yB[k]; }
            yA[a] = t * Li[a * 7]; yB[a] = u * Li[a * 7];
        }
#pragma unroll
        for (int a = 5; a >= 0; --a) {
            double t = yA[a], u = yB[a];
            for (int k = a + 1; k < 6; ++k) { t -= Li[k * 6 + a] * yA[k]; u -= Li[k * 6 + a] * yB[k]; }
            yA[a] = t * Li[a * 7]; yB[a] = u * Li[a * 7];
        }
        PG_COMPILER_FENCE();
        {   // E yA: accumulated into DL (lanes 0..5) / GL (lane 6).  E yB: column c of E_next = -E X_C
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                double t = 0, u = 0;
#pragma unroll
                for (int q = 0; q < 6; ++q) { t += Ec[a * 6 + q] * yA[q]; u += Ec[a * 6 + q] * yB[q]; }
                acc[a] -= t;
                if (is_col) En[a * 6 + c] = -u;
            }
        }
        PG_COMPILER_FENCE();
        {   // C^T y: the next pivot less D_(i+1) from yB (lanes 0..5), the next gradient less g_(i+1) from yA (lane 6)
            double yc[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                double ya1 = yA[q], yb1 = yB[q];
                if constexpr (FROMJ) asm volatile("" : "+v"(ya1), "+v"(yb1));      // (register values: the optimiser otherwise selects between the two ARRAYS through scratch memory)
                yc[q] = is_col ? yb1 : ya1;
            }
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                double u = 0;
#pragma unroll
                for (int q = 0; q < 6; ++q) u += sh.C[q * 6 + a] * yc[q];
                if (is_col) Dn[a * 6 + c] = -u;
                else if (c == 6) Gn[a] = -u;
            }
        }
        if constexpr (FROMJ) {
            if (!last) {                                         // C_i has been used for the last time: its slot takes the next Jacobian
                PG_GROUP_SYNC();
#pragma unroll
                for (int u = 0; u < 5; ++u) { const int a = c + PG_SEG_LANES * u; if (a < 36) sh.C[a] = jn[u]; }
                if (is_col) sh.Rv[c] = rn;
                PG_GROUP_SYNC();
                pg_seg_from_j<true>(sh.C, sh.Rv, rp, sh.Wo, wa, lambda, c, nC, pre, gpre);
                rp = rn;
            } else {
#pragma unroll
                for (int a = 0; a < 6; ++a) pre[a] = 0.0;
                gpre = 0.0;
            }
        }
        cb ^= 1;
        PG_GROUP_SYNC();
    }
    for (int a = c; a < 36; a += PG_SEG_LANES) Dl[(size_t)(R - 1) * 36 + a] = sh.L[a];
    if (c < 6) for (int a = 0; a < 6; ++a) segDL[(size_t)s * 36 + a * 6 + c] = acc[a];
    if (c == 6) for (int a = 0; a < 6; ++a) segGL[(size_t)s * 6 + a] = acc[a];
    for (int a = c; a < 36; a += PG_SEG_LANES) { segDR[(size_t)s * 36 + a] = sh.D[cb][a]; segS[(size_t)s * 36 + a] = sh.E[cb][a]; }
    if (c < 6) segGR[(size_t)s * 6 + c] = sh.G[cb][c];
}
template __global__ void pg_segment_kernel<false>(pg_level, int* __restrict__, const double* __restrict__, const double* __restrict__, pg_weights, const double* __restrict__);
template __global__ void pg_segment_kernel<true>(pg_level, int* __restrict__, const double* __restrict__, const double* __restrict__, pg_weights, const double* __restrict__);

// Node k of a level (lv.ends[k]) once its two segments are condensed onto it: segment k - 1 ends in it and adds segDR / segGR, segment k
// starts in it and adds segDL / segGL -- each only on the rank that owns the segment, so the value is a partial sum on an interface
// node.  el < 36: element el of the diagonal block; otherwise component el - 36 of the gradient.
__device__ __forceinline__ bool pg_seg_left(const pg_level& lv, int k) { return k > 0 && pg_owned_segment(lv, k - 1); }
__device__ __forceinline__ bool pg_seg_right(const pg_level& lv, int k) { return k < lv.nseg && pg_owned_segment(lv, k); }
__device__ __forceinline__ double pg_condensed(const pg_level& lv, int k, int el)
{
    const bool blk = el < 36;
    const int w = blk ? 36 : 6, a = blk ? el : el - 36;
    double v = (blk ? lv.D : lv.g)[(size_t)lv.ends[k] * w + a];
    if (pg_seg_left(lv, k)) v += (blk ? lv.segDR : lv.segGR)[(size_t)(k - 1) * w + a];
    if (pg_seg_right(lv, k)) v += (blk ? lv.segDL : lv.segGL)[(size_t)k * w + a];
    return v;
}
// the level-1 chain after pass 1: diagonal block, coupling to the next entry and gradient of every chunk end / true separator
// (what pass 2 of pg_segment_kernel condenses; same meaning as D, C, g of the pose chain).  Partial sums on interface entries.
__global__ __launch_bounds__(256) void pg_chain1_kernel(pg_level lv0, pg_level lv1)
{
    double* __restrict__ D1 = lv1.D; double* __restrict__ C1 = lv1.C; double* __restrict__ g1 = lv1.g;
    // one thread per element (36 of D1 / C1 + 6 of g1 per node): a thread per node read its eight 288-byte rows alone (114 us)
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int k = (int)(t / 42), a = (int)(t - 42LL * k);
    if (k > lv0.nseg) return;
    if (a < 36) {
        D1[(size_t)k * 36 + a] = pg_condensed(lv0, k, a);
        C1[(size_t)k * 36 + a] = pg_seg_right(lv0, k) ? lv0.segS[(size_t)k * 36 + a] : 0.0;
    } else g1[(size_t)k * 6 + a - 36] = pg_condensed(lv0, k, a);
}

// reduced system: diagonal blocks, chain couplings and right-hand side (one thread per separator, chain order).  Value index
// k = diagonal block of separator k, ns + k = chain coupling S(k, k+1), 2 ns - 1 + e = LC edge e (dsss_pg_sym.h).  A value
// whose destination column is binned goes straight into the block-sparse factor (dest >= 0: position << 1 | transpose); the
// others go, untransposed, into the value array the fronts assemble from.
__global__ __launch_bounds__(256) void pg_scatter_base_kernel(pg_level lv, const int* __restrict__ perm, const int* __restrict__ dest,
                                                              double* __restrict__ Lvals, double* __restrict__ aval, double* __restrict__ rhs,
                                                              const int* __restrict__ if_slot, double* __restrict__ aval_if, double* __restrict__ x_if)
{
    // one thread per element: 36 of the diagonal block, 6 of the right-hand side, 36 of the coupling S(k, k+1)
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int k = (int)(t / 78), el = (int)(t - 78LL * k), ns = lv.nseg + 1;
    if (k >= ns) return;
    const int code = dest[k];
    const bool iface = code <= -2, own = pg_owns(lv.ends[k], lv.lo, lv.hi);
    if (el < 42) {
        if (!(iface || own)) return;
        // an interface separator takes a partial sum from every rank (summed by the all-reduce), an interior one is complete
        if (el < 36) {
            double* dst = code >= 0 ? Lvals + (size_t)(code >> 1) * 36 : (iface ? aval_if + (size_t)(-2 - code) * 36 : aval + (size_t)k * 36);
            dst[el] = pg_condensed(lv, k, el);
        } else {
            double* rr = iface ? x_if + (size_t)if_slot[k] * 6 : rhs + (size_t)perm[k] * 6;
            rr[el - 36] = -pg_condensed(lv, k, el);
        }
    } else if (pg_seg_right(lv, k)) {     // S(k, k+1), written by the owner of segment k: the factor holds the (larger index, smaller index) block
        const int e = el - 42, a = e / 6, b = e - 6 * a;
        const int cc = dest[ns + k];
        const double* S = lv.segS + (size_t)k * 36;
        if (cc >= 0) Lvals[(size_t)(cc >> 1) * 36 + e] = (cc & 1) ? S[b * 6 + a] : S[e];
        else (cc <= -2 ? aval_if + (size_t)(-2 - cc) * 36 : aval + (size_t)(ns + k) * 36)[e] = S[e];
    }
}
// LC off-diagonal blocks H(a, b) = Ji^T W, added after the chain couplings.  The pipeline's per-ping selection gives every unordered
// pose pair at most one loop closure; a caller of dsss_posegraph_solve_edges may pass several (in either direction).  Those land on
// ONE block of the factor: the host chains them in edge order (lc_link[2 e] = e is the first of its group, lc_link[2 e + 1] = the next
// member or -1; NULL when no pair repeats) and the first member's threads add the whole group -- one writer per element, the sum in
// edge order whatever the number of duplicates: same bits every run.  (Round 4 added them atomically, which is order-independent for
// two addends on an empty block only.)
__global__ __launch_bounds__(256) void pg_scatter_lc_kernel(int n, int ne, int ns, const double* __restrict__ Ji, const double* __restrict__ ew,
                                                            const int* __restrict__ dest, double* __restrict__ Lvals, double* __restrict__ aval,
                                                            double* __restrict__ aval_if, const int* __restrict__ eo, int mp0, int mp1, const int* __restrict__ lc_link)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;          // one thread per element of the 6 x 6 block
    const int e = (int)(t / 36), el = (int)(t - 36LL * e);
    if (e >= ne) return;
    if (!pg_owns(eo[e], mp0, mp1)) return;
    const int code = dest[2 * ns - 1 + e];
    if (code >= 0) {                                                        // element el of the factor's block (a group shares code >> 1)
        if (lc_link && !lc_link[2 * e]) return;
        double* dst = Lvals + (size_t)(code >> 1) * 36 + el;
        double v = *dst;
        for (int q = e; q >= 0; q = lc_link ? lc_link[2 * q + 1] : -1) {
            const int tr = dest[2 * ns - 1 + q] & 1;                        // this member's block is stored transposed
            const int a = tr ? el % 6 : el / 6, b = tr ? el / 6 : el % 6;
            v += Ji[(size_t)(n + q) * 36 + b * 6 + a] * ew[(size_t)q * 6 + b];      // (Ji^T W)(a, b)
        }
        *dst = v;
    } else {                                                                // the fronts' value array: a slot per edge, summed by the extend-add
        const int a = el / 6, b = el - 6 * a;
        (code <= -2 ? aval_if + (size_t)(-2 - code) * 36 : aval + (size_t)(2 * ns - 1 + e) * 36)[el] = Ji[(size_t)(n + e) * 36 + b * 6 + a] * ew[(size_t)e * 6 + b];
    }
}

// update matrices that cross from this rank's interior into the interface, packed (6b x 6b lower block triangle, then 6b of
// right-hand side) into the buffer the all-reduce sums; one workgroup per (child, block row)
__global__ __launch_bounds__(256) void pg_comm_pack_kernel(const int* __restrict__ it_child, const int* __restrict__ it_row, const pg_pack* __restrict__ PK)
{
    const pg_pack pk = PK[it_child[blockIdx.x]];
    const int i = it_row[blockIdx.x], b6 = 6 * pk.cb, wcols = 6 * (i + 1);
    for (int cc = threadIdx.x; cc < wcols; cc += 256) {
#pragma unroll
        for (int a = 0; a < 6; ++a) pk.dst[(size_t)(6 * i + a) * b6 + cc] = pk.U[(size_t)(6 * i + a) * pk.cld + cc];
    }
    if (threadIdx.x < 6) pk.dst[(size_t)b6 * b6 + 6 * i + threadIdx.x] = pk.g[6 * i + threadIdx.x];
}
// interface right-hand sides out of the summed buffer into the solver's vector; three scalars + the failure flag into the
// little buffer of the second all-reduce
__global__ __launch_bounds__(256) void pg_comm_xif_kernel(int nif, const int* __restrict__ if_sep, const int* __restrict__ perm, const double* __restrict__ x_if, double* __restrict__ x)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nif) return;
    for (int a = 0; a < 6; ++a) x[(size_t)perm[if_sep[q]] * 6 + a] = x_if[(size_t)q * 6 + a];
}
__global__ void pg_comm_scal_kernel(const double* __restrict__ scal, const int* __restrict__ fail, double* __restrict__ red)
{
    if (threadIdx.x < 3) red[threadIdx.x] = scal[threadIdx.x];
    if (threadIdx.x == 3) red[3] = (double)*fail;
}

// the solution at the ends of a level's segments, out of x: the solver's vector through `perm`, or (perm NULL) the delta of the level above
__global__ __launch_bounds__(256) void pg_sep_delta_kernel(pg_level lv, const int* __restrict__ perm, const double* __restrict__ x)
{
    const int* __restrict__ sep_pose = lv.ends; double* __restrict__ delta = lv.delta;
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k > lv.nseg) return;
    const int src = perm ? perm[k] : k;
    if (src < 0) return;                                     // (rank-local analysis: another rank's interior separator -- not solved here, not read here)
    for (int a = 0; a < 6; ++a) delta[(size_t)sep_pose[k] * 6 + a] = x[(size_t)src * 6 + a];
}

// interiors, right to left: delta_i = D_i^-1 (-g_i - E_i^T delta_L - C_i delta_{i+1}).  EIGHT LANES PER SEGMENT: lane a < 6 forms
// component a of the right-hand side (column a of E_i, row a of C_i: the group reads the 288-byte blocks together; one thread
// per segment read them alone, 8.7 us per pose), the six components are exchanged, and every lane solves the 6 x 6 system itself,
// which leaves delta_i in all of them for the next step.  The blocks of pose i - 1 are requested before pose i is computed.
#define PG_BS_LANES 8
struct pg_bs_blk { double Ec[6], Cr[6], gv, Lm[21]; };
// FROMJ (pass 1 on the pose chain): row aa of C_i = column aa of the Jacobian of factor i + 1, times the weights -- the product
// pg_assemble_kernel forms (it no longer writes the blocks of interior poses, see pg_segment_kernel<true>)
template <bool FROMJ>
__device__ __forceinline__ void pg_bs_load(pg_bs_blk& B, int i, int aa, const double* __restrict__ C, const double* __restrict__ E,
                                           const double* __restrict__ Dl, const double* __restrict__ gi, const double* __restrict__ Jf, const pg_weights& W)
{
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        B.Ec[q] = E[(size_t)i * 36 + q * 6 + aa];
        if constexpr (FROMJ) B.Cr[q] = Jf[(size_t)(i + 1) * 36 + q * 6 + aa] * W.odo[q];
        else B.Cr[q] = C[(size_t)i * 36 + aa * 6 + q];
    }
    B.gv = gi[(size_t)i * 6 + aa];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int k = 0; k <= r; ++k) B.Lm[r * (r + 1) / 2 + k] = Dl[(size_t)i * 36 + r * 6 + k];
}
template <bool FROMJ>
__global__ __launch_bounds__(256) void pg_backsub_kernel(pg_level lv, const double* __restrict__ Jf, pg_weights W)
{
    const double* __restrict__ C = lv.C; const double* __restrict__ E = lv.E; const double* __restrict__ Dl = lv.Dl;
    const double* __restrict__ gi = lv.gi; double* __restrict__ delta = lv.delta;
    const int slot = blockIdx.x * (256 / PG_BS_LANES) + threadIdx.x / PG_BS_LANES, a = threadIdx.x % PG_BS_LANES;
    if (slot >= lv.nseg) return;                                // whole groups leave together
    const int s = lv.order[slot];                               // descending length, as in pg_segment_kernel
    const int L = lv.ends[s], R = lv.ends[s + 1];
    if (!pg_owned_segment(lv, s) || R == L + 1) return;
    const int aa = a < 6 ? a : 5;                               // lanes 6 and 7 shadow lane 5 and store nothing
    double dL[6], dn[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) { dL[q] = delta[(size_t)L * 6 + q]; dn[q] = delta[(size_t)R * 6 + q]; }
    pg_bs_blk cur, nxt;
    pg_bs_load<FROMJ>(cur, R - 1, aa, C, E, Dl, gi, Jf, W);
    for (int i = R - 1; i > L; --i) {
        if (i - 1 > L) pg_bs_load<FROMJ>(nxt, i - 1, aa, C, E, Dl, gi, Jf, W);
        double t = -cur.gv;
#pragma unroll
        for (int q = 0; q < 6; ++q) { t -= cur.Ec[q] * dL[q]; t -= cur.Cr[q] * dn[q]; }
        double b[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) b[q] = __shfl(t, q, PG_BS_LANES);
        // (L L^T) x = b; the record holds 1 / L_jj on the diagonal (pg_segment_kernel)
#pragma unroll
        for (int r = 0; r < 6; ++r) { double v = b[r]; for (int k = 0; k < r; ++k) v -= cur.Lm[r * (r + 1) / 2 + k] * b[k]; b[r] = v * cur.Lm[r * (r + 1) / 2 + r]; }
#pragma unroll
        for (int r = 5; r >= 0; --r) { double v = b[r]; for (int k = r + 1; k < 6; ++k) v -= cur.Lm[k * (k + 1) / 2 + r] * b[k]; b[r] = v * cur.Lm[r * (r + 1) / 2 + r]; }
        const double mine = a == 0 ? b[0] : a == 1 ? b[1] : a == 2 ? b[2] : a == 3 ? b[3] : a == 4 ? b[4] : b[5];
        if (a < 6) delta[(size_t)i * 6 + a] = mine;
#pragma unroll
        for (int q = 0; q < 6; ++q) dn[q] = b[q];
        cur = nxt;
    }
}
template __global__ void pg_backsub_kernel<false>(pg_level, const double* __restrict__, pg_weights);
template __global__ void pg_backsub_kernel<true>(pg_level, const double* __restrict__, pg_weights);

// 0.5 * || J delta + r ||^2 over all factors (linear.error(delta))
__global__ __launch_bounds__(256) void pg_linerr_kernel(int n, int ne, pg_weights W, const int* __restrict__ ea, const int* __restrict__ eb, const int* __restrict__ eo,
                                                        const double* __restrict__ ew, const double* __restrict__ r, const double* __restrict__ Ji,
                                                        const double* __restrict__ delta, double* __restrict__ partial, int mp0, int mp1)
{
    __shared__ double s_w[4];
    // a block covers 256 factors; a thread takes residual component (factor, a) six times over, so that consecutive threads read
    // consecutive rows of the Jacobians (a thread per factor read its 288-byte block alone)
    double e2 = 0;
#pragma unroll
    for (int it = 0; it < 6; ++it) {
        const int el = it * 256 + threadIdx.x, k = blockIdx.x * 256 + el / 6, a = el % 6;
        if (k < n + ne && pg_owned_factor(k, n, eo, mp0, mp1)) {
            int i = -1, j; double wa;
            if (k == 0) { j = 0; wa = W.prior[a]; }
            else if (k < n) { i = k - 1; j = k; wa = W.odo[a]; }
            else { i = ea[k - n]; j = eb[k - n]; wa = ew[(size_t)(k - n) * 6 + a]; }
            double s = r[(size_t)k * 6 + a] + wa * delta[(size_t)j * 6 + a];
            if (i >= 0) for (int q = 0; q < 6; ++q) s += Ji[(size_t)k * 36 + a * 6 + q] * delta[(size_t)i * 6 + q];
            e2 += s * s;
        }
    }
    const double s = block_sum256(e2, s_w);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void pg_retract_kernel(int n, const pose_t* __restrict__ X, const double* __restrict__ delta, pose_t* __restrict__ Xn)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    pose_t o;
    pose_retract(&X[i], delta + (size_t)i * 6, &o);
    Xn[i] = o;
}


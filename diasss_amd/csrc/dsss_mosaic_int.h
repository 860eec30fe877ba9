// diasss_amd/csrc/dsss_mosaic_int.h -- what the mosaic family shares (dsss_mosaic.hip, dsss_mosaic_comp.hip, dsss_mosaic_reg.hip,
// dsss_mosaic_canvas.hip, dsss_mosaic_profile.hip); every rule here is written once and nowhere else.  Device: the job and window
// records and the job lookup (mosaic_job_of); the ping prologue of every ping-per-workgroup kernel (mosaic_ping_of: pose row, gain row,
// bearings in LDS, in the partner form a second row, the neighbouring ping or one the caller names); the rules of a sample (mask, cell,
// corrected value: mosaic_sample_cell) and the sub-samples of a footprint (footprint_steps, mosaic_footprint_samples); the segmented
// reduction (mosaic_run_reduce) and the accumulator word count << 32 | sum (mosaic_acc: packing a run, the signed add, count and sum of
// a word, the sample limit, the rounded mean); the two sample loops of the mean, each with a sign (mosaic_scatter_samples,
// mosaic_scatter_footprints); the rules of the composite and the score, order and sub-cell rules of the registration, one body for host
// and device.  Host: the typed arena over mosaic_buf and the three layers of a read in it (mosaic_layers), the argument rules
// (mosaic_check_args), the windows of the grid (mosaic_grid_win, mosaic_window with its metric growth), the cut of a job table into
// launches (mosaic_cut_launches), the sample-limit flag (mosaic_flag_down), the upload of a caller's trajectory and the scatter launch,
// defined in dsss_mosaic.hip, and what dsss_mosaic_reg.hip needs of the registration's host arithmetic (dsss_mosaic_edge.cpp).
#pragma once
#include "dsss_internal.h"

#define MOSAIC_MAX_CELLS (1ll << 28)
#define MOSAIC_MAX_SAMPLES (1u << 24)      // per cell: 255 * 2^24 < 2^32, the u32 sum cannot wrap below it
#define REG_MAX_RADIUS 16                  // the registration's search radius, in cells
#define REG_MAX_YAW 17                     // angles of a yaw fan
#define PYR_MAX_LEVELS 4                   // levels of a cell pyramid
#define PYR_MAX_CENTRE (1 << 28)           // |cx|, |cy| of a level's centre: twice the centre plus the radius stays an int32

// the one-band record: what a column table, or no table, is to everything that carries bands (every altitude lies in band 0)
__host__ __device__ constexpr dsss_gain_bands gain_one_band() { return dsss_gain_bands{ 0.0, 1.0, 1, 0 }; }

// one frame of a launch: its pose rows (the frame's own or the caller's trajectory), geometry and images; blk0 = its first workgroup;
// gain = the context's range-gain table (M x u16, Q8), null: none set -- the same in every job of a launch, so the test is uniform
// g0 = the canonical number of the frame's first ping (composite mosaic; the other kernels do not read it)
// alt, bands = the frame's altitudes and the bands of a banded table ("altitude-banded range gain" in the header): gain then holds
// bands.nbands rows of M, and a ping reads the row of its altitude's band; nbands == 1 (a column table, or none): alt is not read
struct mosaic_job { const double* pose; const double* gr; const uint8_t* img; const uint8_t* mask; const uint16_t* gain; int N, M, blk0, g0;
                    const double* alt = nullptr; dsss_gain_bands bands = gain_one_band(); };
// the grid (x0, y0, cell, W, H: where a point falls and whether it is kept) and the window of it the accumulators cover
// (ox, oy, bw, bh: the whole grid for the mosaic, one frame's cell bounding box for the consistency map and the registration)
struct mosaic_win { double x0, y0, cell; int W, H, ox, oy, bw, bh, use_mask; };
// one segment of a frame in the segmented scatter: its window of the grid (bw = 0: no cell of it lies on the grid) and where its
// accumulators start, in cells, behind the frame's first
struct mosaic_seg { int ox, oy, bw, bh; unsigned long long off; };

// the corrected sample ("range-gain normalisation" in the header); gain == null: none set
__device__ __forceinline__ unsigned mosaic_gain_apply(unsigned v, const uint16_t* __restrict__ gain, int col)
{
    return gain ? min(255u, (v * gain[col] + 128u) >> 8) : v;
}

// the band of an altitude, ONE body for dsss_gain_band and the kernels (B as the entries admit it: nbands >= 1, dalt > 0, both finite)
__host__ __device__ inline int gain_band(const dsss_gain_bands& B, double alt)
{
    const double t = floor((alt - B.alt0) / B.dalt);
    if (!(t >= 0.0)) return 0;                                                     // on the f64 value: NaN, -inf and altitudes below alt0
    if (t >= (double)B.nbands) return B.nbands - 1;
    return (int)t;
}
// the row of the job's table that the ping `row` of its frame is corrected with (uniform per ping); null: no table set
__device__ __forceinline__ const uint16_t* mosaic_gain_row(const mosaic_job& J, int row)
{
    return J.bands.nbands > 1 ? J.gain + (size_t)gain_band(J.bands, J.alt[row]) * J.M : J.gain;
}

// The three rules of a sample on the device, each written once: the mask test (mosaic_sample_kept: -1 for a column behind M or one the
// mask rejects, what kept() returns otherwise; mask = the ping's row of the frame's mask), the cell of the window G a point falls into
// (mosaic_point_cell: -1 off the grid or the window or not finite, otherwise the cell, after kept() ran) and the corrected value
// (mosaic_gain_apply above).  mosaic_sample_cell puts them together for a point sample, mosaic_footprint_samples for the sub-samples of
// a footprint.  What follows a test is handed in and runs in tail position, so a caller's code is what it was with the tests written
// out in it (the point kernels' instructions did not change when these were split off).
template <class KEPT>
__device__ __forceinline__ int mosaic_sample_kept(int M, const uint8_t* __restrict__ mask, int col, const mosaic_win& G, KEPT kept)
{
    if (col >= M || (G.use_mask && mask[col] == 0)) return -1;
    return kept();
}
template <class KEPT>
__device__ __forceinline__ int mosaic_point_cell(double x, double y, const mosaic_win& G, KEPT kept)
{
    const double fx = floor((x - G.x0) / G.cell), fy = floor((y - G.y0) / G.cell);
    if (!(fx >= 0.0 && fx < (double)G.W && fy >= 0.0 && fy < (double)G.H)) return -1;   // on the f64 values: NaN, infinite and huge points drop out here
    const int ix = (int)fx - G.ox, iy = (int)fy - G.oy;
    if (!(ix >= 0 && ix < G.bw && iy >= 0 && iy < G.bh)) return -1;
    kept();
    return iy * G.bw + ix;
}

// The one place a sample is binned on the device: the cell of the window G that the sample (row, col) falls into, -1 when it is
// dropped (mask, off the grid or the window, not finite), and *val = its corrected value.  P = the ping's pose row, sc = sin and cos of
// the bearing of the port and of the starboard side (dsss_geo_side on P, in LDS), img, mask = the ping's row of the frame's images.
// The mean scatter, the yaw fan and the composite scatter call it; a caller that does not use *val pays nothing for it.
__device__ __forceinline__ int mosaic_sample_cell(const double* P, const double* sc, const mosaic_job& J, const uint8_t* __restrict__ img,
                                                  const uint8_t* __restrict__ mask, int col, const mosaic_win& G, unsigned* val)
{
    const int M = J.M, half = M / 2;
    return mosaic_sample_kept(M, mask, col, G, [&] {
        const int side = col >= half;
        double x, y;
        dsss_geo_bin(P, J.gr, M, col, sc[2 * side], sc[2 * side + 1], &x, &y);
        return mosaic_point_cell(x, y, G, [&] { *val = mosaic_gain_apply(img[col], J.gain, col); });      // (J.gain: uniform per workgroup)
    });
}

// The job of this workgroup in a table whose blk0 ascend from 0: the last one whose blk0 is not above blockIdx.x.  The one job lookup
// of the family; JOB needs a blk0 and nothing else (mosaic_job here, the registration's own records in dsss_mosaic_reg.hip).
template <class JOB> __device__ __forceinline__ JOB mosaic_job_of(const JOB* __restrict__ jobs, int njobs)
{
    int lo = 0, hi = njobs - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (jobs[mid].blk0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1; }
    return jobs[lo];
}

// the footprint kernels' partner of a ping: the next ping of the frame, the one before for its last (a frame of one ping: itself)
struct mosaic_partner_neighbour {
    template <class JOB> __device__ __forceinline__ const double* operator()(const JOB& J, int row, bool& last) const
    { last = row == J.N - 1; return J.pose + (size_t)(last ? (row > 0 ? row - 1 : row) : row + 1) * 6; }
};

// What a workgroup of one ping does first, in every ping-per-workgroup kernel of the family: its job J, the ping's row in the frame and
// pose row P, and sin and cos of the bearing of each side in s_sc (the kernel's __shared__ double[4]), behind the barrier.  False: the
// workgroup has no ping; it leaves in front of the barrier (uniform per workgroup; cannot happen with the host's blk0).
// The partner form (PP given): *PP = partner(J, row, *last), a second pose row -- the ping's neighbour for the footprint kernels
// (mosaic_partner_neighbour), the row the frame moves to for the canvas's fused move -- and s_sc is the kernel's __shared__ double[8]:
// behind the ping's four values, sin and cos of both sides of the partner.  JOB = mosaic_job, or a record that derives from it (the
// profile's prof_job, the canvas's canvas_job).
template <class JOB, class PARTNER = mosaic_partner_neighbour>
__device__ __forceinline__ bool mosaic_ping_of(const JOB* __restrict__ jobs, int njobs, double* s_sc, JOB& J, int& row, const double*& P,
                                               const double** PP = nullptr, bool* last = nullptr, PARTNER partner = PARTNER())
{
    J = mosaic_job_of(jobs, njobs); row = (int)blockIdx.x - J.blk0;
    if (row >= J.N) return false;
    P = J.pose + (size_t)row * 6;
    J.gain = mosaic_gain_row(J, row);                                              // the ping's band, once per workgroup: the samples see a column table
    if (PP) {
        *PP = partner(J, row, *last);
        if (threadIdx.x < 4) dsss_geo_side(threadIdx.x < 2 ? P : *PP, threadIdx.x & 1, &s_sc[2 * threadIdx.x], &s_sc[2 * threadIdx.x + 1]);
    }
    else if (threadIdx.x < 2) dsss_geo_side(P, threadIdx.x == 1, &s_sc[2 * threadIdx.x], &s_sc[2 * threadIdx.x + 1]);
    __syncthreads();
    return true;
}

// The segmented reduction of the family, written once: lanes of a wavefront that hold the same key as their neighbour form a run, v is
// reduced with op over the lane's run (afterwards v = op over the run's lanes up to this one), and the last lane of a run gets true: it
// holds the run's value and issues the run's ONE atomic.  op is associative; the mean scatter reduces with +, the composite with min.
template <class T, class OP> __device__ __forceinline__ bool mosaic_run_reduce(int key, T& v, OP op)
{
    const int lane = threadIdx.x & 63;
    const int prev = __shfl_up(key, 1);
    const bool head = lane == 0 || prev != key;
    const unsigned long long hb = __ballot(head);
    const int start = 63 - __clzll((long long)(hb & (~0ull >> (63 - lane))));       // first lane of this lane's run
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const T t = __shfl_up(v, d); if (lane - d >= start) v = op(v, t); }
    return lane == 63 || ((hb >> (lane + 1)) & 1ull);
}

// The accumulator word of a cell of the mean mosaic, count << 32 | sum, in its one place: a word read back is taken apart (c, s, the
// sample limit, the rounded mean), a run's value v (count << 16 | sum within the wavefront) is packed and added, signed.  The word is
// modular: a negative add (the canvas) adds the two's complement, and while the jobs of one call are in flight a borrow or carry may
// pass between sum and count.  That is harmless: the adds commute, every job of a call has landed before anything is read, and then
// both fields are what a fresh render of the same frames gives -- only the final fields are ever read.
struct mosaic_acc {
    uint32_t c, s;
    __device__ __forceinline__ explicit mosaic_acc(unsigned long long a) : c((uint32_t)(a >> 32)), s((uint32_t)a) {}
    __device__ __forceinline__ bool over_limit() const { return c > MOSAIC_MAX_SAMPLES; }
    __device__ __forceinline__ uint32_t mean() const { return (s + c / 2) / c; }   // c > 0
    static __device__ __forceinline__ unsigned long long word(unsigned v) { return ((unsigned long long)(v >> 16) << 32) | (v & 0xffffu); }
    template <bool SIGNED> static __device__ __forceinline__ void add(unsigned long long* acc, int key, unsigned v, bool negative)
    { atomicAdd(&acc[key], SIGNED && negative ? 0ull - word(v) : word(v)); }      // (SIGNED false: always added, the render kernels; the atomic without return)
};

// what the lanes of a wavefront add to their cells: v (0 under key -1) summed over the runs, the run's ONE atomic by its tail lane
template <bool SIGNED> __device__ __forceinline__ void mosaic_run_add(unsigned long long* __restrict__ acc, int key, unsigned v, bool negative)
{
    const bool tail = mosaic_run_reduce(key, v, [](unsigned a, unsigned b) { return a + b; });
    if (tail && key >= 0) mosaic_acc::add<SIGNED>(acc, key, v, negative);
}

// The samples of one ping, by the 256 threads of its workgroup (mosaic_scatter_kernel's comment in dsss_mosaic.hip): row = the ping's
// row in the frame's images, acc = the window's accumulators.  SIGNED (the canvas): negative = the samples are taken out, uniform per
// workgroup; everywhere else the sign is no question at compile time.
template <bool SIGNED = false>
__device__ __forceinline__ void mosaic_scatter_samples(const double* P, const double* sc, const mosaic_job& J, int row, const mosaic_win& G,
                                                       unsigned long long* __restrict__ acc, bool negative = false)
{
    const int M = J.M;
    const uint8_t* __restrict__ img = J.img + (size_t)row * M;
    const uint8_t* __restrict__ mask = J.mask + (size_t)row * M;
    for (int c0 = 0; c0 < M; c0 += 256) {
        unsigned g = 0;
        const int key = mosaic_sample_cell(P, sc, J, img, mask, c0 + (int)threadIdx.x, G, &g);
        mosaic_run_add<SIGNED>(acc, key, key >= 0 ? (1u << 16) | g : 0u, negative);     // v: count << 16 | sum within the wavefront
    }
}

// ---- footprint rendering ("footprint rendering" in the header): a sample stands for the area up to the next ping and the next bin
#define FP_MAX_STEPS 8
// the sub-samples along a step S = (sx, sy), ONE body for dsss_mosaic_footprint_steps and the kernels (F and cell as the entries admit
// them); every comparison on the f64 values: a NaN or infinite component fails the first test
__host__ __device__ inline int footprint_steps(const dsss_footprint_params& F, double cell, double sx, double sy)
{
    const double ax = fabs(sx), ay = fabs(sy);
    if (!(ax <= 1.7976931348623157e308 && ay <= 1.7976931348623157e308)) return 1;  // not finite
    const double l = ax > ay ? ax : ay;
    if (l > F.max_gap) return 1;                                                   // a jump is not bridged
    const double t = ceil(l / cell);
    if (t < 1.0) return 1;
    if (t > (double)F.max_steps) return F.max_steps;
    return (int)t;
}

// The sub-samples of one ping, by the 256 threads of its workgroup: what mosaic_scatter_samples does for the samples.  PP = the pose row
// of the partner ping and last (mosaic_ping_of's partner form), sc = the eight values it left in LDS.  A lane owns a column: its point,
// the partner ping's and its across neighbour's (three dsss_geo_bin), the along step A and the across step B, and na, nc sub-samples
// along them -- 0 for a lane whose sample is not kept.  The (i, j) loops run to the wavefront's maxima of na and nc, uniform over the
// wavefront, because the shuffles of mosaic_run_reduce need every lane; a lane with i >= na or j >= nc carries key -1.  Consecutive
// columns still walk through the grid for a fixed (i, j), so runs form as they do for the samples.  value(col) = what the lane
// contributes, once per kept sample; emit(key, v) = the reduction over the runs and the run's one atomic.  Every operation on a
// coordinate is one unfused IEEE operation in the order of the header; x + (i / na) ax does not depend on j and is formed once per i.
template <class VALUE, class EMIT>
__device__ __forceinline__ void mosaic_footprint_samples(const double* P, const double* PP, bool last, const double* sc, const mosaic_job& J, int row,
                                                         const mosaic_win& G, const dsss_footprint_params& F, VALUE value, EMIT emit)
{
    const int M = J.M, half = M / 2;
    const uint8_t* __restrict__ mask = J.mask + (size_t)row * M;
    for (int c0 = 0; c0 < M; c0 += 256) {
        const int col = c0 + (int)threadIdx.x;
        double x = 0.0, y = 0.0, ax = 0.0, ay = 0.0, bx = 0.0, by = 0.0;
        int na = 0, nc = 0;
        unsigned v = 0;
        mosaic_sample_kept(M, mask, col, G, [&] {
            const int side = col >= half, idx = dsss_geo_index(M, col);
            const bool outer = idx >= half - 1;                                    // the side's last index: the step comes from the bin inside
            const int nidx = outer ? idx - 1 : idx + 1, ncol = side ? half + nidx : half - nidx;
            const double s = sc[2 * side], c = sc[2 * side + 1];
            double xn, yn, xp, yp;
            dsss_geo_bin(P, J.gr, M, col, s, c, &x, &y);
            dsss_geo_bin(P, J.gr, M, ncol, s, c, &xn, &yn);
            dsss_geo_bin(PP, J.gr, M, col, sc[4 + 2 * side], sc[5 + 2 * side], &xp, &yp);
            ax = last ? x - xp : xp - x; ay = last ? y - yp : yp - y;              // (a frame of one ping: x - x, one sub-sample either way)
            bx = outer ? x - xn : xn - x; by = outer ? y - yn : yn - y;
            na = footprint_steps(F, G.cell, ax, ay); nc = footprint_steps(F, G.cell, bx, by);
            v = value(col);
            return 0;
        });
        int na_max = 0, nc_max = 0;                                                // over the wavefront: scalar
#pragma unroll
        for (int k = 0; k < FP_MAX_STEPS; ++k) { na_max += __ballot(na > k) != 0ull; nc_max += __ballot(nc > k) != 0ull; }
        for (int i = 0; i < na_max; ++i) {
            double xi = x, yi = y;
            if (i > 0) { const double q = (double)i / (double)na; xi = xi + q * ax; yi = yi + q * ay; }
            for (int j = 0; j < nc_max; ++j) {
                double xs = xi, ys = yi;
                if (j > 0) { const double q = (double)j / (double)nc; xs = xs + q * bx; ys = ys + q * by; }
                emit(i < na && j < nc ? mosaic_point_cell(xs, ys, G, [] {}) : -1, v);
            }
        }
    }
}

// the mean's sub-samples: mosaic_scatter_samples' sum and count over the runs and its sign, the parent's corrected value
template <bool SIGNED = false>
__device__ __forceinline__ void mosaic_scatter_footprints(const double* P, const double* PP, bool last, const double* sc, const mosaic_job& J, int row,
                                                          const mosaic_win& G, const dsss_footprint_params& F, unsigned long long* __restrict__ acc, bool negative = false)
{
    const uint8_t* __restrict__ img = J.img + (size_t)row * J.M;
    mosaic_footprint_samples(P, PP, last, sc, J, row, G, F,
        [&](int col) { return (1u << 16) | mosaic_gain_apply(img[col], J.gain, col); },
        [&](int key, unsigned g) { mosaic_run_add<SIGNED>(acc, key, key >= 0 ? g : 0u, negative); });
}

// ---- composite mosaic ("composite mosaic" in the header; dsss_mosaic_comp.hip).  A cell's key: q << 47 | g << 16 | col, 15 + 31 + 16
// bits, so the top two bits of a sample's key are 0 and all ones, the value the cells are cleared to, is no sample's key.
#define COMP_EMPTY (~0ull)
#define COMP_MAX_M 65534                   // q <= half - 1 <= 32766 and col < 2^16
#define COMP_MAX_FILL 4                    // the fill radius, in cells
// the priority rank of a column, ONE body for dsss_mosaic_comp_rank and mosaic_composite_kernel (mode 0..3, M even)
__host__ __device__ inline int comp_rank(int mode, int M, int col)
{
    const int half = M / 2, idx = dsss_geo_index(M, col);
    if (mode == DSSS_COMP_NEAR) return idx;
    if (mode == DSSS_COMP_FAR) return half - 1 - idx;
    if (mode == DSSS_COMP_MID) { const int d = 2 * idx - (half - 1); return d < 0 ? -d : d; }
    return 0;
}
// The fill rule of one empty cell, ONE body for dsss_mosaic_fill_host and mosaic_fill_kernel: valid(x, y) = 1 where the cell is in V0,
// 0 elsewhere and outside the grid.  Returns dx^2 + dy^2 of the donor and its offset, or 0 when the cell is not enclosed.  A candidate
// is packed as d2 << 16 | dy + 4 << 8 | dx + 4, so the smallest integer is the first under (d2, dy, dx) whatever the order of the
// visit; a cell outside V0 gets the bits 0x7f000000 on top and never wins.  Integer arithmetic alone: no branch, no lane mask per cell.
template <class V>
__host__ __device__ inline int comp_fill_rule(const V& valid, int ix, int iy, int R, int* ddx, int* ddy)
{
    int l = 0, r = 0, u = 0, d = 0;
    for (int a = 1; a <= R; ++a) { l |= valid(ix - a, iy); r |= valid(ix + a, iy); u |= valid(ix, iy - a); d |= valid(ix, iy + a); }
    if (!((l & r) | (u & d))) return 0;
    int best = 0x7fffffff;
    for (int dy = -R; dy <= R; ++dy)
        for (int dx = -R; dx <= R; ++dx) {
            const int cand = ((dx * dx + dy * dy) << 16) | ((dy + COMP_MAX_FILL) << 8) | (dx + COMP_MAX_FILL) | ((valid(ix + dx, iy + dy) - 1) & 0x7f000000);
            best = cand < best ? cand : best;
        }
    *ddx = (best & 0xff) - COMP_MAX_FILL; *ddy = ((best >> 8) & 0xff) - COMP_MAX_FILL;
    return best >> 16;
}

// ---- the score, order and sub-cell rules of the registration ("overlap registration" in the header): ONE body for the host
// (dsss_mosaic_register_peak) and the device (mosaic_peak_kernel), as dsss_rotate_row is for the fan.  Everything in it is an IEEE-754
// basic operation -- 128-bit integer multiply and subtract, integer to the nearest double, * / sqrt + - in f64, unfused
// (-ffp-contract=off) -- so both sides give the same bits.
// exact integer -> the nearest double, ties to even (what Python's float() of an int does): below 2^64 the hardware conversion is that
// already; above, the value is cut to 64 bits with a sticky bit first, which leaves the rounding of the 53-bit result unchanged
__host__ __device__ inline double reg_i128_to_double(__int128 v)
{
    const bool neg = v < 0;
    unsigned __int128 u = neg ? (unsigned __int128)0 - (unsigned __int128)v : (unsigned __int128)v;
    double d;
    if ((u >> 64) == 0) d = (double)(uint64_t)u;
    else {
        const int sh = 64 - __builtin_clzll((uint64_t)(u >> 64));            // bits above the low 64
        const uint64_t top = (uint64_t)(u >> sh);
        const bool sticky = (u & (((unsigned __int128)1 << sh) - 1)) != 0;
        d = ldexp((double)(top | (sticky ? 1ull : 0ull)), sh);
    }
    return neg ? -d : d;
}

struct reg_score { double z; bool ok; };

// one shift's six sums n, Sa, Sb, Sab, Saa, Sbb -> its score; not usable: -2
__host__ __device__ inline reg_score reg_score_of(const uint64_t* s6, int min_cells)
{
    const __int128 n = s6[0], Sa = s6[1], Sb = s6[2], Sab = s6[3], Saa = s6[4], Sbb = s6[5];
    const __int128 num = n * Sab - Sa * Sb, da = n * Saa - Sa * Sa, db = n * Sbb - Sb * Sb;
    if (s6[0] < (uint64_t)min_cells || da <= 0 || db <= 0) return { -2.0, false };
    return { reg_i128_to_double(num) / sqrt(reg_i128_to_double(da) * reg_i128_to_double(db)), true };
}

// the order of the peak among usable shifts: the larger z, then the smaller dx^2 + dy^2, then the smaller dy, then the smaller dx.
// Total: two different shifts are never equal under it, so the winner does not depend on the order they are looked at in.
__host__ __device__ inline bool reg_better(double z, int dx, int dy, double zb, int bx, int by)
{
    const int d2 = dx * dx + dy * dy, b2 = bx * bx + by * by;
    return z > zb || (z == zb && (d2 < b2 || (d2 == b2 && (dy < by || (dy == by && dx < bx)))));
}

// the sub-cell position on one axis: the parabola through the peak z0 and its two neighbours, 0 where one is not usable or the
// denominator is not below 0
__host__ __device__ inline double reg_parabola(const reg_score& m, double z0, const reg_score& p)
{
    if (!m.ok || !p.ok) return 0.0;
    const double den = m.z - 2.0 * z0 + p.z;
    return den < 0.0 ? 0.5 * (m.z - p.z) / den : 0.0;
}

// the record of a table whose peak is known: found = a usable shift exists, (bx, by) = the peak, z0 and n0 = score and cells of the
// zero shift, zp and np = those of the peak, xm, xp, ym, yp = the scores of its four neighbours (read only where the peak is not on
// the border).  Every byte of *out is written.
__host__ __device__ inline void reg_record(bool found, int bx, int by, int radius, double cell, const reg_score& z0, uint64_t n0, const reg_score& zp, uint64_t np,
                                           const reg_score& xm, const reg_score& xp, const reg_score& ym, const reg_score& yp, dsss_reg_result* out)
{
    dsss_reg_result r;
    r.dx = 0; r.dy = 0; r.off_x = 0.0; r.off_y = 0.0; r.zncc = -2.0; r.zncc0 = z0.z; r.n = (int64_t)n0; r.n0 = (int64_t)n0; r.on_border = 0; r.pad_ = 0;
    if (found) {
        r.dx = bx; r.dy = by; r.zncc = zp.z; r.n = (int64_t)np;
        r.on_border = (bx == radius || bx == -radius || by == radius || by == -radius) ? 1 : 0;
        double px = 0.0, py = 0.0;
        if (!r.on_border) { px = reg_parabola(xm, zp.z, xp); py = reg_parabola(ym, zp.z, yp); }
        r.off_x = ((double)bx + px) * cell; r.off_y = ((double)by + py) * cell;
    }
    *out = r;
}

// mosaic_buf in typed, 256-byte aligned pieces: take<T>(count) before reserve, at(piece) after it; the one place an offset of mosaic_buf
// becomes a pointer.  An output layer the caller did not ask for is a piece of no elements: no bytes, and opt(piece) reads it back as
// null.  A piece that comes down behind a correlation launch is taken with take_flagged: the registration's sample-limit flag lies in
// the 8 bytes in front of it, so one copy that starts at flag_of(piece) brings the flag and the payload.
template <class T> struct mosaic_piece { size_t off = 0, count = 0; };
struct mosaic_arena {
    size_t bytes = 0; char* B = nullptr;
    template <class T> mosaic_piece<T> take(size_t count, size_t lead = 0) { const size_t o = bytes + lead; bytes += (lead + count * sizeof(T) + 255) & ~(size_t)255; return { o, count }; }
    template <class T> mosaic_piece<T> take_flagged(size_t count) { return take<T>(count, 256); }
    int reserve(dsss_ctx* c) { const int rc = c->mosaic_buf.reserve(c, bytes); B = c->mosaic_buf.as<char>(); return rc; }
    template <class T> T* at(mosaic_piece<T> p) const { return reinterpret_cast<T*>(B + p.off); }
    template <class T> T* opt(mosaic_piece<T> p) const { return p.count ? at(p) : nullptr; }
    template <class T> int* flag_of(mosaic_piece<T> p) const { return reinterpret_cast<int*>(B + p.off - 8); }
};

// The three layers of a read (sum, cnt, img of `cells` cells each) in the arena, taken before the reserve: a layer whose host pointer
// is null takes no bytes and reads back (opt) as the null device pointer the unpack kernels skip; down() queues the copies of the others.
struct mosaic_layers {
    size_t cells; uint32_t* h_sum; uint32_t* h_cnt; uint8_t* h_img;
    mosaic_piece<uint32_t> o_sum, o_cnt; mosaic_piece<uint8_t> o_img;
    mosaic_layers(mosaic_arena& A, size_t cells_, uint32_t* sum, uint32_t* cnt, uint8_t* img) : cells(cells_), h_sum(sum), h_cnt(cnt), h_img(img),
        o_sum(A.take<uint32_t>(sum ? cells_ : 0)), o_cnt(A.take<uint32_t>(cnt ? cells_ : 0)), o_img(A.take<uint8_t>(img ? cells_ : 0)) {}
    bool any() const { return h_sum || h_cnt || h_img; }
    int down(dsss_ctx* c, const mosaic_arena& A) const {
        if (h_sum) HIPCHK(c, hipMemcpyAsync(h_sum, A.at(o_sum), cells * 4, hipMemcpyDeviceToHost, c->stream));
        if (h_cnt) HIPCHK(c, hipMemcpyAsync(h_cnt, A.at(o_cnt), cells * 4, hipMemcpyDeviceToHost, c->stream));
        if (h_img) HIPCHK(c, hipMemcpyAsync(h_img, A.at(o_img), cells, hipMemcpyDeviceToHost, c->stream));
        return DSSS_OK;
    }
};

int mosaic_check_frames(dsss_ctx* c, const int* ids, int n, const double* rpy6, const int* ping_off, bool need_img, size_t* rows);
int mosaic_check_params(dsss_ctx* c, const dsss_mosaic_params* p);
// the argument rules of every entry that bins samples onto a grid, in the order the error precedence rests on: the frames
// (mosaic_check_frames with their images; *rows = their pings), then the grid, then the range-gain table
int mosaic_check_args(dsss_ctx* c, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params* p, size_t* rows);
// the one rule the footprint entries add, behind mosaic_check_args: *out = the caller's parameters, or the defaults for null, inside
// their ranges, and every listed frame has an even M of at least 4
bool footprint_params_ok(const dsss_footprint_params& F);
int mosaic_check_footprint(dsss_ctx* c, const int* ids, int n, const dsss_footprint_params* fp, dsss_footprint_params* out);
void frame_extent(const dsss_frame& f, const double* rows, double* bb);
void frame_extent_rows(const dsss_frame& f, const double* rows, int r0, int r1, double* bb);      // pings [r0, r1) only
bool cell_range(double lo, double hi, double origin, double cell, int n, int* a, int* b);
mosaic_win mosaic_grid_win(const dsss_mosaic_params* p);      // the grid p with the whole of it as the window: what the mean render and the composite scatter into
// the window of the pings [r0, r1) of a frame on the grid p: the cells their geo extremes, grown by `grow` metres on every side, can
// reach (0: the point samples; 2 max_gap: the sub-samples of a footprint); false: none on the grid, *w untouched
bool mosaic_window(const dsss_frame& f, const double* rows, int r0, int r1, const dsss_mosaic_params* p, mosaic_win* w, double grow = 0.0);
// the sample-limit flag of a finished render copied down, the stream synchronised; set: DSSS_E_CAPACITY with the entry's own message (fmt takes the cell)
int mosaic_flag_down(dsss_ctx* c, const int* d_flag, const char* fmt, double cell);
int upload_rows(dsss_ctx* c, const int* ids, int n, const double* rpy6, const int* ping_off, double* d_rows, std::vector<const double*>& dev_rows);
// the rule of the range-gain table, part of the argument checks of every entry that bins samples (behind mosaic_check_frames, before
// anything is reserved, cleared or launched): a table is set and a listed frame has another M -> DSSS_E_ARG
int mosaic_check_gain(dsss_ctx* c, const int* ids, int n);
// The mosaic_job table of the listed frames as the host keeps it (blk0 = 0), the ONE place a job of the scatter kernels is filled: mosaic_check_gain once
// more (a job never carries a table of another M, whatever the caller checked), then the trajectory rows go up (upload_rows into
// d_rows) and every job gets its rows, geometry, images and the context's table.
int mosaic_fill_jobs(dsss_ctx* c, const int* ids, int n, const double* rpy6, const int* ping_off, double* d_rows, std::vector<mosaic_job>& jobs);
// The one cut of a job table (one workgroup per ping) into launches: jobs [j0, j1) with `blocks` workgroups, at most 2^31 samples a
// launch (sub-samples under fp: max_steps^2 a sample at most), blk0 of every job set.  With the sample limit checked between the launches
// a cell's count stays far below 2^32 until the check sees it, so the packed accumulator cannot wrap unnoticed whatever the number of
// frames.  blocks fits an int: frames have 4 columns or more, so several jobs have 2^29 pings at most, one alone 2^31 - 1 (mosaic_check_frames).
struct mosaic_launch { int j0, j1, blocks; };
template <class JOB> std::vector<mosaic_launch> mosaic_cut_launches(std::vector<JOB>& jobs, const dsss_footprint_params* fp)
{
    const size_t per_sample = fp ? (size_t)fp->max_steps * fp->max_steps : 1;
    const int n = (int)jobs.size(); std::vector<mosaic_launch> out;
    for (int j0 = 0; j0 < n;) {
        int j1 = j0, blocks = 0; size_t samples = 0;
        while (j1 < n) {
            const size_t s = (size_t)jobs[j1].N * jobs[j1].M * per_sample;
            if (j1 > j0 && samples + s > (1ull << 31)) break;
            jobs[j1].blk0 = blocks; blocks += jobs[j1].N; samples += s; ++j1;
        }
        out.push_back({ j0, j1, blocks }); j0 = j1;
    }
    return out;
}
void launch_scatter(dsss_ctx* c, const mosaic_job* d_jobs, int njobs, int blocks, const mosaic_win& G, unsigned long long* acc);
// the accumulators of a render on the grid p (acc: W x H, cleared here) and the unpack into the layers given, null: the sample-limit
// check alone (d_flag, cleared here; mosaic_flag_down reads it); jobs = mosaic_fill_jobs' table, d_jobs = room for it on the device
int mosaic_render_acc(dsss_ctx* c, std::vector<mosaic_job>& jobs, mosaic_job* d_jobs, const dsss_mosaic_params* p,
                      const dsss_footprint_params* fp, unsigned long long* acc, int* d_flag, uint32_t* d_sum, uint32_t* d_cnt, uint8_t* d_img);
// the segmented form for ONE frame (d_job: its record, blk0 = 0; blocks = its pings): ping p goes into d_segs[p / seg_pings]
void launch_scatter_seg(dsss_ctx* c, const mosaic_job* d_job, int blocks, const mosaic_win& G, unsigned long long* acc, const mosaic_seg* d_segs, int seg_pings);

// ---- the registration's host arithmetic (dsss_mosaic_edge.cpp), as far as the orchestration in dsss_mosaic_reg.hip needs it
int peak_of(const uint64_t* sums, int radius, int min_cells, double cell, dsss_reg_result* out);      // one table -> its record: mosaic_peak_kernel's twin
bool fan_ok(int nyaw, double step);
double fan_theta(int k, int nyaw, double step);
void rotate_rows(const double* rows_b, int p0, int p1, double theta, double* out);
void yaw_peak_of(const dsss_reg_result* z, int nyaw, double step, int32_t* k, int32_t* border, double* theta, double* theta_hat);
bool pyr_ok(const dsss_reg_pyr_params& P);
int pyr_min_cells(int min_cells, int level);
void pyr_centre_of(double cell, int level, int cx, int cy, dsss_reg_result* out, int32_t* usable, int32_t* ncx, int32_t* ncy);

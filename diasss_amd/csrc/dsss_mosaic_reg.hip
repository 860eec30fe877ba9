// diasss_amd/csrc/dsss_mosaic_reg.hip -- dense overlap registration of frame pairs (include/dsss.h, section "mosaic", "overlap
// registration").  Every frame of a pair is rendered alone into its window of the grid (mosaic_scatter_kernel, as the consistency map
// does) and kept as one u16 per cell; mosaic_corr_kernel slides frame b over frame a and accumulates, per shift, the six integer sums
// of the zero-normalised cross-correlation.  Score, peak, tie and sub-cell rules are arithmetic on that table, exact in integers up
// to one conversion per quantity, so a result is the same whatever the order of frames, pairs, tiles and atomics; they are written once
// for host and device (dsss_mosaic_int.h): dsss_mosaic_register_peak on the host, mosaic_peak_kernel where the table lies.
// Dense loop closures ("dense loop closures" in the header): the same registration with frame b cut into segments of pings
// (dsss_mosaic_register_segments: one segmented scatter and one pack per frame, the correlation kernel through its job table,
// mosaic_centroid_kernel for where the overlap lies), and a segment's offset as a pose-graph edge (dsss_register_edge, host arithmetic).
// With a yaw fan ("dense loop closures with a yaw fan"): every segment rendered under a fan of small rotations as well
// (mosaic_scatter_fan_kernel: one scatter per frame for all its segments and angles), the correlation once per angle, the angle rule
// on the host (dsss_register_yaw_peak) and an edge that measures the heading too (dsss_register_edge_yaw).
// Over a cell pyramid ("dense loop closures over a cell pyramid"): the segments registered coarse to fine (dsss_mosaic_register_segments_pyr:
// mosaic_pyr_kernel writes the pooled layers of all levels in one pass over a frame's accumulators, the correlation runs once per level
// around each row's centre, the level rule is host arithmetic in one place, dsss_register_pyr_step).
// Peaks on the device ("peaks on the device" in the header): when the caller asks for no sums, the four entries leave the table on
// the device, mosaic_peak_kernel runs behind the correlation, and the records come down with the sample-limit flag in one copy;
// with sums, or under DSSS_REG_PEAKS=host, the table comes down and the host decides, as before.  dsss_mosaic_register_peaks is the
// kernel as a public entry on any tables, dsss_mosaic_register_info what the last call did.
// Where things live: this file holds the seven kernels with their job records and launch helpers, the registration plan -- what the
// four entries share on the host, each concern with one owner: reg_rows (argument rules, rows and where the peaks are decided),
// reg_layers (frame-a windows), reg_mem (the device memory in typed pieces and the place of the sample-limit flag), reg_upload_jobs,
// reg_render_a / reg_render_b, reg_fetch (what follows every correlation launch), reg_centroids, pyr_apply -- and the four entries,
// each a short list over that plan.  The host arithmetic that launches nothing (peak_of, the angle rule, the level rule, edges) is in
// dsss_mosaic_edge.cpp; the rules shared with the device and the declarations are in dsss_mosaic_int.h.
#include "dsss_mosaic_int.h"
#include "dsss_wave.h"
#include <algorithm>

#define REG_TILE 32                        // a workgroup stages 32 x 32 cells of a and the (32 + 2 r)^2 halo of b
#define REG_HALO (REG_TILE + 2 * REG_MAX_RADIUS)
#define REG_STRIP 8                        // tiles (along x) a workgroup walks before it flushes: 8 x 1024 x 255^2 < 2^32, the u32 partials cannot wrap
#define REG_MAX_THREADS 1024
#define REG_SLOTS 2                        // shifts per thread: (2 x 16 + 1)^2 = 1089 <= 2 x 1024
#define CEN_TW 64                          // a workgroup of mosaic_centroid_kernel looks at 64 x 16 cells of a
#define CEN_TH 16

namespace {

// one pair: the two mean layers with their windows (grid cells), the region of a's cells that is walked (a's window cut with b's
// window dilated by the radius) as tiles, blk0 = its first workgroup, and where its sums go
struct reg_job {
    const uint16_t* la; const uint16_t* lb; unsigned long long* out;
    int aox, aoy, abw, abh, box, boy, bbw, bbh;
    int rx0, ry0, rx1, ry1;                // region, inclusive
    int tiles_x, strips_x, blk0, pad;
};

// 64-bit accumulators of one frame's window -> u16 per cell: validity in the high byte, m_f = (sum + cnt / 2) / cnt in the low one
__global__ __launch_bounds__(256) void mosaic_mean_kernel(const unsigned long long* __restrict__ win, size_t n, uint16_t* __restrict__ lay,
                                                          int* __restrict__ flag)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const mosaic_acc a(win[i]);
    if (a.over_limit()) *flag = 1;
    lay[i] = a.c ? (uint16_t)(0x100u | a.mean()) : (uint16_t)0;
}

// ---- the pyramid of mean layers ("dense loop closures over a cell pyramid" in the header)
#define PYR_TW 64                          // a workgroup of mosaic_pyr_kernel owns 64 x 32 fine cells, aligned to 8 = 2^(PYR_MAX_LEVELS - 1) in grid coordinates
#define PYR_TH 32
#define PYR_ROWS 8                         // fine cells one below the other per thread: the vertical partners of every level are its own registers

// one area of a frame (its whole window where it is an a, one segment's window where it is a b): where its accumulators start behind
// the frame's first, its window in fine grid cells, where the u16 layer of each level starts, tiles and blk0 = its first workgroup.
// The window of level l is what the fine window covers: ox_l = ox >> l, bw_l = ((ox + bw - 1) >> l) - ox_l + 1, the same in y.
struct pyr_job {
    unsigned long long acc; unsigned long long lay[PYR_MAX_LEVELS];
    int ox, oy, bw, bh, bx0, by0, tiles_x, blk0;                               // (bx0, by0) = (ox, oy) rounded down to a multiple of 8
};

// one level's cells of a thread: NV values one below the other, pooled over 2^l x 2^l fine cells and equal in the 2^l lanes of a group;
// the first lane of a group writes validity << 8 | m.  (X0, Y0) = the level's cell of the thread's first value, in grid coordinates.
template <int NV> __device__ __forceinline__ void pyr_store(const unsigned long long (&c)[NV], const unsigned long long (&s)[NV], const pyr_job& J, int l,
                                                            int X0, int Y0, bool first, uint16_t* __restrict__ lay)
{
    const int oxl = J.ox >> l, oyl = J.oy >> l, bwl = ((J.ox + J.bw - 1) >> l) - oxl + 1, bhl = ((J.oy + J.bh - 1) >> l) - oyl + 1;
    const int x = X0 - oxl;
    if (!first || x < 0 || x >= bwl) return;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int y = Y0 + j - oyl;
        if (y < 0 || y >= bhl) continue;
        lay[J.lay[l] + (size_t)y * bwl + x] = c[j] ? (uint16_t)(0x100u | (unsigned)((s[j] + c[j] / 2) / c[j])) : (uint16_t)0;
    }
}

// the next level from 2 NV values per thread: the vertical partner is the thread's next value, the horizontal one the lane 2^l away
template <int NV> __device__ __forceinline__ void pyr_down(const unsigned long long (&ci)[2 * NV], const unsigned long long (&si)[2 * NV],
                                                           unsigned long long (&co)[NV], unsigned long long (&so)[NV], int partner)
{
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        unsigned long long c = ci[2 * j] + ci[2 * j + 1], s = si[2 * j] + si[2 * j + 1];
        c += __shfl_xor(c, partner, 64); s += __shfl_xor(s, partner, 64);
        co[j] = c; so[j] = s;
    }
}

// 64-bit accumulators (count high, sum low) of the areas of one frame -> the u16 layers of all `levels` levels in one pass: every
// accumulator is read once (a wavefront reads 64 neighbouring ones of a row), level 0 is mosaic_mean_kernel's value and flag bit for
// bit, and the pooled counts and sums of the levels above are added up in 64 bits in registers (down a thread's eight rows) and by lane
// exchange (across 2, 4, 8 lanes).  Pooling is by grid coordinates: a tile starts on a multiple of 8 whatever the window's origin,
// and cells outside the window read as empty.
__global__ __launch_bounds__(256) void mosaic_pyr_kernel(const pyr_job* __restrict__ jobs, int njobs, int levels, const unsigned long long* __restrict__ acc,
                                                         uint16_t* __restrict__ lay, int* __restrict__ flag)
{
    const pyr_job J = mosaic_job_of(jobs, njobs);
    const int wg = (int)blockIdx.x - J.blk0;
    const int ty = wg / J.tiles_x, tx = wg - ty * J.tiles_x;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int gx = J.bx0 + tx * PYR_TW + lane, gy0 = J.by0 + ty * PYR_TH + wave * PYR_ROWS;            // gy0 is a multiple of 8
    const int x = gx - J.ox;
    const unsigned long long* __restrict__ win = acc + J.acc;
    unsigned long long c0[PYR_ROWS], s0[PYR_ROWS];
    bool over = false;
#pragma unroll
    for (int k = 0; k < PYR_ROWS; ++k) {
        const int y = gy0 + k - J.oy;
        unsigned long long w = 0;
        if (x >= 0 && x < J.bw && y >= 0 && y < J.bh) w = win[(size_t)y * J.bw + x];
        const mosaic_acc a(w);
        over |= a.over_limit();
        c0[k] = a.c; s0[k] = a.s;
        if (x >= 0 && x < J.bw && y >= 0 && y < J.bh) lay[J.lay[0] + (size_t)y * J.bw + x] = a.c ? (uint16_t)(0x100u | a.mean()) : (uint16_t)0;
    }
    if (over) *flag = 1;
    if (levels < 2) return;                                                    // (uniform: no lane leaves before the exchanges it takes part in)
    unsigned long long c1[4], s1[4], c2[2], s2[2], c3[1], s3[1];
    pyr_down<4>(c0, s0, c1, s1, 1);
    pyr_store<4>(c1, s1, J, 1, gx >> 1, gy0 >> 1, (lane & 1) == 0, lay);
    if (levels < 3) return;
    pyr_down<2>(c1, s1, c2, s2, 2);
    pyr_store<2>(c2, s2, J, 2, gx >> 2, gy0 >> 2, (lane & 3) == 0, lay);
    if (levels < 4) return;
    pyr_down<1>(c2, s2, c3, s3, 4);
    pyr_store<1>(c3, s3, J, 3, gx >> 3, gy0 >> 3, (lane & 7) == 0, lay);
}

// One workgroup per strip of REG_STRIP tiles of a's cells.  Per tile the a cells and the halo of b go into LDS as u16 (cells outside a
// window, and with it outside the grid, as 0 = invalid), with one bit per a cell in s_am.  A thread owns up to two shifts (dx fastest,
// so neighbouring lanes read neighbouring half-words of b) and walks the tile for each: the a operand is the same address in every
// lane and goes through a scalar register, rows and groups of eight cells without a valid a cell are skipped by scalar branches, and
// invalid cells inside a group contribute 0 through the validity factors.  The six u32 partials of a shift live in registers over the
// whole strip and leave as 64-bit atomics without return -- integers, so their order is irrelevant -- and only where n > 0.
__global__ __launch_bounds__(REG_MAX_THREADS) void mosaic_corr_kernel(const reg_job* __restrict__ jobs, int njobs, int radius)
{
    __shared__ __attribute__((aligned(16))) uint16_t s_a[REG_TILE * REG_TILE];
    __shared__ __attribute__((aligned(16))) uint16_t s_b[REG_HALO * REG_HALO];
    __shared__ uint32_t s_am[REG_TILE];
    const reg_job J = mosaic_job_of(jobs, njobs);
    const int wg = (int)blockIdx.x - J.blk0;
    const int ty = wg / J.strips_x, tx0 = (wg - ty * J.strips_x) * REG_STRIP;
    const int tx1 = min(tx0 + REG_STRIP, J.tiles_x);
    const int S = 2 * radius + 1, nshift = S * S, hs = REG_TILE + 2 * radius;
    const int nt = (int)blockDim.x, t = (int)threadIdx.x;
    int boff[REG_SLOTS]; bool act[REG_SLOTS];
    uint32_t pn[REG_SLOTS], pa[REG_SLOTS], pb[REG_SLOTS], pab[REG_SLOTS], paa[REG_SLOTS], pbb[REG_SLOTS];
#pragma unroll
    for (int k = 0; k < REG_SLOTS; ++k) {
        const int s = t + k * nt;
        act[k] = s < nshift;
        const int sy = act[k] ? s / S : 0, sx = act[k] ? s - sy * S : 0;     // dy + radius, dx + radius
        boff[k] = sy * hs + sx;
        pn[k] = pa[k] = pb[k] = pab[k] = paa[k] = pbb[k] = 0;
    }
    const int gy0 = J.ry0 + ty * REG_TILE;
    for (int tx = tx0; tx < tx1; ++tx) {
        const int gx0 = J.rx0 + tx * REG_TILE;
        __syncthreads();                                                        // the previous tile has been walked
        for (int i = t; i < REG_TILE * REG_TILE; i += nt) {
            const int y = i >> 5, x = i & 31, gx = gx0 + x, gy = gy0 + y;
            uint16_t v = 0;
            if (gx <= J.rx1 && gy <= J.ry1) v = J.la[(size_t)(gy - J.aoy) * J.abw + (gx - J.aox)];      // the region lies inside a's window
            s_a[i] = v;
            const unsigned long long bal = __ballot(v != 0);                    // 64 cells = two rows of the tile per wavefront
            if ((i & 63) == 0) { s_am[y] = (uint32_t)bal; s_am[y + 1] = (uint32_t)(bal >> 32); }
        }
        for (int i = t; i < hs * hs; i += nt) {
            const int y = i / hs, x = i - y * hs;
            const int bx = gx0 + x - radius - J.box, by = gy0 + y - radius - J.boy;
            s_b[i] = (bx >= 0 && bx < J.bbw && by >= 0 && by < J.bbh) ? J.lb[(size_t)by * J.bbw + bx] : (uint16_t)0;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < REG_SLOTS; ++k) {
            if (!act[k]) continue;
            for (int y = 0; y < REG_TILE; ++y) {
                const uint32_t m = __builtin_amdgcn_readfirstlane(s_am[y]);
                if (!m) continue;
                const uint16_t* brow = s_b + y * hs + boff[k];
                for (int x8 = 0; x8 < REG_TILE; x8 += 8) {
                    if (!((m >> x8) & 0xffu)) continue;
                    const uint4 av = *reinterpret_cast<const uint4*>(&s_a[y * REG_TILE + x8]);
                    const uint32_t aw[4] = { av.x, av.y, av.z, av.w };
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const uint32_t a = __builtin_amdgcn_readfirstlane((aw[j >> 1] >> (16 * (j & 1))) & 0xffffu);
                        const uint32_t va = a >> 8, ma = a & 0xffu;             // an invalid a cell is 0: va = ma = 0
                        const uint32_t b = brow[x8 + j];
                        const uint32_t vb = b >> 8, mb = b & 0xffu;             // an invalid b cell is 0 too
                        pn[k] += vb * va; pa[k] += vb * ma; pb[k] += mb * va;
                        pab[k] += ma * mb; paa[k] += vb * (ma * ma); pbb[k] += (mb * va) * mb;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < REG_SLOTS; ++k) {
        if (!act[k] || pn[k] == 0) continue;                                    // n == 0: the other five are 0 as well
        unsigned long long* o = J.out + (size_t)(t + k * nt) * 6;
        atomicAdd(o + 0, (unsigned long long)pn[k]); atomicAdd(o + 1, (unsigned long long)pa[k]); atomicAdd(o + 2, (unsigned long long)pb[k]);
        atomicAdd(o + 3, (unsigned long long)pab[k]); atomicAdd(o + 4, (unsigned long long)paa[k]); atomicAdd(o + 5, (unsigned long long)pbb[k]);
    }
}

// one (pair, segment) row with a peak: the two layers (windows as in reg_job), the a cells whose cell shifted by the peak (dx, dy) lies
// in b's window as tiles of CEN_TW x CEN_TH, blk0 = its first workgroup, out = n, sum ix, sum iy
struct cen_job {
    const uint16_t* la; const uint16_t* lb; unsigned long long* out;
    int aox, aoy, abw, box, boy, bbw;
    int rx0, ry0, rx1, ry1;                // region, inclusive
    int dx, dy, tiles_x, blk0;
};

// The centroid sums at the peak: n, sum ix, sum iy over the cells where a is valid and b is valid at the shifted cell, ix and iy in
// grid cells.  One workgroup per tile, a thread looks at CEN_TH / 4 cells one below the other (a wavefront reads 64 neighbouring
// half-words of a row), the three sums are added up over the wavefront (dsss_wave_sum) and leave as 64-bit atomics without return,
// only where n > 0.  Integers: the order is irrelevant.  A tile holds 1024 cells with ix, iy < 2^28, so its sums fit 2^38.
__global__ __launch_bounds__(256) void mosaic_centroid_kernel(const cen_job* __restrict__ jobs, int njobs)
{
    const cen_job J = mosaic_job_of(jobs, njobs);
    const int wg = (int)blockIdx.x - J.blk0;
    const int ty = wg / J.tiles_x, tx = wg - ty * J.tiles_x;
    const int gx = J.rx0 + tx * CEN_TW + ((int)threadIdx.x & 63);
    unsigned long long n = 0, sx = 0, sy = 0;
    if (gx <= J.rx1) {
#pragma unroll
        for (int k = 0; k < CEN_TH / 4; ++k) {
            const int gy = J.ry0 + ty * CEN_TH + 4 * k + ((int)threadIdx.x >> 6);
            if (gy > J.ry1) continue;
            const uint16_t a = J.la[(size_t)(gy - J.aoy) * J.abw + (gx - J.aox)];                          // the region lies inside a's window
            const uint16_t b = J.lb[(size_t)(gy + J.dy - J.boy) * J.bbw + (gx + J.dx - J.box)];            // and, shifted, inside b's
            if (a != 0 && b != 0) { n += 1; sx += (unsigned long long)gx; sy += (unsigned long long)gy; }
        }
    }
    n = dsss_wave_sum(n); sx = dsss_wave_sum(sx); sy = dsss_wave_sum(sy);
    if (((int)threadIdx.x & 63) == 0 && n != 0) { atomicAdd(J.out + 0, n); atomicAdd(J.out + 1, sx); atomicAdd(J.out + 2, sy); }
}

// one (segment, angle) of a frame in the fan scatter: the window of the segment's pings rotated by theta about the pivot (cx, cy)
// (bw = 0: no cell of it lies on the grid), where its accumulators start, in cells, behind the frame's first, and s, c = dsss_sincos(theta)
struct mosaic_fan { int ox, oy, bw, bh; unsigned long long off; double cx, cy, theta, s, c; };

// mosaic_scatter_seg_kernel with one more degree of freedom, the angle: a workgroup is a (ping, angle), angles next to each other so
// that the workgroups that read a ping's image row run together.  The entry of (ping / seg_pings, angle) selects window and
// accumulators as a segment does there; the ping's row is rotated into LDS (dsss_rotate_row: the trajectory is never rotated on the
// host and uploaded), the bearings come from the rotated yaw, and the samples are binned by the one body (mosaic_scatter_samples).
// One launch renders every segment of a frame under every angle of the fan.
__global__ __launch_bounds__(256) void mosaic_scatter_fan_kernel(const mosaic_job* __restrict__ job, mosaic_win G, unsigned long long* __restrict__ acc,
                                                                 const mosaic_fan* __restrict__ fan, int seg_pings, int nyaw)
{
    __shared__ double s_sc[4], s_row[2][6];                                        // the rotated row once per side: the two lanes that need it for the bearing write it
    mosaic_job J = *job;
    const int row = (int)(blockIdx.x / (unsigned)nyaw), k = (int)(blockIdx.x - (unsigned)row * (unsigned)nyaw);
    if (row >= J.N) return;                                                        // (uniform per workgroup; cannot happen with the host's grid)
    J.gain = mosaic_gain_row(J, row);                                              // the ping's band, as in mosaic_ping_of
    const mosaic_fan F = fan[(size_t)(row / seg_pings) * nyaw + k];
    if (F.bw <= 0) return;                                                         // nothing of this segment under this angle on the grid (uniform)
    G.ox = F.ox; G.oy = F.oy; G.bw = F.bw; G.bh = F.bh; acc += F.off;
    if (threadIdx.x < 2) {
        dsss_rotate_row(J.pose + (size_t)row * 6, F.cx, F.cy, F.theta, F.s, F.c, s_row[threadIdx.x]);
        dsss_geo_side(s_row[threadIdx.x], threadIdx.x == 1, &s_sc[2 * threadIdx.x], &s_sc[2 * threadIdx.x + 1]);
    }
    __syncthreads();
    mosaic_scatter_samples(s_row[0], s_sc, J, row, G, acc);
}

// ---- peaks on the device ("peaks on the device" in the header)
#define PEAK_WAVES 4                       // tables per workgroup of mosaic_peak_kernel: one wavefront each

// One table of (2 radius + 1)^2 shifts x six sums -> its record, by one wavefront; rec[k] is what peak_of gives for table k, bit for
// bit (the rules are the one body of dsss_mosaic_int.h).  The lanes stride over the shifts (a lane reads the 48 contiguous bytes of a
// shift) and each keeps its best (z, shift) under reg_better; the order is total, so the butterfly over the wavefront ends with the
// same winner in every lane whatever its shape.  The zero shift, the peak and its four neighbours are then scored again by six lanes
// -- a score is a function of six integers, so it has the same bits as in the scan and no table of scores is kept anywhere -- and
// lane 0 writes the 64 bytes.  No atomics, no LDS.  Radius, min_cells and cell are uniform per launch.
__global__ __launch_bounds__(64 * PEAK_WAVES) void mosaic_peak_kernel(const unsigned long long* __restrict__ sums, long long ntables, int radius, int min_cells,
                                                                      double cell, dsss_reg_result* __restrict__ rec)
{
    const int lane = (int)threadIdx.x & 63;
    const long long k = (long long)blockIdx.x * PEAK_WAVES + ((int)threadIdx.x >> 6);
    if (k >= ntables) return;                                                   // (uniform per wavefront)
    const int S = 2 * radius + 1, nshift = S * S;
    const uint64_t* __restrict__ tab = reinterpret_cast<const uint64_t*>(sums) + (size_t)k * nshift * 6;
    int best = -1; double zb = -2.0;                                            // this lane's best shift, -1: none usable so far
    for (int s = lane; s < nshift; s += 64) {
        const reg_score q = reg_score_of(tab + (size_t)s * 6, min_cells);
        if (!q.ok) continue;
        const int sy = s / S, sx = s - sy * S;
        if (best < 0) { best = s; zb = q.z; continue; }
        const int ty = best / S, tx = best - ty * S;
        if (reg_better(q.z, sx - radius, sy - radius, zb, tx - radius, ty - radius)) { best = s; zb = q.z; }
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int ob = __shfl_xor(best, d, 64); const double oz = __shfl_xor(zb, d, 64);
        const int so = max(ob, 0), sb = max(best, 0);
        const int sy = so / S, sx = so - sy * S, ty = sb / S, tx = sb - ty * S;
        if (ob >= 0 && (best < 0 || reg_better(oz, sx - radius, sy - radius, zb, tx - radius, ty - radius))) { best = ob; zb = oz; }
    }
    const bool found = best >= 0;
    const int zero = radius * S + radius, pk = found ? best : zero;
    const int by = pk / S - radius, bx = pk - (pk / S) * S - radius;
    const bool inner = found && bx != radius && bx != -radius && by != radius && by != -radius;      // the four neighbours exist
    // lanes 0..5: the zero shift, the peak, x-, x+, y-, y+
    int t = zero;
    if (lane == 1) t = pk;
    if (inner) { if (lane == 2) t = pk - 1; if (lane == 3) t = pk + 1; if (lane == 4) t = pk - S; if (lane == 5) t = pk + S; }
    reg_score q = { -2.0, false }; unsigned long long nq = 0;
    if (lane < 6) { q = reg_score_of(tab + (size_t)t * 6, min_cells); nq = tab[(size_t)t * 6]; }
    reg_score g[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) { g[j].z = __shfl(q.z, j, 64); g[j].ok = __shfl((int)q.ok, j, 64) != 0; }
    const unsigned long long n0 = __shfl(nq, 0, 64), np = __shfl(nq, 1, 64);
    if (lane == 0) reg_record(found, bx, by, radius, cell, g[0], n0, g[1], np, g[2], g[3], g[4], g[5], rec + k);
}

// the launches of mosaic_peak_kernel over ntables tables, cut where one launch's workgroup count would not fit
int reg_launch_peaks(dsss_ctx* c, const unsigned long long* d_tab, long long ntables, int radius, int min_cells, double cell, dsss_reg_result* d_rec)
{
    const long long per = 0x7fffffffll * PEAK_WAVES;                            // tables of one launch
    const size_t tsz = (size_t)(2 * radius + 1) * (2 * radius + 1) * 6;
    for (long long k0 = 0; k0 < ntables; k0 += per) {
        const long long nt = std::min(per, ntables - k0);
        hipLaunchKernelGGL(mosaic_peak_kernel, dim3((unsigned)((nt + PEAK_WAVES - 1) / PEAK_WAVES)), dim3(64 * PEAK_WAVES), 0, c->stream,
                           d_tab + (size_t)k0 * tsz, nt, radius, min_cells, cell, d_rec + k0);
        HIPCHK(c, hipGetLastError());
    }
    return DSSS_OK;
}

// what a registration call did (dsss_reg_call_info), counted where the call enqueues its copies and synchronises
struct reg_count {
    dsss_reg_call_info I{0, 0, 0, 0};
    void down(size_t bytes) { I.bytes_down += (int64_t)bytes; }
    void sync() { I.syncs += 1; }
};

// ---- what the registration entries share on the host (a frame's window of the grid is mosaic_window, the consistency map's too)
// the job of layer la (window A) against layer lb (window Bw) with its sums at out, appended to pj; *blocks = workgroups so far.
// Windows that do not come within the radius give no job: all sums stay 0.  False: more workgroups than one launch takes.
bool reg_push_job(std::vector<reg_job>& pj, long long* blocks, const uint16_t* la, const mosaic_win& A, const uint16_t* lb, const mosaic_win& Bw,
                  int r, unsigned long long* out)
{
    const int rx0 = std::max(A.ox, Bw.ox - r), rx1 = std::min(A.ox + A.bw - 1, Bw.ox + Bw.bw - 1 + r);
    const int ry0 = std::max(A.oy, Bw.oy - r), ry1 = std::min(A.oy + A.bh - 1, Bw.oy + Bw.bh - 1 + r);
    if (rx1 < rx0 || ry1 < ry0) return true;
    reg_job J;
    J.la = la; J.lb = lb; J.out = out;
    J.aox = A.ox; J.aoy = A.oy; J.abw = A.bw; J.abh = A.bh; J.box = Bw.ox; J.boy = Bw.oy; J.bbw = Bw.bw; J.bbh = Bw.bh;
    J.rx0 = rx0; J.ry0 = ry0; J.rx1 = rx1; J.ry1 = ry1;
    J.tiles_x = (rx1 - rx0) / REG_TILE + 1; J.strips_x = (J.tiles_x + REG_STRIP - 1) / REG_STRIP;
    J.blk0 = (int)*blocks; J.pad = 0;
    *blocks += (long long)J.strips_x * ((ry1 - ry0) / REG_TILE + 1);
    if (*blocks > 0x7fffffffll) return false;
    pj.push_back(J);
    return true;
}

// all jobs in one launch
int reg_launch_corr(dsss_ctx* c, const std::vector<reg_job>& pj, long long blocks, reg_job* d_pairs, int r)
{
    if (pj.empty()) return DSSS_OK;
    const int nshift = (2 * r + 1) * (2 * r + 1);
    const int slots = (nshift + REG_MAX_THREADS - 1) / REG_MAX_THREADS;        // 1, or 2 from radius 16 on
    const int threads = (((nshift + slots - 1) / slots) + 63) & ~63;
    HIPCHK(c, hipMemcpyAsync(d_pairs, pj.data(), pj.size() * sizeof(reg_job), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(mosaic_corr_kernel, dim3((unsigned)blocks), dim3((unsigned)threads), 0, c->stream, d_pairs, (int)pj.size(), r);
    HIPCHK(c, hipGetLastError());
    return DSSS_OK;
}

// the centroid job of a row with the peak q (layers and windows as in reg_push_job), its sums at out, appended to cj; *blocks =
// workgroups so far.  False: more workgroups than one launch takes.
bool cen_push_job(std::vector<cen_job>& cj, long long* blocks, const uint16_t* la, const mosaic_win& A, const uint16_t* lb, const mosaic_win& Bw,
                  const dsss_reg_result& q, unsigned long long* out)
{
    cen_job J;
    J.la = la; J.lb = lb; J.out = out;
    J.aox = A.ox; J.aoy = A.oy; J.abw = A.bw; J.box = Bw.ox; J.boy = Bw.oy; J.bbw = Bw.bw;
    J.rx0 = std::max(A.ox, Bw.ox - q.dx); J.rx1 = std::min(A.ox + A.bw - 1, Bw.ox + Bw.bw - 1 - q.dx);
    J.ry0 = std::max(A.oy, Bw.oy - q.dy); J.ry1 = std::min(A.oy + A.bh - 1, Bw.oy + Bw.bh - 1 - q.dy);
    if (J.rx1 < J.rx0 || J.ry1 < J.ry0) return true;                            // (cannot be: a usable shift has cells; the callers' check of n reports it)
    J.dx = q.dx; J.dy = q.dy; J.tiles_x = (J.rx1 - J.rx0) / CEN_TW + 1; J.blk0 = (int)*blocks;
    *blocks += (long long)J.tiles_x * ((J.ry1 - J.ry0) / CEN_TH + 1);
    if (*blocks > 0x7fffffffll) return false;
    cj.push_back(J);
    return true;
}

// ---- the registration plan: what the four entries share on the host, each concern written once

// cells of a layer, or of a window's accumulators, rounded up so that the next one starts on 256 bytes
inline size_t reg_round(size_t cells) { return (cells + 127) & ~(size_t)127; }
// the 64-bit sums of one table
inline size_t reg_table_words(int r) { return (size_t)(2 * r + 1) * (2 * r + 1) * 6; }
// the grid without a window: what the segmented scatters take, and what a segment keeps that has no cell on the grid (bw = 0)
inline mosaic_win reg_grid(const dsss_mosaic_params* p) { mosaic_win w = mosaic_grid_win(p); w.bw = w.bh = 0; return w; }

// What the argument rules establish: the parameters in force, the frames' places in ids, which frames occur as a and as b, where the
// peaks are decided, and for the segment entries the rows -- by pair and then by segment of the pair's frame b.
struct reg_rows {
    dsss_ctx* c = nullptr; const int* ids = nullptr; const double* rpy6 = nullptr; const int* ping_off = nullptr;
    const int* pair_a = nullptr; const int* pair_b = nullptr;
    int n = 0, npairs = 0, seg_pings = 1, nseg = 0;
    dsss_reg_params R; std::vector<int> slot; size_t traj_rows = 0;            // slot: frame id -> its index in ids; traj_rows = pings of all frames
    bool dev = false;                                                           // the peaks on the device: nobody reads the table on the host
    std::vector<char> as_a, as_b;
    std::vector<int> row_a, row_b; std::vector<size_t> row_g;                   // a row's frames (index in ids) and its segment's first entry in the entry's window list

    const dsss_frame& frame(int i) const { return c->frames[ids[i]]; }
    const double* rows_of(int i) const { return rpy6 ? rpy6 + (size_t)ping_off[i] * 6 : frame(i).h_geo; }
    int segs_of(int i) const { return (int)(((long long)frame(i).N + seg_pings - 1) / seg_pings); }
    int seg_end(int s, int N) const { return (int)std::min((long long)(s + 1) * seg_pings, (long long)N); }

    // the argument rules of all four entries
    int check(dsss_ctx* ctx, const int* ids_, int n_, const double* rpy6_, const int* ping_off_, const dsss_mosaic_params* p, const int* pa, const int* pb,
              int npairs_, const dsss_reg_params* rp, const void* out_host)
    {
        c = ctx; ids = ids_; n = n_; rpy6 = rpy6_; ping_off = ping_off_; pair_a = pa; pair_b = pb; npairs = npairs_;
        if (dsss_comm_world(c) > 1) DSSS_FAIL(c, DSSS_E_STATE, "mosaic: registration runs on a single rank (communicator of %d)", dsss_comm_world(c));
        const int rc = mosaic_check_args(c, ids, n, rpy6, ping_off, p, &traj_rows); if (rc) return rc;
        dsss_reg_params_default(&R);
        if (rp) R = *rp;
        if (R.radius < 0 || R.radius > REG_MAX_RADIUS) DSSS_FAIL(c, DSSS_E_ARG, "register: radius %d outside 0..%d", R.radius, REG_MAX_RADIUS);
        if (R.min_cells < 1) DSSS_FAIL(c, DSSS_E_ARG, "register: min_cells = %d", R.min_cells);
        if (npairs < 0) DSSS_FAIL(c, DSSS_E_ARG, "register: npairs = %d", npairs);
        if (npairs > 0 && (!pair_a || !pair_b || !out_host)) DSSS_FAIL(c, DSSS_E_ARG, "register: %d pairs without %s", npairs, out_host ? "their frames" : "a result array");
        slot.assign(c->max_frames, -1);
        for (int i = 0; i < n; ++i) slot[ids[i]] = i;
        for (int k = 0; k < npairs; ++k) {
            const int a = pair_a[k], b = pair_b[k];
            if (a < 0 || a >= c->max_frames || slot[a] < 0 || b < 0 || b >= c->max_frames || slot[b] < 0)
                DSSS_FAIL(c, DSSS_E_ARG, "register: pair %d = (%d, %d) names a frame that is not listed", k, a, b);
            if (a == b) DSSS_FAIL(c, DSSS_E_ARG, "register: pair %d is frame %d with itself", k, a);
        }
        return DSSS_OK;
    }
    // ... and those of the segment entries
    int check_segments(int seg_pings_, const int* nseg_host, int cap)
    {
        if (seg_pings_ < 1) DSSS_FAIL(c, DSSS_E_ARG, "register: seg_pings = %d", seg_pings_);
        if (!nseg_host || cap < 0) DSSS_FAIL(c, DSSS_E_ARG, "register: %s", nseg_host ? "negative capacity" : "nowhere to write the number of segments");
        seg_pings = seg_pings_;
        return DSSS_OK;
    }
    // which frames occur as what, and the path: the switch is read here, once per call
    void mark(const uint64_t* sums_host)
    {
        dev = !sums_host && !dsss_switches_read().reg_peaks_host;
        as_a.assign(n, 0); as_b.assign(n, 0);
        for (int k = 0; k < npairs; ++k) { as_a[slot[pair_a[k]]] = 1; as_b[slot[pair_b[k]]] = 1; }
    }
    // the number of rows (a ping of frame b takes nyaw workgroups of its scatter); nseg = 0: nothing to do
    int count(int nyaw, int cap, int* nseg_host, const uint64_t* sums_host)
    {
        long long total = 0;
        for (int k = 0; k < npairs; ++k) {
            const int ib = slot[pair_b[k]];
            if ((long long)frame(ib).N * nyaw > 0x7fffffffll) DSSS_FAIL(c, DSSS_E_ARG, "register: frame %d has %d pings, too many for %d angles in one launch", ids[ib], frame(ib).N, nyaw);
            total += segs_of(ib);
        }
        if (total > 0x7fffffffll) DSSS_FAIL(c, DSSS_E_ARG, "register: %lld segments", total);
        *nseg_host = (int)total;                                                // also when there is no room for them: the caller learns how many
        if (total > cap) DSSS_FAIL(c, DSSS_E_CAPACITY, "register: %lld segments, room for %d", total, cap);
        nseg = (int)total;
        if (nseg) mark(sums_host);
        return DSSS_OK;
    }
    // the rows laid out: the header of row `row` goes to seg_of(row); segment s of frame b is entry first[ib] + s * per of the window list
    template <class SegOf> void layout(const std::vector<size_t>& first, int per, SegOf seg_of)
    {
        row_a.resize(nseg); row_b.resize(nseg); row_g.resize(nseg);
        int row = 0;
        for (int k = 0; k < npairs; ++k) {
            const int ia = slot[pair_a[k]], ib = slot[pair_b[k]];
            for (int s = 0; s < segs_of(ib); ++s, ++row) {
                dsss_reg_seg& o = seg_of(row);
                o.pair = k; o.seg = s; o.p0 = s * seg_pings; o.p1 = seg_end(s, frame(ib).N);
                row_a[row] = ia; row_b[row] = ib; row_g[row] = first[ib] + (size_t)s * per;
            }
        }
    }
};

// The frames as an a: the window of the cells a frame's geo extremes can reach (as the consistency map's) and where its u16 layer
// starts; win_cells = the accumulators the largest render needs, lay_cells = the cells of all layers laid out so far.
struct reg_layers {
    std::vector<mosaic_win> wins; std::vector<char> on_grid; std::vector<size_t> lay_off;
    size_t win_cells = 1, lay_cells = 0;
    explicit reg_layers(int n) : wins(n), on_grid(n, 0), lay_off(n, 0) {}
    void add_a(const reg_rows& Q, int i, const dsss_mosaic_params* p)
    {
        const dsss_frame& f = Q.frame(i);
        if (!mosaic_window(f, Q.rows_of(i), 0, f.N, p, &wins[i])) return;
        on_grid[i] = 1;
        const size_t wc = (size_t)wins[i].bw * wins[i].bh;
        win_cells = std::max(win_cells, wc);
        lay_off[i] = lay_cells; lay_cells += reg_round(wc);
    }
    // the layers of a frame's segments as b: `cells` accumulators, one window behind the other -> where their layers start
    size_t add_b(size_t cells) { win_cells = std::max(win_cells, cells); const size_t o = lay_cells; lay_cells += cells; return o; }
};

// The device memory of a registration call: the pieces every entry needs, out of the family's arena (an entry's own go through A
// between take and reserve).  tab = the sums of one pass, rec = its records on the device path, flag = the sample-limit flag in front
// of whichever comes down (take_flagged / flag_of: the one place the flag's position is decided).
struct reg_mem {
    mosaic_arena A; bool dev = false;
    uint16_t* lay = nullptr; unsigned long long* win = nullptr; mosaic_job* jobs = nullptr; double* rows = nullptr; reg_job* pairs = nullptr;
    cen_job* cj = nullptr; unsigned long long* cen = nullptr; unsigned long long* tab = nullptr; dsss_reg_result* rec = nullptr; int* flag = nullptr;
    mosaic_piece<uint16_t> o_lay; mosaic_piece<unsigned long long> o_win, o_cen, o_tab; mosaic_piece<mosaic_job> o_jobs; mosaic_piece<double> o_rows;
    mosaic_piece<reg_job> o_pairs; mosaic_piece<cen_job> o_cj; mosaic_piece<dsss_reg_result> o_rec;

    // n frames, traj_rows pings of a caller's trajectory (0: the frames' own), nrows tables of at most table_words sums in all per pass
    void take(size_t lay_cells, size_t win_cells, int n, size_t traj_rows, size_t nrows, bool centroids, size_t table_words, bool on_device)
    {
        dev = on_device;
        o_lay = A.take<uint16_t>(lay_cells); o_win = A.take<unsigned long long>(win_cells); o_jobs = A.take<mosaic_job>(n);
        o_rows = A.take<double>(traj_rows * 6); o_pairs = A.take<reg_job>(nrows);
        o_cj = A.take<cen_job>(centroids ? nrows : 0); o_cen = A.take<unsigned long long>(centroids ? nrows * 3 : 0);
        o_tab = A.take_flagged<unsigned long long>(table_words); o_rec = A.take_flagged<dsss_reg_result>(dev ? nrows : 0);
    }
    int reserve(dsss_ctx* c)
    {
        const int rc = A.reserve(c); if (rc) return rc;
        lay = A.at(o_lay); win = A.at(o_win); jobs = A.at(o_jobs); rows = A.at(o_rows); pairs = A.at(o_pairs); cj = A.at(o_cj); cen = A.at(o_cen);
        tab = A.at(o_tab); rec = A.at(o_rec); flag = dev ? A.flag_of(o_rec) : A.flag_of(o_tab);
        return DSSS_OK;
    }
    // what one copy brings down behind a pass of ntab tables of tsz sums: the flag and the records, or the flag and the tables
    size_t down_bytes(size_t ntab, size_t tsz) const { return 8 + (dev ? ntab * sizeof(dsss_reg_result) : ntab * tsz * 8); }
    // the flag and `words` sums cleared: one memset where the flag lies in front of the table, two where it lies in front of the records
    int clear_both(dsss_ctx* c, size_t words) const
    {
        if (!dev) { HIPCHK(c, hipMemsetAsync(flag, 0, 8 + words * 8, c->stream)); return DSSS_OK; }
        HIPCHK(c, hipMemsetAsync(tab, 0, words * 8, c->stream));
        HIPCHK(c, hipMemsetAsync(flag, 0, 8, c->stream));
        return DSSS_OK;
    }
};

// the trajectory rows and the mosaic_job table of the frames go up; jobs = the table as the host keeps it
int reg_upload_jobs(const reg_rows& Q, const reg_mem& M, std::vector<mosaic_job>& jobs)
{
    dsss_ctx* c = Q.c;
    const int rc = mosaic_fill_jobs(c, Q.ids, Q.n, Q.rpy6, Q.ping_off, M.rows, jobs); if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(M.jobs, jobs.data(), (size_t)Q.n * sizeof(mosaic_job), hipMemcpyHostToDevice, c->stream));
    return DSSS_OK;
}

// wc accumulators of M.win -> the u16 layer at lay_off, with the sample-limit flag: the one launch of mosaic_mean_kernel
int reg_pack(dsss_ctx* c, const reg_mem& M, size_t wc, size_t lay_off)
{
    hipLaunchKernelGGL(mosaic_mean_kernel, dim3((unsigned)((wc + 255) / 256)), dim3(256), 0, c->stream, M.win, wc, M.lay + lay_off, M.flag);
    HIPCHK(c, hipGetLastError());
    return DSSS_OK;
}

// frame i as an a: scatter into the 64-bit window, pack into the frame's resident u16 layer
int reg_render_a(dsss_ctx* c, const reg_mem& M, const reg_layers& W, int i, int pings)
{
    const size_t wc = (size_t)W.wins[i].bw * W.wins[i].bh;
    HIPCHK(c, hipMemsetAsync(M.win, 0, wc * 8, c->stream));
    launch_scatter(c, M.jobs + i, 1, pings, W.wins[i], M.win);
    return reg_pack(c, M, wc, W.lay_off[i]);
}

// all segments of a frame as b, their windows one behind the other in `cells` accumulators: ONE scatter (the entry's) and ONE pack
template <class Scatter> int reg_render_b(dsss_ctx* c, const reg_mem& M, size_t cells, size_t lay_off, Scatter scatter)
{
    HIPCHK(c, hipMemsetAsync(M.win, 0, cells * 8, c->stream));
    scatter();
    return reg_pack(c, M, cells, lay_off);
}

// one correlation launch's radius, min_cells and cell: uniform over its tables
struct reg_pass { int radius, min_cells; double cell; };

// what reg_fetch brought down, read by index: a record on either path (the device's, or decided here from the table), a table on the host path
struct reg_view {
    bool dev; const dsss_reg_result* rec; const uint64_t* tab; size_t tsz; reg_pass P;
    dsss_reg_result record(size_t k) const
    {
        if (dev) return rec[k];
        dsss_reg_result q; peak_of(tab + k * tsz, P.radius, P.min_cells, P.cell, &q);
        return q;
    }
    const uint64_t* table(size_t k) const { return tab + k * tsz; }
};

// The step behind every correlation launch over ntab tables: on the device path mosaic_peak_kernel, then ONE copy of the flag and
// the records (or the tables) to `land`, ONE synchronisation, the bookkeeping (`decided` tables count as decided) and the flag.
int reg_fetch(dsss_ctx* c, const reg_mem& M, size_t ntab, size_t decided, const reg_pass& P, double grid_cell, void* land, reg_count& cnt, reg_view* v)
{
    const size_t tsz = reg_table_words(P.radius), down = M.down_bytes(ntab, tsz);
    if (M.dev) { const int rc = reg_launch_peaks(c, M.tab, (long long)ntab, P.radius, P.min_cells, P.cell, M.rec); if (rc) return rc; }
    HIPCHK(c, hipMemcpyAsync(land, M.flag, down, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    cnt.down(down); cnt.sync();
    if (*static_cast<const int*>(land)) DSSS_FAIL(c, DSSS_E_CAPACITY, "mosaic: a cell received more than 2^24 samples of one frame (cell %g too coarse)", grid_cell);
    (M.dev ? cnt.I.tables_device : cnt.I.tables_host) += (int64_t)decided;
    const char* payload = static_cast<const char*>(land) + 8;
    *v = reg_view{ M.dev, reinterpret_cast<const dsss_reg_result*>(payload), reinterpret_cast<const uint64_t*>(payload), tsz, P };
    return DSSS_OK;
}

// a row that gets a centroid: its two layers with their windows, and the row, whose record holds the peak
struct cen_src { const uint16_t* la; const mosaic_win* A; const uint16_t* lb; const mosaic_win* Bw; dsss_reg_seg* o; };

// The centroid sums of the rows that have a peak: row_of(row, &src) says which (false: the row keeps sx = sy = 0).  One launch, one
// download, n held against the record's, sx and sy written.  bounded: the entry has bounded the workgroups before it launched anything.
template <class RowOf> int reg_centroids(dsss_ctx* c, const reg_mem& M, int nseg, bool bounded, reg_count& cnt, RowOf row_of)
{
    std::vector<cen_job> cj; std::vector<dsss_reg_seg*> into(nseg, nullptr);
    long long cblocks = 0;
    for (int row = 0; row < nseg; ++row) {
        cen_src s;
        if (!row_of(row, &s)) continue;
        into[row] = s.o;
        if (cen_push_job(cj, &cblocks, s.la, *s.A, s.lb, *s.Bw, s.o->r, M.cen + (size_t)row * 3)) continue;
        if (bounded) DSSS_FAIL(c, DSSS_E_NUMERIC, "register: internal error, the centroid of %d segments takes more workgroups than was bounded", nseg);
        DSSS_FAIL(c, DSSS_E_ARG, "register: %d segments are more than one launch takes", nseg);
    }
    if (cj.empty()) return DSSS_OK;
    std::vector<uint64_t> cen((size_t)nseg * 3);
    HIPCHK(c, hipMemcpyAsync(M.cj, cj.data(), cj.size() * sizeof(cen_job), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(mosaic_centroid_kernel, dim3((unsigned)cblocks), dim3(256), 0, c->stream, M.cj, (int)cj.size());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(cen.data(), M.cen, cen.size() * 8, hipMemcpyDeviceToHost, c->stream));      // (M.cen was cleared before the first launch)
    HIPCHK(c, hipStreamSynchronize(c->stream));
    cnt.down(cen.size() * 8); cnt.sync();
    for (int row = 0; row < nseg; ++row) {
        dsss_reg_seg* o = into[row];
        if (!o) continue;
        if ((int64_t)cen[(size_t)row * 3] != o->r.n)
            DSSS_FAIL(c, DSSS_E_NUMERIC, "register: internal error, row %d has %lld cells at its peak and %lld in its centroid", row,
                      (long long)o->r.n, (long long)cen[(size_t)row * 3]);
        o->sx = (int64_t)cen[(size_t)row * 3 + 1]; o->sy = (int64_t)cen[(size_t)row * 3 + 2];
    }
    return DSSS_OK;
}

// ---- the cell pyramid
// the window of level l that the fine window w covers (only ox, oy, bw, bh differ), moved by (-cx, -cy)
mosaic_win pyr_window(const mosaic_win& w, int l, int cx, int cy)
{
    mosaic_win q = w;
    q.ox = w.ox >> l; q.oy = w.oy >> l;
    q.bw = ((w.ox + w.bw - 1) >> l) - q.ox + 1; q.bh = ((w.oy + w.bh - 1) >> l) - q.oy + 1;
    q.ox -= cx; q.oy -= cy;
    return q;
}

// A row after level l, q = the level's record with the centre added (pyr_centre_of).  Not usable: the row dies, and no level having a
// usable peak leaves the top level's record; otherwise the level, its shift, score and border bit, and (nx, ny) = the centre below.
void pyr_apply(dsss_reg_seg_pyr& o, const dsss_reg_result& q, bool usable, int l, bool top, int32_t nx, int32_t ny, char* alive, int32_t* cx, int32_t* cy)
{
    if (!usable) { *alive = 0; if (top) o.s.r = q; return; }
    o.s.r = q; o.level = l; o.lx[l] = q.dx; o.ly[l] = q.dy; o.lz[l] = q.zncc;
    if (q.on_border) o.border_mask |= 1 << l;
    *cx = nx; *cy = ny;
}

} // namespace

extern "C" {

int dsss_mosaic_register(dsss_ctx* c, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params* p,
                         const int* pair_a, const int* pair_b, int npairs, const dsss_reg_params* rp,
                         dsss_reg_result* out_host, uint64_t* sums_host)
{
    if (!c) return DSSS_E_ARG;
    reg_rows Q;
    int rc = Q.check(c, ids, n, rpy6, ping_off, p, pair_a, pair_b, npairs, rp, out_host); if (rc) return rc;
    reg_count cnt;
    if (npairs == 0) { c->reg_info = cnt.I; return DSSS_OK; }
    Q.mark(sums_host);
    HIPCHK(c, hipSetDevice(c->device));
    const reg_pass P{ Q.R.radius, Q.R.min_cells, p->cell };
    const size_t tsz = reg_table_words(P.radius), table = (size_t)npairs * tsz;
    reg_layers W(n);                                                            // every frame that occurs in a pair is rendered whole
    for (int i = 0; i < n; ++i) if (Q.as_a[i] || Q.as_b[i]) W.add_a(Q, i, p);
    reg_mem M;
    M.take(W.lay_cells, W.win_cells, n, rpy6 ? Q.traj_rows : 0, npairs, false, table, Q.dev);
    rc = M.reserve(c); if (rc) return rc;
    if (Q.dev) { rc = c->mosaic_pinned.reserve(c, M.down_bytes(npairs, tsz)); if (rc) return rc; }
    std::vector<mosaic_job> jobs;
    rc = reg_upload_jobs(Q, M, jobs); if (rc) return rc;
    rc = M.clear_both(c, table); if (rc) return rc;
    // 1. mean layers
    for (int i = 0; i < n; ++i) if (W.on_grid[i]) { rc = reg_render_a(c, M, W, i, jobs[i].N); if (rc) return rc; }
    // 2. all pairs in one launch
    std::vector<reg_job> pj; pj.reserve(npairs);
    long long blocks = 0;
    for (int k = 0; k < npairs; ++k) {
        const int ia = Q.slot[pair_a[k]], ib = Q.slot[pair_b[k]];
        if (!W.on_grid[ia] || !W.on_grid[ib]) continue;
        if (!reg_push_job(pj, &blocks, M.lay + W.lay_off[ia], W.wins[ia], M.lay + W.lay_off[ib], W.wins[ib], P.radius, M.tab + (size_t)k * tsz))
            DSSS_FAIL(c, DSSS_E_ARG, "register: %d pairs are more than one launch takes", npairs);
    }
    rc = reg_launch_corr(c, pj, blocks, M.pairs, P.radius); if (rc) return rc;
    // 3. the records come down into the page-locked area; a table of the whole-frame form (138 MB-class) into pageable memory of this call
    std::vector<uint64_t> own;
    if (!Q.dev) own.resize(1 + table);
    reg_view v;
    rc = reg_fetch(c, M, npairs, npairs, P, p->cell, Q.dev ? c->mosaic_pinned.p : (void*)own.data(), cnt, &v); if (rc) return rc;
    for (int k = 0; k < npairs; ++k) out_host[k] = v.record(k);
    if (sums_host) memcpy(sums_host, v.table(0), table * 8);
    c->reg_info = cnt.I;
    return DSSS_OK;
}

// The segments of frame b against the whole of frame a.  Per frame that occurs as b: ONE segmented scatter into the accumulators of all
// its segments (each segment its own window, one behind the other) and ONE mosaic_mean_kernel over that whole area, whatever the number
// of segments and of pairs that name the frame; the layers use the accumulators' offsets, so the pack needs no segment table.  The
// correlation is mosaic_corr_kernel with one job per (pair, segment); the peaks are decided by mosaic_peak_kernel behind it (on the
// host when the sums are asked for), then mosaic_centroid_kernel runs once over the rows that have one.
int dsss_mosaic_register_segments(dsss_ctx* c, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params* p,
                                  const int* pair_a, const int* pair_b, int npairs, int seg_pings, const dsss_reg_params* rp,
                                  dsss_reg_seg* out_host, int cap, int* nseg_host, uint64_t* sums_host)
{
    if (!c) return DSSS_E_ARG;
    reg_rows Q;
    int rc = Q.check(c, ids, n, rpy6, ping_off, p, pair_a, pair_b, npairs, rp, out_host); if (rc) return rc;
    rc = Q.check_segments(seg_pings, nseg_host, cap); if (rc) return rc;
    rc = Q.count(1, cap, nseg_host, sums_host); if (rc) return rc;
    reg_count cnt;
    if (Q.nseg == 0) { c->reg_info = cnt.I; return DSSS_OK; }
    const int nseg = Q.nseg;
    HIPCHK(c, hipSetDevice(c->device));
    const reg_pass P{ Q.R.radius, Q.R.min_cells, p->cell };
    const size_t tsz = reg_table_words(P.radius), table = (size_t)nseg * tsz;
    // windows: the whole frame where it occurs as a, every segment where it occurs as b
    reg_layers W(n);
    std::vector<size_t> seg0(n, 0), seg_lay(n, 0), seg_cells(n, 0);             // a frame's first segment in sw / hseg, its segments' layers and accumulators
    std::vector<mosaic_win> sw; std::vector<mosaic_seg> hseg;
    for (int i = 0; i < n; ++i) {
        if (Q.as_a[i]) W.add_a(Q, i, p);
        if (!Q.as_b[i]) continue;
        const dsss_frame& f = Q.frame(i);
        seg0[i] = sw.size();
        size_t cells = 0;
        for (int s = 0; s < Q.segs_of(i); ++s) {
            mosaic_win w = reg_grid(p);
            mosaic_window(f, Q.rows_of(i), s * seg_pings, Q.seg_end(s, f.N), p, &w);
            sw.push_back(w); hseg.push_back(mosaic_seg{ w.ox, w.oy, w.bw, w.bh, (unsigned long long)cells });
            cells += reg_round((size_t)w.bw * w.bh);
        }
        seg_cells[i] = cells; seg_lay[i] = W.add_b(cells);
    }
    reg_mem M;
    M.take(W.lay_cells, W.win_cells, n, rpy6 ? Q.traj_rows : 0, nseg, true, table, Q.dev);
    const mosaic_piece<mosaic_seg> o_segs = M.A.take<mosaic_seg>(hseg.size());
    rc = M.reserve(c); if (rc) return rc;
    rc = c->mosaic_pinned.reserve(c, M.down_bytes(nseg, tsz)); if (rc) return rc;
    mosaic_seg* d_segs = M.A.at(o_segs);
    std::vector<mosaic_job> jobs;
    rc = reg_upload_jobs(Q, M, jobs); if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(d_segs, hseg.data(), hseg.size() * sizeof(mosaic_seg), hipMemcpyHostToDevice, c->stream));
    rc = M.clear_both(c, table); if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(M.cen, 0, (size_t)nseg * 3 * 8, c->stream));
    // 1. mean layers: a frame's whole layer where it is an a, the layers of all its segments (one scatter, one pack) where it is a b
    const mosaic_win grid = reg_grid(p);
    for (int i = 0; i < n; ++i) {
        if (W.on_grid[i]) { rc = reg_render_a(c, M, W, i, jobs[i].N); if (rc) return rc; }
        if (Q.as_b[i] && seg_cells[i]) {
            rc = reg_render_b(c, M, seg_cells[i], seg_lay[i], [&] { launch_scatter_seg(c, M.jobs + i, jobs[i].N, grid, M.win, d_segs + seg0[i], seg_pings); });
            if (rc) return rc;
        }
    }
    // 2. one correlation job per row, all in one launch
    memset(out_host, 0, (size_t)nseg * sizeof(dsss_reg_seg));
    Q.layout(seg0, 1, [&](int row) -> dsss_reg_seg& { return out_host[row]; });
    auto layer_b = [&](int row) { return M.lay + seg_lay[Q.row_b[row]] + hseg[Q.row_g[row]].off; };
    std::vector<reg_job> pj; pj.reserve(nseg);
    long long blocks = 0;
    for (int row = 0; row < nseg; ++row) {
        const int ia = Q.row_a[row]; const size_t g = Q.row_g[row];
        if (!W.on_grid[ia] || sw[g].bw == 0) continue;
        if (!reg_push_job(pj, &blocks, M.lay + W.lay_off[ia], W.wins[ia], layer_b(row), sw[g], P.radius, M.tab + (size_t)row * tsz))
            DSSS_FAIL(c, DSSS_E_ARG, "register: %d segments are more than one launch takes", nseg);
    }
    rc = reg_launch_corr(c, pj, blocks, M.pairs, P.radius); if (rc) return rc;
    reg_view v;
    rc = reg_fetch(c, M, nseg, nseg, P, p->cell, c->mosaic_pinned.p, cnt, &v); if (rc) return rc;
    // 3. the peaks, then the centroid sums of the rows that have one
    for (int row = 0; row < nseg; ++row) out_host[row].r = v.record(row);
    rc = reg_centroids(c, M, nseg, false, cnt, [&](int row, cen_src* s) {
        if (!(out_host[row].r.zncc > -2.0)) return false;                       // no usable shift: sx = sy = 0
        *s = cen_src{ M.lay + W.lay_off[Q.row_a[row]], &W.wins[Q.row_a[row]], layer_b(row), &sw[Q.row_g[row]], &out_host[row] };
        return true; });
    if (rc) return rc;
    if (sums_host) memcpy(sums_host, v.table(0), table * 8);
    c->reg_info = cnt.I;
    return DSSS_OK;
}

// dsss_mosaic_register_segments under every angle of the fan.  Per frame that occurs as b: ONE memset, ONE mosaic_scatter_fan_kernel into
// the accumulators of all its (segment, angle) windows and ONE mosaic_mean_kernel over that whole area; the windows of the rotated
// segments come from the host's twin of the kernel's rotation (rotate_rows -> dsss_rotate_row).  The correlation runs in PASSES, one
// per angle, each mosaic_corr_kernel with one job per (pair, segment) and one download: of that angle's records (mosaic_peak_kernel),
// or, when the sums are asked for, of a table of ONE angle's size, whose peaks the host decides -- the page-locked landing area stays
// what the translation-only call needs instead of nyaw times that.  The angle rule is the host's on both paths.  The centroid runs
// once, for the chosen angle of every row.
int dsss_mosaic_register_segments_yaw(dsss_ctx* c, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params* p,
                                      const int* pair_a, const int* pair_b, int npairs, int seg_pings, const dsss_reg_params* rp,
                                      const dsss_reg_yaw_params* yp, dsss_reg_seg_yaw* out_host, int cap, int* nseg_host, uint64_t* sums_host)
{
    if (!c) return DSSS_E_ARG;
    reg_rows Q;
    int rc = Q.check(c, ids, n, rpy6, ping_off, p, pair_a, pair_b, npairs, rp, out_host); if (rc) return rc;
    rc = Q.check_segments(seg_pings, nseg_host, cap); if (rc) return rc;
    dsss_reg_yaw_params Y; dsss_reg_yaw_params_default(&Y);
    if (yp) Y = *yp;
    if (!fan_ok(Y.nyaw, Y.step)) DSSS_FAIL(c, DSSS_E_ARG, "register: a fan of %d angles, %g rad apart (an odd number up to %d, a positive step)", Y.nyaw, Y.step, REG_MAX_YAW);
    const int nyaw = Y.nyaw, mid = (nyaw - 1) / 2;
    rc = Q.count(nyaw, cap, nseg_host, sums_host); if (rc) return rc;
    reg_count cnt;
    if (Q.nseg == 0) { c->reg_info = cnt.I; return DSSS_OK; }
    const int nseg = Q.nseg;
    const reg_pass P{ Q.R.radius, Q.R.min_cells, p->cell };
    const size_t tsz = reg_table_words(P.radius), table = (size_t)nseg * tsz;   // one angle's sums
    // windows: the whole frame where it occurs as a, every (segment, angle) where it occurs as b
    reg_layers W(n);
    std::vector<size_t> fan0(n, 0), fan_lay(n, 0), fan_cells(n, 0);             // a frame's first entry in sw / hfan; (segment s, angle k) is entry s nyaw + k behind it
    std::vector<mosaic_win> sw; std::vector<mosaic_fan> hfan;
    std::vector<double> rot;
    for (int i = 0; i < n; ++i) {
        if (Q.as_a[i]) W.add_a(Q, i, p);
        if (!Q.as_b[i]) continue;
        const dsss_frame& f = Q.frame(i);
        const double* fr = Q.rows_of(i);
        fan0[i] = sw.size();
        size_t cells = 0;
        for (int s = 0; s < Q.segs_of(i); ++s) {
            const int p0 = s * seg_pings, p1 = Q.seg_end(s, f.N);
            const double* piv = fr + (size_t)(((long long)p0 + p1) / 2) * 6;
            rot.resize((size_t)(p1 - p0) * 6);
            for (int k = 0; k < nyaw; ++k) {
                mosaic_win w = reg_grid(p);
                mosaic_fan F; F.cx = piv[3]; F.cy = piv[4]; F.theta = fan_theta(k, nyaw, Y.step);
                dsss_sincos(F.theta, &F.s, &F.c);
                rotate_rows(fr, p0, p1, F.theta, rot.data());
                mosaic_window(f, rot.data(), 0, p1 - p0, p, &w);
                F.ox = w.ox; F.oy = w.oy; F.bw = w.bw; F.bh = w.bh; F.off = (unsigned long long)cells;
                sw.push_back(w); hfan.push_back(F);
                cells += reg_round((size_t)w.bw * w.bh);
            }
        }
        fan_cells[i] = cells; fan_lay[i] = W.add_b(cells);
    }
    HIPCHK(c, hipSetDevice(c->device));
    reg_mem M;
    M.take(W.lay_cells, W.win_cells, n, rpy6 ? Q.traj_rows : 0, nseg, true, table, Q.dev);
    const mosaic_piece<mosaic_fan> o_fan = M.A.take<mosaic_fan>(hfan.size());
    rc = M.reserve(c); if (rc) return rc;
    rc = c->mosaic_pinned.reserve(c, M.down_bytes(nseg, tsz)); if (rc) return rc;
    mosaic_fan* d_fan = M.A.at(o_fan);
    // the rows and every pass's jobs before anything is launched: what one launch cannot take is refused here.  A row's centroid
    // region lies inside the correlation region of its angle, so the largest of those bounds it.
    memset(out_host, 0, (size_t)nseg * sizeof(dsss_reg_seg_yaw));
    Q.layout(fan0, nyaw, [&](int row) -> dsss_reg_seg& { return out_host[row].s; });
    auto layer_b = [&](int row, int a) { return M.lay + fan_lay[Q.row_b[row]] + hfan[Q.row_g[row] + a].off; };
    std::vector<std::vector<reg_job>> pj(nyaw);
    std::vector<long long> blocks(nyaw, 0);
    long long cen_bound = 0;
    for (int row = 0; row < nseg; ++row) {
        const int ia = Q.row_a[row]; const size_t g = Q.row_g[row];
        if (!W.on_grid[ia]) continue;
        long long most = 0;
        for (int a = 0; a < nyaw; ++a) {
            if (sw[g + a].bw == 0) continue;
            const size_t before = pj[a].size();
            if (!reg_push_job(pj[a], &blocks[a], M.lay + W.lay_off[ia], W.wins[ia], layer_b(row, a), sw[g + a], P.radius, M.tab + (size_t)row * tsz))
                DSSS_FAIL(c, DSSS_E_ARG, "register: %d segments are more than one launch takes", nseg);
            if (pj[a].size() == before) continue;
            const reg_job& J = pj[a].back();
            most = std::max(most, (long long)((J.rx1 - J.rx0) / CEN_TW + 2) * ((J.ry1 - J.ry0) / CEN_TH + 2));
        }
        cen_bound += most;
    }
    if (cen_bound > 0x7fffffffll) DSSS_FAIL(c, DSSS_E_ARG, "register: %d segments are more than one launch takes", nseg);
    std::vector<mosaic_job> jobs;
    rc = reg_upload_jobs(Q, M, jobs); if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(d_fan, hfan.data(), hfan.size() * sizeof(mosaic_fan), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(M.flag, 0, 8, c->stream));
    HIPCHK(c, hipMemsetAsync(M.cen, 0, (size_t)nseg * 3 * 8, c->stream));
    // 1. mean layers: a frame's whole layer where it is an a, the layers of all its segments under all angles (one scatter, one pack) where it is a b
    const mosaic_win grid = reg_grid(p);
    for (int i = 0; i < n; ++i) {
        if (W.on_grid[i]) { rc = reg_render_a(c, M, W, i, jobs[i].N); if (rc) return rc; }
        if (Q.as_b[i] && fan_cells[i]) {
            rc = reg_render_b(c, M, fan_cells[i], fan_lay[i], [&] {
                hipLaunchKernelGGL(mosaic_scatter_fan_kernel, dim3((unsigned)jobs[i].N * (unsigned)nyaw), dim3(256), 0, c->stream, M.jobs + i, grid, M.win,
                                   d_fan + fan0[i], seg_pings, nyaw); });
            if (rc) return rc;
        }
    }
    // 2. one pass per angle: the table cleared, one correlation job per row, one download, the records of the angle
    std::vector<dsss_reg_result> per((size_t)nseg * nyaw);
    for (int a = 0; a < nyaw; ++a) {
        HIPCHK(c, hipMemsetAsync(M.tab, 0, table * 8, c->stream));
        rc = reg_launch_corr(c, pj[a], blocks[a], M.pairs, P.radius); if (rc) return rc;
        reg_view v;
        rc = reg_fetch(c, M, nseg, nseg, P, p->cell, c->mosaic_pinned.p, cnt, &v); if (rc) return rc;
        for (int row = 0; row < nseg; ++row) {
            per[(size_t)row * nyaw + a] = v.record(row);
            if (sums_host) memcpy(sums_host + ((size_t)row * nyaw + a) * tsz, v.table(row), tsz * 8);
        }
    }
    // 3. the angle of every row on the host, then the centroid sums of the rows that have a peak under that angle
    for (int row = 0; row < nseg; ++row) {
        dsss_reg_seg_yaw& o = out_host[row];
        const dsss_reg_result* z = per.data() + (size_t)row * nyaw;
        yaw_peak_of(z, nyaw, Y.step, &o.k, &o.yaw_on_border, &o.theta, &o.theta_hat);
        o.s.r = z[o.k]; o.zncc_k0 = z[mid].zncc;
    }
    rc = reg_centroids(c, M, nseg, true, cnt, [&](int row, cen_src* s) {
        dsss_reg_seg_yaw& o = out_host[row];
        if (!(o.s.r.zncc > -2.0)) return false;                                 // no usable shift under any angle: sx = sy = 0
        *s = cen_src{ M.lay + W.lay_off[Q.row_a[row]], &W.wins[Q.row_a[row]], layer_b(row, o.k), &sw[Q.row_g[row] + o.k], &o.s };
        return true; });
    if (rc) return rc;
    c->reg_info = cnt.I;
    return DSSS_OK;
}

// dsss_mosaic_register_segments coarse to fine.  Per frame: ONE memset, the unchanged scatter kernels into the accumulators of its whole
// window (where it is an a) and of all its segments (where it is a b), and ONE mosaic_pyr_kernel over all those areas that writes
// the layers of every level; the layers of all levels stay resident.  Per level, from the top: mosaic_corr_kernel with one job per row
// that is still alive (the segment's window moved by minus the row's centre), one download -- of the records of the live rows, whose
// tables then lie one behind the other (mosaic_peak_kernel with the level's radius, min_cells and cell), or of that level's tables of
// all rows when the sums are asked for -- and the level rule on the host: the level's record (reg_view), then pyr_centre_of and
// pyr_apply on both paths.  mosaic_centroid_kernel runs once, at the total shift, for the rows that finished at level 0.  What one
// launch cannot take is bounded and refused before anything is launched.
int dsss_mosaic_register_segments_pyr(dsss_ctx* c, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params* p,
                                      const int* pair_a, const int* pair_b, int npairs, int seg_pings, const dsss_reg_params* rp,
                                      const dsss_reg_pyr_params* pp, dsss_reg_seg_pyr* out_host, int cap, int* nseg_host, uint64_t* sums_host)
{
    if (!c) return DSSS_E_ARG;
    reg_rows Q;
    int rc = Q.check(c, ids, n, rpy6, ping_off, p, pair_a, pair_b, npairs, rp, out_host); if (rc) return rc;
    rc = Q.check_segments(seg_pings, nseg_host, cap); if (rc) return rc;
    dsss_reg_pyr_params P; dsss_reg_pyr_params_default(&P);
    if (pp) P = *pp;
    if (!pyr_ok(P)) DSSS_FAIL(c, DSSS_E_ARG, "register: a pyramid of %d levels refined within %d cells (1..%d levels, 1..%d cells)", P.levels, P.refine, PYR_MAX_LEVELS, REG_MAX_RADIUS);
    const int L = P.levels;
    rc = Q.count(1, cap, nseg_host, sums_host); if (rc) return rc;
    reg_count cnt;
    if (Q.nseg == 0) { c->reg_info = cnt.I; return DSSS_OK; }
    const int nseg = Q.nseg; const bool dev = Q.dev;
    auto radius_of = [&](int l) { return l == L - 1 ? Q.R.radius : P.refine; };
    auto words_of = [&](int l) { return reg_table_words(radius_of(l)); };
    // areas: the whole frame where it occurs as a, every segment where it occurs as b; an area's accumulators lie behind the frame's
    // first, its layers of all levels in M.lay
    struct area_lay { size_t off[PYR_MAX_LEVELS]; };
    std::vector<mosaic_win> wins(n); std::vector<char> on_grid(n, 0); std::vector<area_lay> a_lay(n);
    std::vector<size_t> seg0(n, 0);                                             // a frame's first segment in sw / hseg
    std::vector<int> job0(n, 0), njobs(n, 0);                                   // a frame's areas in hpj
    std::vector<size_t> a_cells(n, 0), acc_cells(n, 0); std::vector<long long> pyr_blocks(n, 0);
    std::vector<mosaic_win> sw; std::vector<mosaic_seg> hseg; std::vector<area_lay> seg_lay; std::vector<pyr_job> hpj;
    size_t win_cells = 1, lay_cells = 0;
    auto add_area = [&](int i, const mosaic_win& w, size_t acc, area_lay* lay) {
        pyr_job J;
        J.acc = (unsigned long long)acc; J.ox = w.ox; J.oy = w.oy; J.bw = w.bw; J.bh = w.bh; J.bx0 = w.ox & ~7; J.by0 = w.oy & ~7;
        for (int l = 0; l < PYR_MAX_LEVELS; ++l) {
            lay->off[l] = J.lay[l] = lay_cells;
            if (l >= L) continue;
            const mosaic_win q = pyr_window(w, l, 0, 0);
            lay_cells += reg_round((size_t)q.bw * q.bh);
        }
        J.tiles_x = (w.ox + w.bw - 1 - J.bx0) / PYR_TW + 1; J.blk0 = (int)pyr_blocks[i];
        pyr_blocks[i] += (long long)J.tiles_x * ((w.oy + w.bh - 1 - J.by0) / PYR_TH + 1);
        if (pyr_blocks[i] <= 0x7fffffffll) { hpj.push_back(J); ++njobs[i]; }   // (more is refused below, before anything is launched)
    };
    for (int i = 0; i < n; ++i) {
        const dsss_frame& f = Q.frame(i);
        const double* fr = Q.rows_of(i);
        job0[i] = (int)hpj.size();
        if (Q.as_a[i] && mosaic_window(f, fr, 0, f.N, p, &wins[i])) {
            on_grid[i] = 1;
            add_area(i, wins[i], 0, &a_lay[i]);
            a_cells[i] = reg_round((size_t)wins[i].bw * wins[i].bh);
        }
        size_t cells = 0;
        if (Q.as_b[i]) {
            seg0[i] = sw.size();
            for (int s = 0; s < Q.segs_of(i); ++s) {
                mosaic_win w = reg_grid(p);
                area_lay al{};
                if (mosaic_window(f, fr, s * seg_pings, Q.seg_end(s, f.N), p, &w)) add_area(i, w, a_cells[i] + cells, &al);
                sw.push_back(w); seg_lay.push_back(al); hseg.push_back(mosaic_seg{ w.ox, w.oy, w.bw, w.bh, (unsigned long long)cells });
                cells += reg_round((size_t)w.bw * w.bh);
            }
        }
        acc_cells[i] = a_cells[i] + cells; win_cells = std::max(win_cells, acc_cells[i]);
        if (pyr_blocks[i] > 0x7fffffffll) DSSS_FAIL(c, DSSS_E_ARG, "register: the areas of frame %d are more than one launch takes", ids[i]);
    }
    // the rows, and what the launches of every level and of the centroid can need at most: a level's region lies inside the
    // segment's window of that level dilated by the radius, the centroid's inside the segment's fine window
    memset(out_host, 0, (size_t)nseg * sizeof(dsss_reg_seg_pyr));
    Q.layout(seg0, 1, [&](int row) -> dsss_reg_seg& { return out_host[row].s; });
    {
        long long bound[PYR_MAX_LEVELS] = { 0, 0, 0, 0 }, cen_bound = 0;
        for (int row = 0; row < nseg; ++row) {
            dsss_reg_seg_pyr& o = out_host[row];
            o.level = -1;
            for (int l = 0; l < PYR_MAX_LEVELS; ++l) o.lz[l] = -2.0;
            const int ia = Q.row_a[row]; const size_t g = Q.row_g[row];
            if (!on_grid[ia] || sw[g].bw == 0) continue;
            for (int l = 0; l < L; ++l) {
                const mosaic_win A = pyr_window(wins[ia], l, 0, 0), Bw = pyr_window(sw[g], l, 0, 0);
                const long long w = std::min(A.bw, Bw.bw + 2 * radius_of(l)), h = std::min(A.bh, Bw.bh + 2 * radius_of(l));
                bound[l] += (((w - 1) / REG_TILE + 1) + REG_STRIP - 1) / REG_STRIP * ((h - 1) / REG_TILE + 1);
            }
            cen_bound += (long long)((std::min(wins[ia].bw, sw[g].bw) - 1) / CEN_TW + 1) * ((std::min(wins[ia].bh, sw[g].bh) - 1) / CEN_TH + 1);
        }
        for (int l = 0; l < L; ++l)
            if (bound[l] > 0x7fffffffll || cen_bound > 0x7fffffffll) DSSS_FAIL(c, DSSS_E_ARG, "register: %d segments are more than one launch takes", nseg);
    }
    HIPCHK(c, hipSetDevice(c->device));
    const size_t words_max = std::max(words_of(L - 1), words_of(0));
    reg_mem M;
    M.take(lay_cells, win_cells, n, rpy6 ? Q.traj_rows : 0, nseg, true, (size_t)nseg * words_max, dev);
    const mosaic_piece<mosaic_seg> o_segs = M.A.take<mosaic_seg>(hseg.size());
    const mosaic_piece<pyr_job> o_pj = M.A.take<pyr_job>(hpj.size());
    rc = M.reserve(c); if (rc) return rc;
    rc = c->mosaic_pinned.reserve(c, M.down_bytes(nseg, words_max)); if (rc) return rc;
    mosaic_seg* d_segs = M.A.at(o_segs); pyr_job* d_pj = M.A.at(o_pj);
    std::vector<mosaic_job> jobs;
    rc = reg_upload_jobs(Q, M, jobs); if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(d_segs, hseg.data(), hseg.size() * sizeof(mosaic_seg), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_pj, hpj.data(), hpj.size() * sizeof(pyr_job), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(M.flag, 0, 8, c->stream));
    HIPCHK(c, hipMemsetAsync(M.cen, 0, (size_t)nseg * 3 * 8, c->stream));
    // 1. the layers of all levels: per frame one memset, its scatters and one pyramid launch over all its areas
    const mosaic_win grid = reg_grid(p);
    for (int i = 0; i < n; ++i) {
        if (!njobs[i]) continue;
        HIPCHK(c, hipMemsetAsync(M.win, 0, acc_cells[i] * 8, c->stream));
        if (on_grid[i]) launch_scatter(c, M.jobs + i, 1, jobs[i].N, wins[i], M.win);
        if (acc_cells[i] > a_cells[i]) launch_scatter_seg(c, M.jobs + i, jobs[i].N, grid, M.win + a_cells[i], d_segs + seg0[i], seg_pings);
        hipLaunchKernelGGL(mosaic_pyr_kernel, dim3((unsigned)pyr_blocks[i]), dim3(256), 0, c->stream, d_pj + job0[i], njobs[i], L, M.win, M.lay, M.flag);
        HIPCHK(c, hipGetLastError());
    }
    // 2. level by level from the top: the rows still alive around their centres, one launch, one download, the level rule on the host
    std::vector<int> live; live.reserve(nseg);                                  // the rows still alive; device path: their tables lie one behind the other
    const size_t row_sums = words_of(L - 1) + (size_t)(L - 1) * words_of(0);
    std::vector<char> alive(nseg, 1); std::vector<int32_t> cx(nseg, 0), cy(nseg, 0);
    std::vector<reg_job> pj; pj.reserve(nseg);
    for (int l = L - 1; l >= 0; --l) {
        const reg_pass Pl{ radius_of(l), pyr_min_cells(Q.R.min_cells, l), ldexp(p->cell, l) };
        const size_t tsz = words_of(l);
        auto place = [&](size_t k) { return dev ? k : (size_t)live[k]; };       // host path: every row keeps its place
        pj.clear(); live.clear();
        long long blocks = 0;
        for (int row = 0; row < nseg; ++row) {
            const int ia = Q.row_a[row]; const size_t g = Q.row_g[row];
            if (!alive[row]) continue;
            live.push_back(row);                                                // (a live row off the grid has no job: its table stays zero)
            if (!on_grid[ia] || sw[g].bw == 0) continue;
            if (!reg_push_job(pj, &blocks, M.lay + a_lay[ia].off[l], pyr_window(wins[ia], l, 0, 0), M.lay + seg_lay[g].off[l], pyr_window(sw[g], l, cx[row], cy[row]),
                              Pl.radius, M.tab + place(live.size() - 1) * tsz))
                DSSS_FAIL(c, DSSS_E_NUMERIC, "register: internal error, level %d of %d segments takes more workgroups than was bounded", l, nseg);
        }
        const size_t ntab = dev ? live.size() : (size_t)nseg;
        HIPCHK(c, hipMemsetAsync(M.tab, 0, ntab * tsz * 8, c->stream));
        rc = reg_launch_corr(c, pj, blocks, M.pairs, Pl.radius); if (rc) return rc;
        reg_view v;
        rc = reg_fetch(c, M, ntab, live.size(), Pl, p->cell, c->mosaic_pinned.p, cnt, &v); if (rc) return rc;
        if (sums_host) {
            const size_t at = l == L - 1 ? 0 : words_of(L - 1) + (size_t)(L - 2 - l) * words_of(0);      // this level's table within a row of sums_host
            for (int row = 0; row < nseg; ++row) {
                if (alive[row]) memcpy(sums_host + (size_t)row * row_sums + at, v.table(row), tsz * 8);
                else memset(sums_host + (size_t)row * row_sums + at, 0, tsz * 8);
            }
        }
        for (size_t k = 0; k < live.size(); ++k) {
            const int row = live[k];
            dsss_reg_result q = v.record(place(k)); int32_t usable = 0, nx = 0, ny = 0;
            pyr_centre_of(p->cell, l, cx[row], cy[row], &q, &usable, &nx, &ny);
            pyr_apply(out_host[row], q, usable != 0, l, l == L - 1, nx, ny, &alive[row], &cx[row], &cy[row]);
        }
    }
    // 3. the centroid sums at the total shift of the rows that finished at level 0
    for (int row = 0; row < nseg; ++row) {
        dsss_reg_seg_pyr& o = out_host[row];
        if (o.level >= 0) o.s.r.on_border = (o.border_mask != 0 || o.level != 0) ? 1 : 0;      // the no-usable-shift record stays as it is
    }
    rc = reg_centroids(c, M, nseg, true, cnt, [&](int row, cen_src* s) {
        if (out_host[row].level != 0) return false;
        *s = cen_src{ M.lay + a_lay[Q.row_a[row]].off[0], &wins[Q.row_a[row]], M.lay + seg_lay[Q.row_g[row]].off[0], &sw[Q.row_g[row]], &out_host[row].s };
        return true; });
    if (rc) return rc;
    c->reg_info = cnt.I;
    return DSSS_OK;
}

// ---- peaks on the device: the public batched entry and what the last call did
int dsss_mosaic_register_peaks(dsss_ctx* c, const uint64_t* sums, int64_t ntables, int radius, int min_cells, double cell, dsss_reg_result* out_host)
{
    if (!c) return DSSS_E_ARG;
    if (ntables < 0) DSSS_FAIL(c, DSSS_E_ARG, "register: ntables = %lld", (long long)ntables);
    if (ntables > 0 && (!sums || !out_host)) DSSS_FAIL(c, DSSS_E_ARG, "register: %lld tables without %s", (long long)ntables, sums ? "a result array" : "their sums");
    if (radius < 0 || radius > REG_MAX_RADIUS) DSSS_FAIL(c, DSSS_E_ARG, "register: radius %d outside 0..%d", radius, REG_MAX_RADIUS);
    if (min_cells < 1) DSSS_FAIL(c, DSSS_E_ARG, "register: min_cells = %d", min_cells);
    if (!(cell > 0.0) || !std::isfinite(cell)) DSSS_FAIL(c, DSSS_E_ARG, "register: cell = %g", cell);
    reg_count cnt;
    if (ntables == 0) { c->reg_info = cnt.I; return DSSS_OK; }
    HIPCHK(c, hipSetDevice(c->device));
    const size_t tsz = reg_table_words(radius), nt = (size_t)ntables;
    hipPointerAttribute_t at;
    const bool on_dev = (hipPointerGetAttributes(&at, sums) == hipSuccess) && at.type == hipMemoryTypeDevice;
    (void)hipGetLastError();
    mosaic_arena A;
    const mosaic_piece<dsss_reg_result> o_rec = A.take<dsss_reg_result>(nt);
    const mosaic_piece<unsigned long long> o_tab = A.take<unsigned long long>(on_dev ? 0 : nt * tsz);      // host tables go up into mosaic_buf
    int rc = A.reserve(c); if (rc) return rc;
    rc = c->mosaic_pinned.reserve(c, nt * sizeof(dsss_reg_result)); if (rc) return rc;
    dsss_reg_result* d_rec = A.at(o_rec);
    const unsigned long long* d_tab = reinterpret_cast<const unsigned long long*>(sums);
    if (!on_dev) {
        HIPCHK(c, hipMemcpyAsync(A.at(o_tab), sums, nt * tsz * 8, hipMemcpyHostToDevice, c->stream));
        d_tab = A.at(o_tab);
    }
    rc = reg_launch_peaks(c, d_tab, ntables, radius, min_cells, cell, d_rec); if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->mosaic_pinned.p, d_rec, nt * sizeof(dsss_reg_result), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    cnt.down(nt * sizeof(dsss_reg_result)); cnt.sync();
    memcpy(out_host, c->mosaic_pinned.p, nt * sizeof(dsss_reg_result));
    cnt.I.tables_device = ntables; c->reg_info = cnt.I;
    return DSSS_OK;
}

int dsss_mosaic_register_info(const dsss_ctx* c, dsss_reg_call_info* out)
{
    if (!c || !out) return DSSS_E_ARG;
    *out = c->reg_info;
    return DSSS_OK;
}

} // extern "C"

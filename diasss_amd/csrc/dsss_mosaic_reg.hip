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
#include "dsss_mosaic_int.h"
#include "dsss_pose.h"
#include "dsss_wave.h"
#include <algorithm>

#define REG_MAX_RADIUS 16
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
    const unsigned long long a = win[i];
    const uint32_t c = (uint32_t)(a >> 32), s = (uint32_t)a;
    if (c > MOSAIC_MAX_SAMPLES) *flag = 1;
    lay[i] = c ? (uint16_t)(0x100u | ((s + c / 2) / c)) : (uint16_t)0;
}

// ---- the pyramid of mean layers ("dense loop closures over a cell pyramid" in the header)
#define PYR_MAX_LEVELS 4
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
    int lo = 0, hi = njobs - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (jobs[mid].blk0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1; }
    const pyr_job J = jobs[lo];
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
        unsigned long long a = 0;
        if (x >= 0 && x < J.bw && y >= 0 && y < J.bh) a = win[(size_t)y * J.bw + x];
        const uint32_t c = (uint32_t)(a >> 32), s = (uint32_t)a;
        over |= c > MOSAIC_MAX_SAMPLES;
        c0[k] = c; s0[k] = s;
        if (x >= 0 && x < J.bw && y >= 0 && y < J.bh) lay[J.lay[0] + (size_t)y * J.bw + x] = c ? (uint16_t)(0x100u | ((s + c / 2) / c)) : (uint16_t)0;
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
    int lo = 0, hi = njobs - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (jobs[mid].blk0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1; }
    const reg_job J = jobs[lo];
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
    int lo = 0, hi = njobs - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (jobs[mid].blk0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1; }
    const cen_job J = jobs[lo];
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
    const mosaic_job J = *job;
    const int row = (int)(blockIdx.x / (unsigned)nyaw), k = (int)(blockIdx.x - (unsigned)row * (unsigned)nyaw);
    if (row >= J.N) return;                                                        // (uniform per workgroup; cannot happen with the host's grid)
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

int peak_of(const uint64_t* sums, int radius, int min_cells, double cell, dsss_reg_result* out)
{
    const int S = 2 * radius + 1;
    std::vector<reg_score> z((size_t)S * S);
    for (int s = 0; s < S * S; ++s) z[s] = reg_score_of(sums + (size_t)s * 6, min_cells);
    bool found = false; int bx = 0, by = 0;
    for (int dy = -radius; dy <= radius; ++dy)
        for (int dx = -radius; dx <= radius; ++dx) {
            const reg_score& q = z[(size_t)(dy + radius) * S + (dx + radius)];
            if (!q.ok) continue;
            if (!found || reg_better(q.z, dx, dy, z[(size_t)(by + radius) * S + (bx + radius)].z, bx, by)) { found = true; bx = dx; by = dy; }
        }
    const size_t zero = (size_t)radius * S + radius, pk = (size_t)(by + radius) * S + (bx + radius);
    const bool inner = found && abs(bx) != radius && abs(by) != radius;      // the four neighbours exist
    const reg_score none = { -2.0, false };
    reg_record(found, bx, by, radius, cell, z[zero], sums[zero * 6], z[pk], sums[pk * 6], inner ? z[pk - 1] : none, inner ? z[pk + 1] : none,
               inner ? z[pk - S] : none, inner ? z[pk + S] : none, out);
    return DSSS_OK;
}

// what a registration call did (dsss_reg_call_info), counted where the call enqueues its copies and synchronises
struct reg_count {
    dsss_reg_call_info I{0, 0, 0, 0};
    void down(size_t bytes) { I.bytes_down += (int64_t)bytes; }
    void sync() { I.syncs += 1; }
};

// ---- what dsss_mosaic_register and dsss_mosaic_register_segments share on the host
// the argument rules of both entries; R = the parameters in force, slot = frame id -> its index in ids, rows = pings of all frames
int reg_check(dsss_ctx* c, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params* p, const int* pair_a,
              const int* pair_b, int npairs, const dsss_reg_params* rp, const void* out_host, dsss_reg_params* R, std::vector<int>& slot, size_t* rows)
{
    if (dsss_comm_world(c) > 1) DSSS_FAIL(c, DSSS_E_STATE, "mosaic: registration runs on a single rank (communicator of %d)", dsss_comm_world(c));
    int rc = mosaic_check_frames(c, ids, n, rpy6, ping_off, true, rows); if (rc) return rc;
    rc = mosaic_check_params(c, p); if (rc) return rc;
    dsss_reg_params_default(R);
    if (rp) *R = *rp;
    if (R->radius < 0 || R->radius > REG_MAX_RADIUS) DSSS_FAIL(c, DSSS_E_ARG, "register: radius %d outside 0..%d", R->radius, REG_MAX_RADIUS);
    if (R->min_cells < 1) DSSS_FAIL(c, DSSS_E_ARG, "register: min_cells = %d", R->min_cells);
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

// the window of the pings [r0, r1) of a frame: the cells their geo extremes can reach (as the consistency map's); false: none on the grid
bool reg_window(const dsss_frame& f, const double* rows, int r0, int r1, const dsss_mosaic_params* p, mosaic_win* w)
{
    double bb[4] = { INFINITY, -INFINITY, INFINITY, -INFINITY };
    frame_extent_rows(f, rows, r0, r1, bb);
    int ax, bx, ay, by;
    if (!cell_range(bb[0], bb[1], p->x0, p->cell, p->W, &ax, &bx) || !cell_range(bb[2], bb[3], p->y0, p->cell, p->H, &ay, &by)) return false;
    *w = mosaic_win{ p->x0, p->y0, p->cell, p->W, p->H, ax, ay, bx - ax + 1, by - ay + 1, p->use_mask != 0 };
    return true;
}

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

// all centroid jobs in one launch, and the nseg x 3 sums back in cen (d_cen was cleared before)
int reg_launch_centroids(dsss_ctx* c, const std::vector<cen_job>& cj, long long cblocks, cen_job* d_cj, const unsigned long long* d_cen, std::vector<uint64_t>& cen,
                         reg_count& cnt)
{
    HIPCHK(c, hipMemcpyAsync(d_cj, cj.data(), cj.size() * sizeof(cen_job), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(mosaic_centroid_kernel, dim3((unsigned)cblocks), dim3(256), 0, c->stream, d_cj, (int)cj.size());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(cen.data(), d_cen, cen.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    cnt.down(cen.size() * 8); cnt.sync();
    return DSSS_OK;
}

// ---- the yaw fan
#define REG_MAX_YAW 17

bool fan_ok(int nyaw, double step) { return nyaw >= 1 && nyaw <= REG_MAX_YAW && (nyaw & 1) && step > 0.0 && std::isfinite(step); }
double fan_theta(int k, int nyaw, double step) { return (double)(k - (nyaw - 1) / 2) * step; }

// the pings [p0, p1) of rows_b rotated by theta about the position of ping (p0 + p1) / 2 -> out, (p1 - p0) x 6
void rotate_rows(const double* rows_b, int p0, int p1, double theta, double* out)
{
    const double* piv = rows_b + (size_t)(((long long)p0 + p1) / 2) * 6;
    double s, co; dsss_sincos(theta, &s, &co);
    for (int i = p0; i < p1; ++i) dsss_rotate_row(rows_b + (size_t)i * 6, piv[3], piv[4], theta, s, co, out + (size_t)(i - p0) * 6);
}

// the angle rule of the header, "dense loop closures with a yaw fan": the one place it is written
void yaw_peak_of(const dsss_reg_result* z, int nyaw, double step, int32_t* k, int32_t* border, double* theta, double* theta_hat)
{
    const int mid = (nyaw - 1) / 2;
    int best = -1;
    for (int i = 0; i < nyaw; ++i) {
        if (!(z[i].zncc > -2.0)) continue;
        if (best < 0 || z[i].zncc > z[best].zncc || (z[i].zncc == z[best].zncc && abs(i - mid) < abs(best - mid))) best = i;   // equals at one distance: the lower k came first
    }
    if (best < 0) { *k = mid; *border = 0; *theta = 0.0; *theta_hat = 0.0; return; }
    *k = best; *border = (nyaw > 1 && (best == 0 || best == nyaw - 1)) ? 1 : 0;
    *theta = fan_theta(best, nyaw, step);
    double q = 0.0;
    if (!*border && nyaw > 1 && z[best - 1].zncc > -2.0 && z[best + 1].zncc > -2.0) {
        const double zm = z[best - 1].zncc, z0 = z[best].zncc, zp = z[best + 1].zncc;
        const double den = zm - 2.0 * z0 + zp;
        if (den < 0.0) q = 0.5 * (zm - zp) / den;
    }
    *theta_hat = *theta + q * step;
}

// dsss_register_edge and dsss_register_edge_yaw: the segment row s as an edge, its pings rotated by theta where the anchor ping is
// looked for and by theta_hat where it is measured (both 0: the rows as they are), s_yaw = the sigma of the yaw
int edge_of(const dsss_reg_seg* s, const dsss_mosaic_params* grid, const double* rows_a, int Na, int base_a, const double* rows_b, int Nb, int base_b,
            const dsss_reg_edge_params& E, double theta, double theta_hat, double s_yaw, dsss_lc_edge* edge)
{
    if (!s || !grid || !rows_a || !rows_b || !edge || Na < 1 || Nb < 1) return DSSS_E_ARG;
    if (s->p0 < 0 || s->p0 >= s->p1 || s->p1 > Nb) return DSSS_E_ARG;
    if (!(grid->cell > 0.0) || !std::isfinite(grid->cell)) return DSSS_E_ARG;
    const double sig[4] = { E.sigma_xy_cells, E.sigma_z, E.sigma_rot, s_yaw };
    for (double v : sig) if (!(v > 0.0) || !std::isfinite(v)) return DSSS_E_ARG;
    if (!std::isfinite(theta) || !std::isfinite(theta_hat)) return DSSS_E_ARG;
    if (!(s->r.zncc >= E.min_zncc) || s->r.on_border != 0) return 0;
    if (s->r.n <= 0) return DSSS_E_ARG;
    const double cell = grid->cell;
    const double cx = grid->x0 + ((double)s->sx / (double)s->r.n + 0.5) * cell, cy = grid->y0 + ((double)s->sy / (double)s->r.n + 0.5) * cell;
    // the ping whose scan line (through the ping, across the heading) passes nearest the point: the lowest index among equals
    auto anchor = [](const double* rows, int r0, int r1, double px, double py) {
        int best = r0; double dbest = INFINITY;
        for (int i = r0; i < r1; ++i) {
            const double* P = rows + (size_t)i * 6;
            const double d = fabs(cos(P[2]) * (px - P[3]) + sin(P[2]) * (py - P[4]));
            if (d < dbest) { dbest = d; best = i; }
        }
        return best;
    };
    const int i = anchor(rows_a, 0, Na, cx, cy);
    std::vector<double> rot((size_t)(s->p1 - s->p0) * 6);                       // the segment's rows under theta (theta == 0: a copy)
    rotate_rows(rows_b, s->p0, s->p1, theta, rot.data());
    const int j = s->p0 + anchor(rot.data(), 0, s->p1 - s->p0, cx + s->r.off_x, cy + s->r.off_y);      // b's rendering lies off from where it belongs
    double rowj[6], sh, ch;                                                     // row j of the rows under theta_hat
    const double* piv = rows_b + (size_t)(((long long)s->p0 + s->p1) / 2) * 6;
    dsss_sincos(theta_hat, &sh, &ch);
    dsss_rotate_row(rows_b + (size_t)j * 6, piv[3], piv[4], theta_hat, sh, ch, rowj);
    pose_t Xa, Xb, rel;
    pose_from_rodrigues(rows_a + (size_t)i * 6, &Xa);
    pose_from_rodrigues(rowj, &Xb);
    Xb.t[0] -= s->r.off_x; Xb.t[1] -= s->r.off_y;
    const long long ga = (long long)base_a + i, gb = (long long)base_b + j;
    if (ga < 0 || gb < 0 || ga > 0x7fffffffll || gb > 0x7fffffffll) return DSSS_E_ARG;
    if (ga < gb) { edge->a = (int32_t)ga; edge->b = (int32_t)gb; pose_between(&Xa, &Xb, &rel); }
    else { edge->a = (int32_t)gb; edge->b = (int32_t)ga; pose_between(&Xb, &Xa, &rel); }
    memcpy(edge->rel, rel.R, 9 * sizeof(double)); memcpy(edge->rel + 9, rel.t, 3 * sizeof(double));
    const double sxy = E.sigma_xy_cells * cell;
    edge->var[0] = edge->var[1] = E.sigma_rot * E.sigma_rot; edge->var[2] = s_yaw * s_yaw;
    edge->var[3] = edge->var[4] = sxy * sxy; edge->var[5] = E.sigma_z * E.sigma_z;
    return 1;
}

// the row loop of dsss_mosaic_register_edges and dsss_mosaic_register_edges_yaw: seg_of(k) = the (pair, segment) part of row k,
// edge_fn(k, rows_a, Na, base_a, rows_b, Nb, base_b, &e) = what dsss_register_edge(_yaw) says about it
template <class SegOf, class EdgeFn>
int edges_loop(dsss_ctx* c, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params* p, const int* pair_a, const int* pair_b,
               bool have_segs, int nsegs, dsss_lc_edge* edges_host, int32_t* edge_seg_host, int cap, int* n_edges, SegOf seg_of, EdgeFn edge_fn)
{
    if (!c) return DSSS_E_ARG;
    if (dsss_comm_world(c) > 1) DSSS_FAIL(c, DSSS_E_STATE, "mosaic: registration runs on a single rank (communicator of %d)", dsss_comm_world(c));
    size_t rows = 0;
    int rc = mosaic_check_frames(c, ids, n, rpy6, ping_off, false, &rows); if (rc) return rc;
    rc = mosaic_check_params(c, p); if (rc) return rc;
    if (nsegs < 0 || cap < 0 || !n_edges) DSSS_FAIL(c, DSSS_E_ARG, "register: nsegs = %d, cap = %d%s", nsegs, cap, n_edges ? "" : ", nowhere to write the number of edges");
    if (nsegs > 0 && (!pair_a || !pair_b || !have_segs)) DSSS_FAIL(c, DSSS_E_ARG, "register: %d segments without %s", nsegs, have_segs ? "their pairs" : "their rows");
    std::vector<int> slot(c->max_frames, -1), base(n);
    int run = 0;
    for (int i = 0; i < n; ++i) { slot[ids[i]] = i; base[i] = ping_off ? ping_off[i] : run; run += c->frames[ids[i]].N; }
    int ne = 0;
    for (int k = 0; k < nsegs; ++k) {
        const dsss_reg_seg& sg = seg_of(k);
        if (sg.pair < 0) DSSS_FAIL(c, DSSS_E_ARG, "register: row %d names pair %d", k, sg.pair);
        const int a = pair_a[sg.pair], b = pair_b[sg.pair];
        if (a < 0 || a >= c->max_frames || slot[a] < 0 || b < 0 || b >= c->max_frames || slot[b] < 0)
            DSSS_FAIL(c, DSSS_E_ARG, "register: row %d, pair (%d, %d) names a frame that is not listed", k, a, b);
        const int ia = slot[a], ib = slot[b];
        const dsss_frame& fa = c->frames[a]; const dsss_frame& fb = c->frames[b];
        dsss_lc_edge e;
        rc = edge_fn(k, rpy6 ? rpy6 + (size_t)ping_off[ia] * 6 : fa.h_geo, fa.N, base[ia],
                     rpy6 ? rpy6 + (size_t)ping_off[ib] * 6 : fb.h_geo, fb.N, base[ib], &e);
        if (rc < 0) DSSS_FAIL(c, rc, "register: row %d (pair %d, segment %d, pings %d..%d) is not a valid segment result", k, sg.pair, sg.seg, sg.p0, sg.p1);
        if (rc == 0) continue;
        if (ne >= cap || !edges_host) DSSS_FAIL(c, DSSS_E_CAPACITY, "register: more than %d edges", edges_host ? cap : 0);
        edges_host[ne] = e;
        if (edge_seg_host) edge_seg_host[ne] = k;
        ++ne;
    }
    *n_edges = ne;
    return DSSS_OK;
}

// ---- the cell pyramid
#define PYR_MAX_CENTRE (1 << 28)           // |cx|, |cy| of a level's centre: twice the centre plus the radius stays an int32

bool pyr_ok(const dsss_reg_pyr_params& P) { return P.levels >= 1 && P.levels <= PYR_MAX_LEVELS && (P.levels == 1 || (P.refine >= 1 && P.refine <= REG_MAX_RADIUS)); }

// the level rule of the header, "dense loop closures over a cell pyramid": the one place it is written.  sums = the table of level
// `level` around the centre (cx, cy); min_cells and cell are the level-0 values.  It has two parts: the record of the level's table
// under pyr_min_cells and the level's cell (peak_of on the host, mosaic_peak_kernel on the device), and pyr_centre_of, which adds the
// centre to that record (*out) and is host arithmetic on both paths.
void pyr_centre_of(double cell, int level, int cx, int cy, dsss_reg_result* out, int32_t* usable, int32_t* ncx, int32_t* ncy)
{
    const double cell_l = ldexp(cell, level);
    *usable = out->zncc > -2.0 ? 1 : 0;
    if (!*usable) return;                                                       // the no-usable-shift record as it is: no centre is added to it
    out->dx += cx; out->dy += cy;
    const double mx = (double)cx * cell_l, my = (double)cy * cell_l;            // one multiply and one add each, unfused (-ffp-contract=off)
    out->off_x = out->off_x + mx; out->off_y = out->off_y + my;
    if (level > 0) { *ncx = 2 * out->dx; *ncy = 2 * out->dy; }
}
int pyr_min_cells(int min_cells, int level) { return std::max(1, min_cells >> (2 * level)); }
void pyr_step_of(const uint64_t* sums, int radius, int min_cells, double cell, int level, int cx, int cy, dsss_reg_result* out, int32_t* usable,
                 int32_t* ncx, int32_t* ncy)
{
    peak_of(sums, radius, pyr_min_cells(min_cells, level), ldexp(cell, level), out);
    pyr_centre_of(cell, level, cx, cy, out, usable, ncx, ncy);
}

// the window of level l that the fine window w covers (only ox, oy, bw, bh differ), moved by (-cx, -cy)
mosaic_win pyr_window(const mosaic_win& w, int l, int cx, int cy)
{
    mosaic_win q = w;
    q.ox = w.ox >> l; q.oy = w.oy >> l;
    q.bw = ((w.ox + w.bw - 1) >> l) - q.ox + 1; q.bh = ((w.oy + w.bh - 1) >> l) - q.oy + 1;
    q.ox -= cx; q.oy -= cy;
    return q;
}

} // namespace

extern "C" {

void dsss_reg_params_default(dsss_reg_params* p) { if (p) { p->radius = 8; p->min_cells = 256; } }

int dsss_mosaic_register_peak(const uint64_t* sums, int radius, int min_cells, double cell, dsss_reg_result* out)
{
    if (!sums || !out || radius < 0 || radius > REG_MAX_RADIUS || min_cells < 1 || !(cell > 0.0) || !std::isfinite(cell)) return DSSS_E_ARG;
    return peak_of(sums, radius, min_cells, cell, out);
}

int dsss_mosaic_register(dsss_ctx* c, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params* p,
                         const int* pair_a, const int* pair_b, int npairs, const dsss_reg_params* rp,
                         dsss_reg_result* out_host, uint64_t* sums_host)
{
    if (!c) return DSSS_E_ARG;
    size_t rows = 0;
    dsss_reg_params R; std::vector<int> slot;                                   // slot: frame id -> its index in ids
    int rc = reg_check(c, ids, n, rpy6, ping_off, p, pair_a, pair_b, npairs, rp, out_host, &R, slot, &rows); if (rc) return rc;
    std::vector<char> used(n, 0);
    for (int k = 0; k < npairs; ++k) used[slot[pair_a[k]]] = used[slot[pair_b[k]]] = 1;
    reg_count cnt;
    if (npairs == 0) { c->reg_info = cnt.I; return DSSS_OK; }
    const bool dev = !sums_host && !dsss_switches_read().reg_peaks_host;       // the peaks on the device: nobody reads the table on the host
    HIPCHK(c, hipSetDevice(c->device));
    const int r = R.radius, S = 2 * r + 1, nshift = S * S;
    // the window of every frame that occurs in a pair: the cells its geo extremes can reach (as the consistency map's)
    std::vector<mosaic_win> wins(n); std::vector<char> on_grid(n, 0); std::vector<size_t> lay_off(n, 0);
    size_t win_cells = 1, lay_cells = 0;
    for (int i = 0; i < n; ++i) {
        if (!used[i]) continue;
        const dsss_frame& f = c->frames[ids[i]];
        if (!reg_window(f, rpy6 ? rpy6 + (size_t)ping_off[i] * 6 : f.h_geo, 0, f.N, p, &wins[i])) continue;
        on_grid[i] = 1;
        const size_t wc = (size_t)wins[i].bw * wins[i].bh;
        win_cells = std::max(win_cells, wc);
        lay_off[i] = lay_cells; lay_cells += (wc + 127) & ~(size_t)127;        // layers start on 256 bytes
    }
    const size_t table = (size_t)npairs * nshift * 6;
    carve L;
    const size_t o_lay = L.take(lay_cells * 2), o_win = L.take(win_cells * 8), o_jobs = L.take((size_t)n * sizeof(mosaic_job)),
                 o_rows = L.take(rpy6 ? rows * 6 * sizeof(double) : 0), o_pairs = L.take((size_t)npairs * sizeof(reg_job)),
                 o_tab = L.take((table + 1) * 8),                               // the sums and, behind them, the sample-limit flag: one download
                 o_rec = L.take(dev ? ((size_t)npairs + 1) * sizeof(dsss_reg_result) : 0);      // device path: the records and, behind them, the flag
    rc = c->mosaic_buf.reserve(c, L.off); if (rc) return rc;
    if (dev) { rc = c->mosaic_pinned.reserve(c, (size_t)npairs * sizeof(dsss_reg_result) + 8); if (rc) return rc; }
    char* B = c->mosaic_buf.as<char>();
    uint16_t* d_lay = reinterpret_cast<uint16_t*>(B + o_lay);
    unsigned long long* d_win = reinterpret_cast<unsigned long long*>(B + o_win);
    mosaic_job* d_jobs = reinterpret_cast<mosaic_job*>(B + o_jobs);
    reg_job* d_pairs = reinterpret_cast<reg_job*>(B + o_pairs);
    unsigned long long* d_tab = reinterpret_cast<unsigned long long*>(B + o_tab);
    dsss_reg_result* d_rec = reinterpret_cast<dsss_reg_result*>(B + o_rec);
    int* d_flag = dev ? reinterpret_cast<int*>(d_rec + npairs) : reinterpret_cast<int*>(d_tab + table);
    std::vector<const double*> dev_rows;
    rc = upload_rows(c, ids, n, rpy6, ping_off, reinterpret_cast<double*>(B + o_rows), dev_rows); if (rc) return rc;
    std::vector<mosaic_job> jobs(n);
    for (int i = 0; i < n; ++i) { const dsss_frame& f = c->frames[ids[i]]; jobs[i] = mosaic_job{ dev_rows[i], f.gr, f.lvl[0], f.mask, f.N, f.M, 0, 0 }; }
    HIPCHK(c, hipMemcpyAsync(d_jobs, jobs.data(), (size_t)n * sizeof(mosaic_job), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d_tab, 0, (table + 1) * 8, c->stream));
    if (dev) HIPCHK(c, hipMemsetAsync(d_flag, 0, 8, c->stream));
    // 1. mean layers: scatter into the 64-bit window, pack into the frame's resident u16 layer
    for (int i = 0; i < n; ++i) {
        if (!on_grid[i]) continue;
        const size_t wc = (size_t)wins[i].bw * wins[i].bh;
        HIPCHK(c, hipMemsetAsync(d_win, 0, wc * 8, c->stream));
        launch_scatter(c, d_jobs + i, 1, jobs[i].N, wins[i], d_win);
        hipLaunchKernelGGL(mosaic_mean_kernel, dim3((unsigned)((wc + 255) / 256)), dim3(256), 0, c->stream, d_win, wc, d_lay + lay_off[i], d_flag);
        HIPCHK(c, hipGetLastError());
    }
    // 2. all pairs in one launch
    std::vector<reg_job> pj; pj.reserve(npairs);
    long long blocks = 0;
    for (int k = 0; k < npairs; ++k) {
        const int ia = slot[pair_a[k]], ib = slot[pair_b[k]];
        if (!on_grid[ia] || !on_grid[ib]) continue;
        if (!reg_push_job(pj, &blocks, d_lay + lay_off[ia], wins[ia], d_lay + lay_off[ib], wins[ib], r, d_tab + (size_t)k * nshift * 6))
            DSSS_FAIL(c, DSSS_E_ARG, "register: %d pairs are more than one launch takes", npairs);
    }
    rc = reg_launch_corr(c, pj, blocks, d_pairs, r); if (rc) return rc;
    if (dev) {                                                                  // the records and the flag in one copy; the table stays where it is
        rc = reg_launch_peaks(c, d_tab, npairs, r, R.min_cells, p->cell, d_rec); if (rc) return rc;
        const size_t down = (size_t)npairs * sizeof(dsss_reg_result) + 8;
        HIPCHK(c, hipMemcpyAsync(c->mosaic_pinned.p, d_rec, down, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        cnt.down(down); cnt.sync();
        const dsss_reg_result* rec = c->mosaic_pinned.as<dsss_reg_result>();
        if (*reinterpret_cast<const int*>(rec + npairs)) DSSS_FAIL(c, DSSS_E_CAPACITY, "mosaic: a cell received more than 2^24 samples of one frame (cell %g too coarse)", p->cell);
        memcpy(out_host, rec, (size_t)npairs * sizeof(dsss_reg_result));
        cnt.I.tables_device = npairs; c->reg_info = cnt.I;
        return DSSS_OK;
    }
    std::vector<uint64_t> own;
    uint64_t* tab = nullptr;
    own.resize(table + 1); tab = own.data();
    HIPCHK(c, hipMemcpyAsync(tab, d_tab, (table + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    cnt.down((table + 1) * 8); cnt.sync();
    if ((int)tab[table]) DSSS_FAIL(c, DSSS_E_CAPACITY, "mosaic: a cell received more than 2^24 samples of one frame (cell %g too coarse)", p->cell);
    for (int k = 0; k < npairs; ++k) peak_of(tab + (size_t)k * nshift * 6, r, R.min_cells, p->cell, out_host + k);
    if (sums_host) memcpy(sums_host, tab, table * 8);
    cnt.I.tables_host = npairs; c->reg_info = cnt.I;
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
    size_t rows = 0;
    dsss_reg_params R; std::vector<int> slot;
    int rc = reg_check(c, ids, n, rpy6, ping_off, p, pair_a, pair_b, npairs, rp, out_host, &R, slot, &rows); if (rc) return rc;
    if (seg_pings < 1) DSSS_FAIL(c, DSSS_E_ARG, "register: seg_pings = %d", seg_pings);
    if (!nseg_host || cap < 0) DSSS_FAIL(c, DSSS_E_ARG, "register: %s", nseg_host ? "negative capacity" : "nowhere to write the number of segments");
    auto segs_of = [&](int i) { return (int)(((long long)c->frames[ids[i]].N + seg_pings - 1) / seg_pings); };
    auto seg_end = [&](int s, int N) { return (int)std::min((long long)(s + 1) * seg_pings, (long long)N); };
    long long total = 0;
    for (int k = 0; k < npairs; ++k) total += segs_of(slot[pair_b[k]]);
    if (total > 0x7fffffffll) DSSS_FAIL(c, DSSS_E_ARG, "register: %lld segments", total);
    *nseg_host = (int)total;                                                    // also when there is no room for them: the caller learns how many
    if (total > cap) DSSS_FAIL(c, DSSS_E_CAPACITY, "register: %lld segments, room for %d", total, cap);
    reg_count cnt;
    if (total == 0) { c->reg_info = cnt.I; return DSSS_OK; }
    const int nseg = (int)total;
    const bool dev = !sums_host && !dsss_switches_read().reg_peaks_host;       // the peaks on the device: nobody reads the table on the host
    std::vector<char> as_a(n, 0), as_b(n, 0);
    for (int k = 0; k < npairs; ++k) { as_a[slot[pair_a[k]]] = 1; as_b[slot[pair_b[k]]] = 1; }
    HIPCHK(c, hipSetDevice(c->device));
    const int r = R.radius, S = 2 * r + 1, nshift = S * S;
    // windows: the whole frame where it occurs as a, every segment where it occurs as b
    std::vector<mosaic_win> wins(n); std::vector<char> on_grid(n, 0); std::vector<size_t> lay_off(n, 0), seg_lay(n, 0), seg_cells(n, 0);
    std::vector<int> seg0(n, 0);                                                // a frame's first segment in sw / hseg
    std::vector<mosaic_win> sw; std::vector<mosaic_seg> hseg;
    size_t win_cells = 1, lay_cells = 0;
    for (int i = 0; i < n; ++i) {
        const dsss_frame& f = c->frames[ids[i]];
        const double* fr = rpy6 ? rpy6 + (size_t)ping_off[i] * 6 : f.h_geo;
        if (as_a[i] && reg_window(f, fr, 0, f.N, p, &wins[i])) {
            on_grid[i] = 1;
            const size_t wc = (size_t)wins[i].bw * wins[i].bh;
            win_cells = std::max(win_cells, wc);
            lay_off[i] = lay_cells; lay_cells += (wc + 127) & ~(size_t)127;    // layers start on 256 bytes
        }
        if (!as_b[i]) continue;
        seg0[i] = (int)sw.size();
        size_t cells = 0;
        for (int s = 0; s < segs_of(i); ++s) {
            mosaic_win w{ p->x0, p->y0, p->cell, p->W, p->H, 0, 0, 0, 0, p->use_mask != 0 };      // bw = 0: not on the grid
            reg_window(f, fr, s * seg_pings, seg_end(s, f.N), p, &w);
            sw.push_back(w); hseg.push_back(mosaic_seg{ w.ox, w.oy, w.bw, w.bh, (unsigned long long)cells });
            cells += ((size_t)w.bw * w.bh + 127) & ~(size_t)127;
        }
        seg_cells[i] = cells; win_cells = std::max(win_cells, cells);
        seg_lay[i] = lay_cells; lay_cells += cells;
    }
    const size_t table = (size_t)nseg * nshift * 6;
    carve L;
    const size_t o_lay = L.take(lay_cells * 2), o_win = L.take(win_cells * 8), o_jobs = L.take((size_t)n * sizeof(mosaic_job)),
                 o_rows = L.take(rpy6 ? rows * 6 * sizeof(double) : 0), o_segs = L.take(hseg.size() * sizeof(mosaic_seg)),
                 o_pairs = L.take((size_t)nseg * sizeof(reg_job)), o_cj = L.take((size_t)nseg * sizeof(cen_job)),
                 o_cen = L.take((size_t)nseg * 3 * 8), o_tab = L.take((table + 1) * 8),      // the sums and, behind them, the sample-limit flag
                 o_rec = L.take(dev ? ((size_t)nseg + 1) * sizeof(dsss_reg_result) : 0);      // device path: the records and, behind them, the flag
    rc = c->mosaic_buf.reserve(c, L.off); if (rc) return rc;
    const size_t down = dev ? (size_t)nseg * sizeof(dsss_reg_result) + 8 : (table + 1) * 8;      // what comes down behind the correlation
    rc = c->mosaic_pinned.reserve(c, down); if (rc) return rc;
    char* B = c->mosaic_buf.as<char>();
    uint16_t* d_lay = reinterpret_cast<uint16_t*>(B + o_lay);
    unsigned long long* d_win = reinterpret_cast<unsigned long long*>(B + o_win);
    mosaic_job* d_jobs = reinterpret_cast<mosaic_job*>(B + o_jobs);
    mosaic_seg* d_segs = reinterpret_cast<mosaic_seg*>(B + o_segs);
    reg_job* d_pairs = reinterpret_cast<reg_job*>(B + o_pairs);
    cen_job* d_cj = reinterpret_cast<cen_job*>(B + o_cj);
    unsigned long long* d_cen = reinterpret_cast<unsigned long long*>(B + o_cen);
    unsigned long long* d_tab = reinterpret_cast<unsigned long long*>(B + o_tab);
    dsss_reg_result* d_rec = reinterpret_cast<dsss_reg_result*>(B + o_rec);
    int* d_flag = dev ? reinterpret_cast<int*>(d_rec + nseg) : reinterpret_cast<int*>(d_tab + table);
    std::vector<const double*> dev_rows;
    rc = upload_rows(c, ids, n, rpy6, ping_off, reinterpret_cast<double*>(B + o_rows), dev_rows); if (rc) return rc;
    std::vector<mosaic_job> jobs(n);
    for (int i = 0; i < n; ++i) { const dsss_frame& f = c->frames[ids[i]]; jobs[i] = mosaic_job{ dev_rows[i], f.gr, f.lvl[0], f.mask, f.N, f.M, 0, 0 }; }
    HIPCHK(c, hipMemcpyAsync(d_jobs, jobs.data(), (size_t)n * sizeof(mosaic_job), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_segs, hseg.data(), hseg.size() * sizeof(mosaic_seg), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d_tab, 0, (table + 1) * 8, c->stream));
    if (dev) HIPCHK(c, hipMemsetAsync(d_flag, 0, 8, c->stream));
    HIPCHK(c, hipMemsetAsync(d_cen, 0, (size_t)nseg * 3 * 8, c->stream));
    // 1. mean layers: a frame's whole layer where it is an a, the layers of all its segments (one scatter, one pack) where it is a b
    const mosaic_win grid{ p->x0, p->y0, p->cell, p->W, p->H, 0, 0, 0, 0, p->use_mask != 0 };
    for (int i = 0; i < n; ++i) {
        if (on_grid[i]) {
            const size_t wc = (size_t)wins[i].bw * wins[i].bh;
            HIPCHK(c, hipMemsetAsync(d_win, 0, wc * 8, c->stream));
            launch_scatter(c, d_jobs + i, 1, jobs[i].N, wins[i], d_win);
            hipLaunchKernelGGL(mosaic_mean_kernel, dim3((unsigned)((wc + 255) / 256)), dim3(256), 0, c->stream, d_win, wc, d_lay + lay_off[i], d_flag);
            HIPCHK(c, hipGetLastError());
        }
        if (as_b[i] && seg_cells[i]) {
            const size_t wc = seg_cells[i];
            HIPCHK(c, hipMemsetAsync(d_win, 0, wc * 8, c->stream));
            launch_scatter_seg(c, d_jobs + i, jobs[i].N, grid, d_win, d_segs + seg0[i], seg_pings);
            hipLaunchKernelGGL(mosaic_mean_kernel, dim3((unsigned)((wc + 255) / 256)), dim3(256), 0, c->stream, d_win, wc, d_lay + seg_lay[i], d_flag);
            HIPCHK(c, hipGetLastError());
        }
    }
    // 2. one correlation job per (pair, segment), all in one launch; the rows are laid out here, by pair and then by segment
    memset(out_host, 0, (size_t)nseg * sizeof(dsss_reg_seg));
    std::vector<reg_job> pj; pj.reserve(nseg);
    std::vector<int> row_a(nseg), row_g(nseg);                                  // a row's frame a (index in ids) and its segment in sw / hseg
    long long blocks = 0;
    int row = 0;
    for (int k = 0; k < npairs; ++k) {
        const int ia = slot[pair_a[k]], ib = slot[pair_b[k]];
        const int Nb = c->frames[ids[ib]].N;
        for (int s = 0; s < segs_of(ib); ++s, ++row) {
            dsss_reg_seg& o = out_host[row];
            o.pair = k; o.seg = s; o.p0 = s * seg_pings; o.p1 = seg_end(s, Nb);
            const int g = seg0[ib] + s;
            row_a[row] = ia; row_g[row] = g;
            if (!on_grid[ia] || sw[g].bw == 0) continue;
            if (!reg_push_job(pj, &blocks, d_lay + lay_off[ia], wins[ia], d_lay + seg_lay[ib] + hseg[g].off, sw[g], r, d_tab + (size_t)row * nshift * 6))
                DSSS_FAIL(c, DSSS_E_ARG, "register: %d segments are more than one launch takes", nseg);
        }
    }
    rc = reg_launch_corr(c, pj, blocks, d_pairs, r); if (rc) return rc;
    if (dev) { rc = reg_launch_peaks(c, d_tab, nseg, r, R.min_cells, p->cell, d_rec); if (rc) return rc; }
    const uint64_t* tab = c->mosaic_pinned.as<uint64_t>();                      // host path: the table and the flag
    const dsss_reg_result* rec = c->mosaic_pinned.as<dsss_reg_result>();        // device path: the records and the flag
    HIPCHK(c, hipMemcpyAsync(c->mosaic_pinned.p, dev ? (const void*)d_rec : (const void*)d_tab, down, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    cnt.down(down); cnt.sync();
    if (dev ? *reinterpret_cast<const int*>(rec + nseg) : (int)tab[table])
        DSSS_FAIL(c, DSSS_E_CAPACITY, "mosaic: a cell received more than 2^24 samples of one frame (cell %g too coarse)", p->cell);
    (dev ? cnt.I.tables_device : cnt.I.tables_host) = nseg;
    // 3. the peaks (the device's records, or decided here from the table), then the centroid sums of the rows that have one: one launch, one download
    std::vector<cen_job> cj;
    long long cblocks = 0;
    for (row = 0; row < nseg; ++row) {
        dsss_reg_result& q = out_host[row].r;
        if (dev) q = rec[row]; else peak_of(tab + (size_t)row * nshift * 6, r, R.min_cells, p->cell, &q);
        if (!(q.zncc > -2.0)) continue;                                         // no usable shift: sx = sy = 0
        if (!cen_push_job(cj, &cblocks, d_lay + lay_off[row_a[row]], wins[row_a[row]], d_lay + seg_lay[slot[pair_b[out_host[row].pair]]] + hseg[row_g[row]].off,
                          sw[row_g[row]], q, d_cen + (size_t)row * 3))
            DSSS_FAIL(c, DSSS_E_ARG, "register: %d segments are more than one launch takes", nseg);
    }
    if (!cj.empty()) {
        std::vector<uint64_t> cen((size_t)nseg * 3);
        rc = reg_launch_centroids(c, cj, cblocks, d_cj, d_cen, cen, cnt); if (rc) return rc;
        for (row = 0; row < nseg; ++row) {
            dsss_reg_seg& o = out_host[row];
            if (!(o.r.zncc > -2.0)) continue;
            if ((int64_t)cen[(size_t)row * 3] != o.r.n)
                DSSS_FAIL(c, DSSS_E_NUMERIC, "register: internal error, row %d has %lld cells at its peak and %lld in its centroid", row,
                          (long long)o.r.n, (long long)cen[(size_t)row * 3]);
            o.sx = (int64_t)cen[(size_t)row * 3 + 1]; o.sy = (int64_t)cen[(size_t)row * 3 + 2];
        }
    }
    if (sums_host) memcpy(sums_host, tab, table * 8);
    c->reg_info = cnt.I;
    return DSSS_OK;
}

void dsss_reg_edge_params_default(dsss_reg_edge_params* e) { if (e) { e->min_zncc = 0.5; e->sigma_xy_cells = 1.0; e->sigma_z = 10.0; e->sigma_rot = 1.0; } }

int dsss_register_edge(const dsss_reg_seg* s, const dsss_mosaic_params* grid, const double* rows_a, int Na, int base_a,
                       const double* rows_b, int Nb, int base_b, const dsss_reg_edge_params* ep, dsss_lc_edge* edge)
{
    dsss_reg_edge_params E; dsss_reg_edge_params_default(&E);
    if (ep) E = *ep;
    return edge_of(s, grid, rows_a, Na, base_a, rows_b, Nb, base_b, E, 0.0, 0.0, E.sigma_rot, edge);
}

int dsss_mosaic_register_edges(dsss_ctx* c, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params* p,
                               const int* pair_a, const int* pair_b, const dsss_reg_seg* segs, int nsegs, const dsss_reg_edge_params* ep,
                               dsss_lc_edge* edges_host, int32_t* edge_seg_host, int cap, int* n_edges)
{
    return edges_loop(c, ids, n, rpy6, ping_off, p, pair_a, pair_b, segs != nullptr, nsegs, edges_host, edge_seg_host, cap, n_edges,
                      [&](int k) -> const dsss_reg_seg& { return segs[k]; },
                      [&](int k, const double* ra, int Na, int ba, const double* rb, int Nb, int bb, dsss_lc_edge* e) {
                          return dsss_register_edge(segs + k, p, ra, Na, ba, rb, Nb, bb, ep, e); });
}

// ---- dense loop closures with a yaw fan
void dsss_reg_yaw_params_default(dsss_reg_yaw_params* y) { if (y) { y->nyaw = 1; y->pad_ = 0; y->step = 0.01; } }

int dsss_register_rotate_rows(const double* rows_b, int Nb, int p0, int p1, double theta, double* out)
{
    if (!rows_b || !out || p0 < 0 || p0 >= p1 || p1 > Nb || !std::isfinite(theta)) return DSSS_E_ARG;
    rotate_rows(rows_b, p0, p1, theta, out);
    return DSSS_OK;
}

int dsss_register_yaw_peak(const dsss_reg_result* per_angle, int nyaw, double step, int32_t* k, int32_t* yaw_on_border, double* theta, double* theta_hat)
{
    if (!per_angle || !k || !yaw_on_border || !theta || !theta_hat || !fan_ok(nyaw, step)) return DSSS_E_ARG;
    yaw_peak_of(per_angle, nyaw, step, k, yaw_on_border, theta, theta_hat);
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
    size_t rows = 0;
    dsss_reg_params R; std::vector<int> slot;
    int rc = reg_check(c, ids, n, rpy6, ping_off, p, pair_a, pair_b, npairs, rp, out_host, &R, slot, &rows); if (rc) return rc;
    if (seg_pings < 1) DSSS_FAIL(c, DSSS_E_ARG, "register: seg_pings = %d", seg_pings);
    if (!nseg_host || cap < 0) DSSS_FAIL(c, DSSS_E_ARG, "register: %s", nseg_host ? "negative capacity" : "nowhere to write the number of segments");
    dsss_reg_yaw_params Y; dsss_reg_yaw_params_default(&Y);
    if (yp) Y = *yp;
    if (!fan_ok(Y.nyaw, Y.step)) DSSS_FAIL(c, DSSS_E_ARG, "register: a fan of %d angles, %g rad apart (an odd number up to %d, a positive step)", Y.nyaw, Y.step, REG_MAX_YAW);
    const int nyaw = Y.nyaw, mid = (nyaw - 1) / 2;
    auto segs_of = [&](int i) { return (int)(((long long)c->frames[ids[i]].N + seg_pings - 1) / seg_pings); };
    auto seg_end = [&](int s, int N) { return (int)std::min((long long)(s + 1) * seg_pings, (long long)N); };
    long long total = 0;
    for (int k = 0; k < npairs; ++k) {
        const int ib = slot[pair_b[k]];
        if ((long long)c->frames[ids[ib]].N * nyaw > 0x7fffffffll) DSSS_FAIL(c, DSSS_E_ARG, "register: frame %d has %d pings, too many for %d angles in one launch", ids[ib], c->frames[ids[ib]].N, nyaw);
        total += segs_of(ib);
    }
    if (total > 0x7fffffffll) DSSS_FAIL(c, DSSS_E_ARG, "register: %lld segments", total);
    *nseg_host = (int)total;                                                    // also when there is no room for them: the caller learns how many
    if (total > cap) DSSS_FAIL(c, DSSS_E_CAPACITY, "register: %lld segments, room for %d", total, cap);
    reg_count cnt;
    if (total == 0) { c->reg_info = cnt.I; return DSSS_OK; }
    const int nseg = (int)total;
    const bool dev = !sums_host && !dsss_switches_read().reg_peaks_host;       // the peaks on the device: nobody reads the table on the host
    std::vector<char> as_a(n, 0), as_b(n, 0);
    for (int k = 0; k < npairs; ++k) { as_a[slot[pair_a[k]]] = 1; as_b[slot[pair_b[k]]] = 1; }
    const int r = R.radius, S = 2 * r + 1, nshift = S * S;
    // windows: the whole frame where it occurs as a, every (segment, angle) where it occurs as b
    std::vector<mosaic_win> wins(n); std::vector<char> on_grid(n, 0); std::vector<size_t> lay_off(n, 0), fan_lay(n, 0), fan_cells(n, 0);
    std::vector<size_t> fan0(n, 0);                                             // a frame's first entry in sw / hfan; (segment s, angle k) is entry s nyaw + k behind it
    std::vector<mosaic_win> sw; std::vector<mosaic_fan> hfan;
    std::vector<double> rot;
    size_t win_cells = 1, lay_cells = 0;
    for (int i = 0; i < n; ++i) {
        const dsss_frame& f = c->frames[ids[i]];
        const double* fr = rpy6 ? rpy6 + (size_t)ping_off[i] * 6 : f.h_geo;
        if (as_a[i] && reg_window(f, fr, 0, f.N, p, &wins[i])) {
            on_grid[i] = 1;
            const size_t wc = (size_t)wins[i].bw * wins[i].bh;
            win_cells = std::max(win_cells, wc);
            lay_off[i] = lay_cells; lay_cells += (wc + 127) & ~(size_t)127;    // layers start on 256 bytes
        }
        if (!as_b[i]) continue;
        fan0[i] = sw.size();
        size_t cells = 0;
        for (int s = 0; s < segs_of(i); ++s) {
            const int p0 = s * seg_pings, p1 = seg_end(s, f.N);
            const double* piv = fr + (size_t)(((long long)p0 + p1) / 2) * 6;
            rot.resize((size_t)(p1 - p0) * 6);
            for (int k = 0; k < nyaw; ++k) {
                mosaic_win w{ p->x0, p->y0, p->cell, p->W, p->H, 0, 0, 0, 0, p->use_mask != 0 };  // bw = 0: not on the grid
                mosaic_fan F; F.cx = piv[3]; F.cy = piv[4]; F.theta = fan_theta(k, nyaw, Y.step);
                dsss_sincos(F.theta, &F.s, &F.c);
                rotate_rows(fr, p0, p1, F.theta, rot.data());
                reg_window(f, rot.data(), 0, p1 - p0, p, &w);
                F.ox = w.ox; F.oy = w.oy; F.bw = w.bw; F.bh = w.bh; F.off = (unsigned long long)cells;
                sw.push_back(w); hfan.push_back(F);
                cells += ((size_t)w.bw * w.bh + 127) & ~(size_t)127;
            }
        }
        fan_cells[i] = cells; win_cells = std::max(win_cells, cells);
        fan_lay[i] = lay_cells; lay_cells += cells;
    }
    const size_t table = (size_t)nseg * nshift * 6;                             // one angle's sums
    HIPCHK(c, hipSetDevice(c->device));
    carve L;
    const size_t o_lay = L.take(lay_cells * 2), o_win = L.take(win_cells * 8), o_jobs = L.take((size_t)n * sizeof(mosaic_job)),
                 o_rows = L.take(rpy6 ? rows * 6 * sizeof(double) : 0), o_fan = L.take(hfan.size() * sizeof(mosaic_fan)),
                 o_pairs = L.take((size_t)nseg * sizeof(reg_job)), o_cj = L.take((size_t)nseg * sizeof(cen_job)),
                 o_cen = L.take((size_t)nseg * 3 * 8), o_tab = L.take((table + 1) * 8),      // the sums and, behind them, the sample-limit flag
                 o_rec = L.take(dev ? ((size_t)nseg + 1) * sizeof(dsss_reg_result) : 0);      // device path: one angle's records and, behind them, the flag
    rc = c->mosaic_buf.reserve(c, L.off); if (rc) return rc;
    const size_t down = dev ? (size_t)nseg * sizeof(dsss_reg_result) + 8 : (table + 1) * 8;      // what comes down per pass
    rc = c->mosaic_pinned.reserve(c, down); if (rc) return rc;
    char* B = c->mosaic_buf.as<char>();
    uint16_t* d_lay = reinterpret_cast<uint16_t*>(B + o_lay);
    unsigned long long* d_win = reinterpret_cast<unsigned long long*>(B + o_win);
    mosaic_job* d_jobs = reinterpret_cast<mosaic_job*>(B + o_jobs);
    mosaic_fan* d_fan = reinterpret_cast<mosaic_fan*>(B + o_fan);
    reg_job* d_pairs = reinterpret_cast<reg_job*>(B + o_pairs);
    cen_job* d_cj = reinterpret_cast<cen_job*>(B + o_cj);
    unsigned long long* d_cen = reinterpret_cast<unsigned long long*>(B + o_cen);
    unsigned long long* d_tab = reinterpret_cast<unsigned long long*>(B + o_tab);
    dsss_reg_result* d_rec = reinterpret_cast<dsss_reg_result*>(B + o_rec);
    int* d_flag = dev ? reinterpret_cast<int*>(d_rec + nseg) : reinterpret_cast<int*>(d_tab + table);
    // the rows and every pass's jobs, laid out by pair and then by segment, before anything is launched: what one launch cannot take
    // is refused here.  A row's centroid region lies inside the correlation region of its angle, so the largest of those bounds it.
    memset(out_host, 0, (size_t)nseg * sizeof(dsss_reg_seg_yaw));
    std::vector<std::vector<reg_job>> pj(nyaw);
    std::vector<long long> blocks(nyaw, 0);
    std::vector<int> row_a(nseg); std::vector<size_t> row_g(nseg);              // a row's frame a (index in ids) and its segment's first entry in sw / hfan
    long long cen_bound = 0;
    int row = 0;
    for (int k = 0; k < npairs; ++k) {
        const int ia = slot[pair_a[k]], ib = slot[pair_b[k]];
        const int Nb = c->frames[ids[ib]].N;
        for (int s = 0; s < segs_of(ib); ++s, ++row) {
            dsss_reg_seg& o = out_host[row].s;
            o.pair = k; o.seg = s; o.p0 = s * seg_pings; o.p1 = seg_end(s, Nb);
            const size_t g = fan0[ib] + (size_t)s * nyaw;
            row_a[row] = ia; row_g[row] = g;
            if (!on_grid[ia]) continue;
            long long most = 0;
            for (int a = 0; a < nyaw; ++a) {
                if (sw[g + a].bw == 0) continue;
                const size_t before = pj[a].size();
                if (!reg_push_job(pj[a], &blocks[a], d_lay + lay_off[ia], wins[ia], d_lay + fan_lay[ib] + hfan[g + a].off, sw[g + a], r, d_tab + (size_t)row * nshift * 6))
                    DSSS_FAIL(c, DSSS_E_ARG, "register: %d segments are more than one launch takes", nseg);
                if (pj[a].size() == before) continue;
                const reg_job& J = pj[a].back();
                most = std::max(most, (long long)((J.rx1 - J.rx0) / CEN_TW + 2) * ((J.ry1 - J.ry0) / CEN_TH + 2));
            }
            cen_bound += most;
        }
    }
    if (cen_bound > 0x7fffffffll) DSSS_FAIL(c, DSSS_E_ARG, "register: %d segments are more than one launch takes", nseg);
    std::vector<const double*> dev_rows;
    rc = upload_rows(c, ids, n, rpy6, ping_off, reinterpret_cast<double*>(B + o_rows), dev_rows); if (rc) return rc;
    std::vector<mosaic_job> jobs(n);
    for (int i = 0; i < n; ++i) { const dsss_frame& f = c->frames[ids[i]]; jobs[i] = mosaic_job{ dev_rows[i], f.gr, f.lvl[0], f.mask, f.N, f.M, 0, 0 }; }
    HIPCHK(c, hipMemcpyAsync(d_jobs, jobs.data(), (size_t)n * sizeof(mosaic_job), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_fan, hfan.data(), hfan.size() * sizeof(mosaic_fan), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d_flag, 0, 8, c->stream));
    HIPCHK(c, hipMemsetAsync(d_cen, 0, (size_t)nseg * 3 * 8, c->stream));
    // 1. mean layers: a frame's whole layer where it is an a, the layers of all its segments under all angles (one scatter, one pack) where it is a b
    const mosaic_win grid{ p->x0, p->y0, p->cell, p->W, p->H, 0, 0, 0, 0, p->use_mask != 0 };
    for (int i = 0; i < n; ++i) {
        if (on_grid[i]) {
            const size_t wc = (size_t)wins[i].bw * wins[i].bh;
            HIPCHK(c, hipMemsetAsync(d_win, 0, wc * 8, c->stream));
            launch_scatter(c, d_jobs + i, 1, jobs[i].N, wins[i], d_win);
            hipLaunchKernelGGL(mosaic_mean_kernel, dim3((unsigned)((wc + 255) / 256)), dim3(256), 0, c->stream, d_win, wc, d_lay + lay_off[i], d_flag);
            HIPCHK(c, hipGetLastError());
        }
        if (as_b[i] && fan_cells[i]) {
            const size_t wc = fan_cells[i];
            HIPCHK(c, hipMemsetAsync(d_win, 0, wc * 8, c->stream));
            hipLaunchKernelGGL(mosaic_scatter_fan_kernel, dim3((unsigned)jobs[i].N * (unsigned)nyaw), dim3(256), 0, c->stream, d_jobs + i, grid, d_win,
                               d_fan + fan0[i], seg_pings, nyaw);
            hipLaunchKernelGGL(mosaic_mean_kernel, dim3((unsigned)((wc + 255) / 256)), dim3(256), 0, c->stream, d_win, wc, d_lay + fan_lay[i], d_flag);
            HIPCHK(c, hipGetLastError());
        }
    }
    // 2. one pass per angle: the table cleared, one correlation job per (pair, segment), one download, the records of the angle
    const uint64_t* tab = c->mosaic_pinned.as<uint64_t>();                      // host path: the table and the flag
    const dsss_reg_result* rec = c->mosaic_pinned.as<dsss_reg_result>();        // device path: the records and the flag
    std::vector<dsss_reg_result> per((size_t)nseg * nyaw);
    for (int a = 0; a < nyaw; ++a) {
        HIPCHK(c, hipMemsetAsync(d_tab, 0, table * 8, c->stream));
        rc = reg_launch_corr(c, pj[a], blocks[a], d_pairs, r); if (rc) return rc;
        if (dev) { rc = reg_launch_peaks(c, d_tab, nseg, r, R.min_cells, p->cell, d_rec); if (rc) return rc; }
        HIPCHK(c, hipMemcpyAsync(c->mosaic_pinned.p, dev ? (const void*)d_rec : (const void*)d_tab, down, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        cnt.down(down); cnt.sync();
        if (dev ? *reinterpret_cast<const int*>(rec + nseg) : (int)tab[table])
            DSSS_FAIL(c, DSSS_E_CAPACITY, "mosaic: a cell received more than 2^24 samples of one frame (cell %g too coarse)", p->cell);
        (dev ? cnt.I.tables_device : cnt.I.tables_host) += nseg;
        for (row = 0; row < nseg; ++row) {
            if (dev) { per[(size_t)row * nyaw + a] = rec[row]; continue; }
            peak_of(tab + (size_t)row * nshift * 6, r, R.min_cells, p->cell, &per[(size_t)row * nyaw + a]);
            if (sums_host) memcpy(sums_host + ((size_t)row * nyaw + a) * nshift * 6, tab + (size_t)row * nshift * 6, (size_t)nshift * 6 * 8);
        }
    }
    // 3. the angle of every row on the host, then the centroid sums of the rows that have one under that angle: one launch, one download
    std::vector<cen_job> cj;
    long long cblocks = 0;
    for (row = 0; row < nseg; ++row) {
        dsss_reg_seg_yaw& o = out_host[row];
        const dsss_reg_result* z = per.data() + (size_t)row * nyaw;
        yaw_peak_of(z, nyaw, Y.step, &o.k, &o.yaw_on_border, &o.theta, &o.theta_hat);
        o.s.r = z[o.k]; o.zncc_k0 = z[mid].zncc;
        if (!(o.s.r.zncc > -2.0)) continue;                                     // no usable shift under any angle: sx = sy = 0
        const size_t g = row_g[row] + o.k;
        if (!cen_push_job(cj, &cblocks, d_lay + lay_off[row_a[row]], wins[row_a[row]], d_lay + fan_lay[slot[pair_b[o.s.pair]]] + hfan[g].off, sw[g], o.s.r,
                          d_cen + (size_t)row * 3))
            DSSS_FAIL(c, DSSS_E_NUMERIC, "register: internal error, the centroid of %d segments takes more workgroups than was bounded", nseg);
    }
    if (!cj.empty()) {
        std::vector<uint64_t> cen((size_t)nseg * 3);
        rc = reg_launch_centroids(c, cj, cblocks, d_cj, d_cen, cen, cnt); if (rc) return rc;
        for (row = 0; row < nseg; ++row) {
            dsss_reg_seg& o = out_host[row].s;
            if (!(o.r.zncc > -2.0)) continue;
            if ((int64_t)cen[(size_t)row * 3] != o.r.n)
                DSSS_FAIL(c, DSSS_E_NUMERIC, "register: internal error, row %d has %lld cells at its peak and %lld in its centroid", row,
                          (long long)o.r.n, (long long)cen[(size_t)row * 3]);
            o.sx = (int64_t)cen[(size_t)row * 3 + 1]; o.sy = (int64_t)cen[(size_t)row * 3 + 2];
        }
    }
    c->reg_info = cnt.I;
    return DSSS_OK;
}

void dsss_reg_edge_yaw_params_default(dsss_reg_edge_yaw_params* e)
{
    if (e) { dsss_reg_edge_params_default(&e->e); dsss_reg_yaw_params_default(&e->fan); e->sigma_yaw_steps = 1.0; }
}

int dsss_register_edge_yaw(const dsss_reg_seg_yaw* s, const dsss_mosaic_params* grid, const double* rows_a, int Na, int base_a,
                           const double* rows_b, int Nb, int base_b, const dsss_reg_edge_yaw_params* ep, dsss_lc_edge* edge)
{
    dsss_reg_edge_yaw_params E; dsss_reg_edge_yaw_params_default(&E);
    if (ep) E = *ep;
    if (!s || !fan_ok(E.fan.nyaw, E.fan.step) || !(E.sigma_yaw_steps > 0.0) || !std::isfinite(E.sigma_yaw_steps)) return DSSS_E_ARG;
    const double s_yaw = E.fan.nyaw == 1 ? E.e.sigma_rot : E.sigma_yaw_steps * E.fan.step;
    // the row's own acceptance comes first in edge_of; a fan row on the border of the fan is rejected after it was found valid
    dsss_lc_edge e;
    const int rc = edge_of(&s->s, grid, rows_a, Na, base_a, rows_b, Nb, base_b, E.e, s->theta, s->theta_hat, s_yaw, edge ? &e : nullptr);
    if (rc != 1) return rc;
    if (s->yaw_on_border != 0) return 0;
    *edge = e;
    return 1;
}

int dsss_mosaic_register_edges_yaw(dsss_ctx* c, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params* p,
                                   const int* pair_a, const int* pair_b, const dsss_reg_seg_yaw* segs, int nsegs, const dsss_reg_edge_yaw_params* ep,
                                   dsss_lc_edge* edges_host, int32_t* edge_seg_host, int cap, int* n_edges)
{
    return edges_loop(c, ids, n, rpy6, ping_off, p, pair_a, pair_b, segs != nullptr, nsegs, edges_host, edge_seg_host, cap, n_edges,
                      [&](int k) -> const dsss_reg_seg& { return segs[k].s; },
                      [&](int k, const double* ra, int Na, int ba, const double* rb, int Nb, int bb, dsss_lc_edge* e) {
                          return dsss_register_edge_yaw(segs + k, p, ra, Na, ba, rb, Nb, bb, ep, e); });
}

// ---- dense loop closures over a cell pyramid
void dsss_reg_pyr_params_default(dsss_reg_pyr_params* q) { if (q) { q->levels = 1; q->refine = 3; } }

int dsss_register_pyr_step(const uint64_t* sums, int radius, int min_cells, double cell, int level, int cx, int cy,
                           dsss_reg_result* out, int32_t* usable, int32_t* ncx, int32_t* ncy)
{
    if (!sums || !out || !usable || !ncx || !ncy || radius < 0 || radius > REG_MAX_RADIUS || min_cells < 1 || !(cell > 0.0) || !std::isfinite(cell) ||
        level < 0 || level >= PYR_MAX_LEVELS || cx < -PYR_MAX_CENTRE || cx > PYR_MAX_CENTRE || cy < -PYR_MAX_CENTRE || cy > PYR_MAX_CENTRE) return DSSS_E_ARG;
    pyr_step_of(sums, radius, min_cells, cell, level, cx, cy, out, usable, ncx, ncy);
    return DSSS_OK;
}

// dsss_mosaic_register_segments coarse to fine.  Per frame: ONE memset, the unchanged scatter kernels into the accumulators of its whole
// window (where it is an a) and of all its segments (where it is a b), and ONE mosaic_pyr_kernel over all those areas that writes
// the layers of every level; the layers of all levels stay resident.  Per level, from the top: mosaic_corr_kernel with one job per row
// that is still alive (the segment's window moved by minus the row's centre), one download -- of the records of the live rows, whose
// tables then lie one behind the other (mosaic_peak_kernel with the level's radius, min_cells and cell), or of that level's tables of
// all rows when the sums are asked for -- and the level rule on the host (pyr_step_of; on the device path its second part, pyr_centre_of).  mosaic_centroid_kernel runs once, at the total shift, for the rows that finished at level 0.  What one
// launch cannot take is bounded and refused before anything is launched.
int dsss_mosaic_register_segments_pyr(dsss_ctx* c, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params* p,
                                      const int* pair_a, const int* pair_b, int npairs, int seg_pings, const dsss_reg_params* rp,
                                      const dsss_reg_pyr_params* pp, dsss_reg_seg_pyr* out_host, int cap, int* nseg_host, uint64_t* sums_host)
{
    if (!c) return DSSS_E_ARG;
    size_t rows = 0;
    dsss_reg_params R; std::vector<int> slot;
    int rc = reg_check(c, ids, n, rpy6, ping_off, p, pair_a, pair_b, npairs, rp, out_host, &R, slot, &rows); if (rc) return rc;
    if (seg_pings < 1) DSSS_FAIL(c, DSSS_E_ARG, "register: seg_pings = %d", seg_pings);
    if (!nseg_host || cap < 0) DSSS_FAIL(c, DSSS_E_ARG, "register: %s", nseg_host ? "negative capacity" : "nowhere to write the number of segments");
    dsss_reg_pyr_params P; dsss_reg_pyr_params_default(&P);
    if (pp) P = *pp;
    if (!pyr_ok(P)) DSSS_FAIL(c, DSSS_E_ARG, "register: a pyramid of %d levels refined within %d cells (1..%d levels, 1..%d cells)", P.levels, P.refine, PYR_MAX_LEVELS, REG_MAX_RADIUS);
    const int L = P.levels;
    auto segs_of = [&](int i) { return (int)(((long long)c->frames[ids[i]].N + seg_pings - 1) / seg_pings); };
    auto seg_end = [&](int s, int N) { return (int)std::min((long long)(s + 1) * seg_pings, (long long)N); };
    long long total = 0;
    for (int k = 0; k < npairs; ++k) total += segs_of(slot[pair_b[k]]);
    if (total > 0x7fffffffll) DSSS_FAIL(c, DSSS_E_ARG, "register: %lld segments", total);
    *nseg_host = (int)total;                                                    // also when there is no room for them: the caller learns how many
    if (total > cap) DSSS_FAIL(c, DSSS_E_CAPACITY, "register: %lld segments, room for %d", total, cap);
    reg_count cnt;
    if (total == 0) { c->reg_info = cnt.I; return DSSS_OK; }
    const int nseg = (int)total;
    const bool dev = !sums_host && !dsss_switches_read().reg_peaks_host;       // the peaks on the device: nobody reads the table on the host
    std::vector<char> as_a(n, 0), as_b(n, 0);
    for (int k = 0; k < npairs; ++k) { as_a[slot[pair_a[k]]] = 1; as_b[slot[pair_b[k]]] = 1; }
    auto radius_of = [&](int l) { return l == L - 1 ? R.radius : P.refine; };
    auto nshift_of = [&](int l) { const int S = 2 * radius_of(l) + 1; return (size_t)S * S; };
    // areas: the whole frame where it occurs as a, every segment where it occurs as b; an area's accumulators lie behind the frame's
    // first, its layers of all levels in d_lay
    struct area_lay { size_t off[PYR_MAX_LEVELS]; };
    std::vector<mosaic_win> wins(n); std::vector<char> on_grid(n, 0); std::vector<area_lay> a_lay(n);
    std::vector<int> seg0(n, 0), job0(n, 0), njobs(n, 0);                       // a frame's first segment in sw / hseg, its areas in hpj
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
            lay_cells += ((size_t)q.bw * q.bh + 127) & ~(size_t)127;            // layers start on 256 bytes
        }
        J.tiles_x = (w.ox + w.bw - 1 - J.bx0) / PYR_TW + 1; J.blk0 = (int)pyr_blocks[i];
        pyr_blocks[i] += (long long)J.tiles_x * ((w.oy + w.bh - 1 - J.by0) / PYR_TH + 1);
        if (pyr_blocks[i] <= 0x7fffffffll) { hpj.push_back(J); ++njobs[i]; }   // (more is refused below, before anything is launched)
    };
    for (int i = 0; i < n; ++i) {
        const dsss_frame& f = c->frames[ids[i]];
        const double* fr = rpy6 ? rpy6 + (size_t)ping_off[i] * 6 : f.h_geo;
        job0[i] = (int)hpj.size();
        if (as_a[i] && reg_window(f, fr, 0, f.N, p, &wins[i])) {
            on_grid[i] = 1;
            add_area(i, wins[i], 0, &a_lay[i]);
            a_cells[i] = ((size_t)wins[i].bw * wins[i].bh + 127) & ~(size_t)127;
        }
        size_t cells = 0;
        if (as_b[i]) {
            seg0[i] = (int)sw.size();
            for (int s = 0; s < segs_of(i); ++s) {
                mosaic_win w{ p->x0, p->y0, p->cell, p->W, p->H, 0, 0, 0, 0, p->use_mask != 0 };  // bw = 0: not on the grid
                area_lay al{};
                if (reg_window(f, fr, s * seg_pings, seg_end(s, f.N), p, &w)) add_area(i, w, a_cells[i] + cells, &al);
                sw.push_back(w); seg_lay.push_back(al); hseg.push_back(mosaic_seg{ w.ox, w.oy, w.bw, w.bh, (unsigned long long)cells });
                cells += ((size_t)w.bw * w.bh + 127) & ~(size_t)127;
            }
        }
        acc_cells[i] = a_cells[i] + cells; win_cells = std::max(win_cells, acc_cells[i]);
        if (pyr_blocks[i] > 0x7fffffffll) DSSS_FAIL(c, DSSS_E_ARG, "register: the areas of frame %d are more than one launch takes", ids[i]);
    }
    // the rows, by pair and then by segment, and what the launches of every level and of the centroid can need at most: a level's
    // region lies inside the segment's window of that level dilated by the radius, the centroid's inside the segment's fine window
    memset(out_host, 0, (size_t)nseg * sizeof(dsss_reg_seg_pyr));
    std::vector<int> row_a(nseg), row_b(nseg), row_g(nseg);                     // a row's frames (index in ids) and its segment in sw / hseg
    {
        long long bound[PYR_MAX_LEVELS] = { 0, 0, 0, 0 }, cen_bound = 0;
        int row = 0;
        for (int k = 0; k < npairs; ++k) {
            const int ia = slot[pair_a[k]], ib = slot[pair_b[k]];
            const int Nb = c->frames[ids[ib]].N;
            for (int s = 0; s < segs_of(ib); ++s, ++row) {
                dsss_reg_seg_pyr& o = out_host[row];
                o.s.pair = k; o.s.seg = s; o.s.p0 = s * seg_pings; o.s.p1 = seg_end(s, Nb);
                o.level = -1;
                for (int l = 0; l < PYR_MAX_LEVELS; ++l) o.lz[l] = -2.0;
                const int g = seg0[ib] + s;
                row_a[row] = ia; row_b[row] = ib; row_g[row] = g;
                if (!on_grid[ia] || sw[g].bw == 0) continue;
                for (int l = 0; l < L; ++l) {
                    const mosaic_win A = pyr_window(wins[ia], l, 0, 0), Bw = pyr_window(sw[g], l, 0, 0);
                    const long long w = std::min(A.bw, Bw.bw + 2 * radius_of(l)), h = std::min(A.bh, Bw.bh + 2 * radius_of(l));
                    bound[l] += (((w - 1) / REG_TILE + 1) + REG_STRIP - 1) / REG_STRIP * ((h - 1) / REG_TILE + 1);
                }
                cen_bound += (long long)((std::min(wins[ia].bw, sw[g].bw) - 1) / CEN_TW + 1) * ((std::min(wins[ia].bh, sw[g].bh) - 1) / CEN_TH + 1);
            }
        }
        for (int l = 0; l < L; ++l)
            if (bound[l] > 0x7fffffffll || cen_bound > 0x7fffffffll) DSSS_FAIL(c, DSSS_E_ARG, "register: %d segments are more than one launch takes", nseg);
    }
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nshift_max = std::max(nshift_of(L - 1), nshift_of(0));
    const size_t table_max = (size_t)nseg * nshift_max * 6;
    carve Cv;
    const size_t o_lay = Cv.take(lay_cells * 2), o_win = Cv.take(win_cells * 8), o_jobs = Cv.take((size_t)n * sizeof(mosaic_job)),
                 o_rows = Cv.take(rpy6 ? rows * 6 * sizeof(double) : 0), o_segs = Cv.take(hseg.size() * sizeof(mosaic_seg)),
                 o_pj = Cv.take(hpj.size() * sizeof(pyr_job)), o_pairs = Cv.take((size_t)nseg * sizeof(reg_job)), o_cj = Cv.take((size_t)nseg * sizeof(cen_job)),
                 o_cen = Cv.take((size_t)nseg * 3 * 8), o_tab = Cv.take((1 + table_max) * 8),      // the sample-limit flag and, behind it, one level's sums
                 o_rec = Cv.take(dev ? ((size_t)nseg + 1) * sizeof(dsss_reg_result) : 0);      // device path: the flag in the last 8 bytes of a first record's room, behind it one level's records
    rc = c->mosaic_buf.reserve(c, Cv.off); if (rc) return rc;
    rc = c->mosaic_pinned.reserve(c, dev ? 8 + (size_t)nseg * sizeof(dsss_reg_result) : (1 + table_max) * 8); if (rc) return rc;
    char* B = c->mosaic_buf.as<char>();
    uint16_t* d_lay = reinterpret_cast<uint16_t*>(B + o_lay);
    unsigned long long* d_win = reinterpret_cast<unsigned long long*>(B + o_win);
    mosaic_job* d_jobs = reinterpret_cast<mosaic_job*>(B + o_jobs);
    mosaic_seg* d_segs = reinterpret_cast<mosaic_seg*>(B + o_segs);
    pyr_job* d_pj = reinterpret_cast<pyr_job*>(B + o_pj);
    reg_job* d_pairs = reinterpret_cast<reg_job*>(B + o_pairs);
    cen_job* d_cj = reinterpret_cast<cen_job*>(B + o_cj);
    unsigned long long* d_cen = reinterpret_cast<unsigned long long*>(B + o_cen);
    unsigned long long* d_tab = reinterpret_cast<unsigned long long*>(B + o_tab) + 1;
    dsss_reg_result* d_rec = reinterpret_cast<dsss_reg_result*>(B + o_rec) + 1;
    int* d_flag = dev ? reinterpret_cast<int*>(reinterpret_cast<char*>(d_rec) - 8) : reinterpret_cast<int*>(B + o_tab);
    std::vector<const double*> dev_rows;
    rc = upload_rows(c, ids, n, rpy6, ping_off, reinterpret_cast<double*>(B + o_rows), dev_rows); if (rc) return rc;
    std::vector<mosaic_job> jobs(n);
    for (int i = 0; i < n; ++i) { const dsss_frame& f = c->frames[ids[i]]; jobs[i] = mosaic_job{ dev_rows[i], f.gr, f.lvl[0], f.mask, f.N, f.M, 0, 0 }; }
    HIPCHK(c, hipMemcpyAsync(d_jobs, jobs.data(), (size_t)n * sizeof(mosaic_job), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_segs, hseg.data(), hseg.size() * sizeof(mosaic_seg), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_pj, hpj.data(), hpj.size() * sizeof(pyr_job), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d_flag, 0, 8, c->stream));
    HIPCHK(c, hipMemsetAsync(d_cen, 0, (size_t)nseg * 3 * 8, c->stream));
    // 1. the layers of all levels: per frame one memset, its scatters and one pyramid launch over all its areas
    const mosaic_win grid{ p->x0, p->y0, p->cell, p->W, p->H, 0, 0, 0, 0, p->use_mask != 0 };
    for (int i = 0; i < n; ++i) {
        if (!njobs[i]) continue;
        HIPCHK(c, hipMemsetAsync(d_win, 0, acc_cells[i] * 8, c->stream));
        if (on_grid[i]) launch_scatter(c, d_jobs + i, 1, jobs[i].N, wins[i], d_win);
        if (acc_cells[i] > a_cells[i]) launch_scatter_seg(c, d_jobs + i, jobs[i].N, grid, d_win + a_cells[i], d_segs + seg0[i], seg_pings);
        hipLaunchKernelGGL(mosaic_pyr_kernel, dim3((unsigned)pyr_blocks[i]), dim3(256), 0, c->stream, d_pj + job0[i], njobs[i], L, d_win, d_lay, d_flag);
        HIPCHK(c, hipGetLastError());
    }
    // 2. level by level from the top: the rows still alive around their centres, one launch, one download, the level rule on the host
    const uint64_t* tab = c->mosaic_pinned.as<uint64_t>() + 1;                  // the flag is tab[-1] on both paths
    const dsss_reg_result* rec = reinterpret_cast<const dsss_reg_result*>(tab); // device path: the records of the level's live rows, in their order
    std::vector<int> live; live.reserve(nseg);                                  // device path: the rows still alive, whose tables lie one behind the other
    const size_t row_sums = (nshift_of(L - 1) + (size_t)(L - 1) * nshift_of(0)) * 6;
    std::vector<char> alive(nseg, 1); std::vector<int32_t> cx(nseg, 0), cy(nseg, 0);
    std::vector<reg_job> pj; pj.reserve(nseg);
    for (int l = L - 1; l >= 0; --l) {
        const int r = radius_of(l); const size_t tsz = nshift_of(l) * 6;
        pj.clear(); live.clear();
        long long blocks = 0;
        for (int row = 0; row < nseg; ++row) {
            const int ia = row_a[row], g = row_g[row];
            if (!alive[row]) continue;
            const size_t at_tab = dev ? live.size() : (size_t)row;              // host path: every row keeps its place
            live.push_back(row);                                                // (a live row off the grid has no job: its table stays zero)
            if (!on_grid[ia] || sw[g].bw == 0) continue;
            if (!reg_push_job(pj, &blocks, d_lay + a_lay[ia].off[l], pyr_window(wins[ia], l, 0, 0), d_lay + seg_lay[g].off[l], pyr_window(sw[g], l, cx[row], cy[row]),
                              r, d_tab + at_tab * tsz))
                DSSS_FAIL(c, DSSS_E_NUMERIC, "register: internal error, level %d of %d segments takes more workgroups than was bounded", l, nseg);
        }
        const size_t ntab = dev ? live.size() : (size_t)nseg;
        const size_t down = dev ? 8 + ntab * sizeof(dsss_reg_result) : (1 + ntab * tsz) * 8;
        HIPCHK(c, hipMemsetAsync(d_tab, 0, ntab * tsz * 8, c->stream));
        rc = reg_launch_corr(c, pj, blocks, d_pairs, r); if (rc) return rc;
        if (dev) { rc = reg_launch_peaks(c, d_tab, (long long)ntab, r, pyr_min_cells(R.min_cells, l), ldexp(p->cell, l), d_rec); if (rc) return rc; }
        HIPCHK(c, hipMemcpyAsync(c->mosaic_pinned.p, d_flag, down, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        cnt.down(down); cnt.sync();
        if ((int)tab[-1]) DSSS_FAIL(c, DSSS_E_CAPACITY, "mosaic: a cell received more than 2^24 samples of one frame (cell %g too coarse)", p->cell);
        (dev ? cnt.I.tables_device : cnt.I.tables_host) += (int64_t)live.size();
        if (dev) {                                                              // the level rule's centre on the downloaded records
            for (size_t k = 0; k < live.size(); ++k) {
                const int row = live[k];
                dsss_reg_seg_pyr& o = out_host[row];
                dsss_reg_result q = rec[k]; int32_t usable = 0, nx = 0, ny = 0;
                pyr_centre_of(p->cell, l, cx[row], cy[row], &q, &usable, &nx, &ny);
                if (!usable) { alive[row] = 0; if (l == L - 1) o.s.r = q; continue; }
                o.s.r = q; o.level = l; o.lx[l] = q.dx; o.ly[l] = q.dy; o.lz[l] = q.zncc;
                if (q.on_border) o.border_mask |= 1 << l;
                cx[row] = nx; cy[row] = ny;
            }
            continue;
        }
        const size_t at = l == L - 1 ? 0 : (nshift_of(L - 1) + (size_t)(L - 2 - l) * nshift_of(0)) * 6;      // this level's table within a row of sums_host
        for (int row = 0; row < nseg; ++row) {
            if (sums_host) {
                if (alive[row]) memcpy(sums_host + (size_t)row * row_sums + at, tab + (size_t)row * tsz, tsz * 8);
                else memset(sums_host + (size_t)row * row_sums + at, 0, tsz * 8);
            }
            if (!alive[row]) continue;
            dsss_reg_seg_pyr& o = out_host[row];
            dsss_reg_result q; int32_t usable = 0, nx = 0, ny = 0;
            pyr_step_of(tab + (size_t)row * tsz, r, R.min_cells, p->cell, l, cx[row], cy[row], &q, &usable, &nx, &ny);
            if (!usable) { alive[row] = 0; if (l == L - 1) o.s.r = q; continue; }              // no level has a usable peak: the top level's record
            o.s.r = q; o.level = l; o.lx[l] = q.dx; o.ly[l] = q.dy; o.lz[l] = q.zncc;
            if (q.on_border) o.border_mask |= 1 << l;
            cx[row] = nx; cy[row] = ny;
        }
    }
    // 3. the centroid sums at the total shift of the rows that finished at level 0: one launch, one download
    std::vector<cen_job> cj;
    long long cblocks = 0;
    for (int row = 0; row < nseg; ++row) {
        dsss_reg_seg_pyr& o = out_host[row];
        if (o.level < 0) continue;                                              // the no-usable-shift record stays as it is
        if (o.level == 0 && !cen_push_job(cj, &cblocks, d_lay + a_lay[row_a[row]].off[0], wins[row_a[row]], d_lay + seg_lay[row_g[row]].off[0], sw[row_g[row]], o.s.r,
                                          d_cen + (size_t)row * 3))
            DSSS_FAIL(c, DSSS_E_NUMERIC, "register: internal error, the centroid of %d segments takes more workgroups than was bounded", nseg);
        o.s.r.on_border = (o.border_mask != 0 || o.level != 0) ? 1 : 0;
    }
    if (!cj.empty()) {
        std::vector<uint64_t> cen((size_t)nseg * 3);
        rc = reg_launch_centroids(c, cj, cblocks, d_cj, d_cen, cen, cnt); if (rc) return rc;
        for (int row = 0; row < nseg; ++row) {
            dsss_reg_seg& o = out_host[row].s;
            if (out_host[row].level != 0) continue;
            if ((int64_t)cen[(size_t)row * 3] != o.r.n)
                DSSS_FAIL(c, DSSS_E_NUMERIC, "register: internal error, row %d has %lld cells at its peak and %lld in its centroid", row,
                          (long long)o.r.n, (long long)cen[(size_t)row * 3]);
            o.sx = (int64_t)cen[(size_t)row * 3 + 1]; o.sy = (int64_t)cen[(size_t)row * 3 + 2];
        }
    }
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
    const size_t tsz = (size_t)(2 * radius + 1) * (2 * radius + 1) * 6, nt = (size_t)ntables;
    hipPointerAttribute_t at;
    const bool on_dev = (hipPointerGetAttributes(&at, sums) == hipSuccess) && at.type == hipMemoryTypeDevice;
    (void)hipGetLastError();
    carve L;
    const size_t o_rec = L.take(nt * sizeof(dsss_reg_result)), o_tab = L.take(on_dev ? 0 : nt * tsz * 8);      // host tables go up into mosaic_buf
    int rc = c->mosaic_buf.reserve(c, L.off); if (rc) return rc;
    rc = c->mosaic_pinned.reserve(c, nt * sizeof(dsss_reg_result)); if (rc) return rc;
    char* B = c->mosaic_buf.as<char>();
    dsss_reg_result* d_rec = reinterpret_cast<dsss_reg_result*>(B + o_rec);
    const unsigned long long* d_tab = reinterpret_cast<const unsigned long long*>(sums);
    if (!on_dev) {
        HIPCHK(c, hipMemcpyAsync(B + o_tab, sums, nt * tsz * 8, hipMemcpyHostToDevice, c->stream));
        d_tab = reinterpret_cast<const unsigned long long*>(B + o_tab);
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

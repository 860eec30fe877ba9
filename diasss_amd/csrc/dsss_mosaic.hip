// diasss_amd/csrc/dsss_mosaic.hip -- georeferenced mosaic and overlap-consistency map (include/dsss.h, section "mosaic").
// The reference has no counterpart: it stops at the trajectory file.  What goes into the mosaic is on the device when the solve
// returns (normalised waterfall, filter mask, geometry), so the map is a forward scatter of the pixels into a grid of integer
// accumulators.  Integers because the result has to be the same whatever the order of the frames and from call to call.
#include "dsss_mosaic_int.h"
#include <algorithm>

namespace {

// One workgroup per ping, one wavefront per 64 consecutive bins.  The bearing of each side is evaluated once per ping (dsss_geo_side)
// and shared through LDS; the bins then cost a multiply-add and two divisions each.  Consecutive bins of a ping walk through the
// grid, so lanes that hit the cell of their neighbour form runs: (sum, count) is reduced within a run with a segmented scan over
// the wavefront (mosaic_run_reduce) and the last lane of the run issues ONE 64-bit atomic without return, count in the high word and sum in the low
// one.  A wavefront adds at most 64 x 255 to a sum, and below 2^24 samples per cell (checked by mosaic_unpack_kernel) the low word
// cannot carry into the high one.  (One atomic per pixel took 13.3 ms where this takes 6.7: DESIGN.md section 4, "Mosaic".)
//
// SEG: the segmented form of the registration's segment layers.  The ping's segment (row / seg_pings) selects the window (ox, oy, bw, bh
// of G are replaced by the segment's) and the accumulator area (acc + the segment's offset), so one launch renders every segment of a
// frame; everything else, the arithmetic of a sample included (mosaic_scatter_samples, dsss_mosaic_int.h: the registration's yaw fan
// runs it too), is the one body.
template <bool SEG>
__device__ __forceinline__ void mosaic_scatter_body(const mosaic_job* __restrict__ jobs, int njobs, mosaic_win G, unsigned long long* __restrict__ acc,
                                                    const mosaic_seg* __restrict__ segs, int seg_pings)
{
    __shared__ double s_sc[4];
    mosaic_job J; int row; const double* P;
    if (!mosaic_ping_of(jobs, njobs, s_sc, J, row, P)) return;
    if (SEG) {
        const mosaic_seg sg = segs[row / seg_pings];
        if (sg.bw <= 0) return;                                                    // a segment with no cell on the grid (uniform per workgroup)
        G.ox = sg.ox; G.oy = sg.oy; G.bw = sg.bw; G.bh = sg.bh; acc += sg.off;
    }
    mosaic_scatter_samples(P, s_sc, J, row, G, acc);
}

__global__ __launch_bounds__(256) void mosaic_scatter_kernel(const mosaic_job* __restrict__ jobs, int njobs, mosaic_win G,
                                                             unsigned long long* __restrict__ acc)
{
    mosaic_scatter_body<false>(jobs, njobs, G, acc, nullptr, 1);
}

__global__ __launch_bounds__(256) void mosaic_scatter_seg_kernel(const mosaic_job* __restrict__ jobs, int njobs, mosaic_win G,
                                                                 unsigned long long* __restrict__ acc, const mosaic_seg* __restrict__ segs, int seg_pings)
{
    mosaic_scatter_body<true>(jobs, njobs, G, acc, segs, seg_pings);
}

// The footprint form of mosaic_scatter_kernel ("footprint rendering" in the header), in its launch shape: the ping's prologue in the
// partner form (sin and cos of both sides of the next ping beside the ping's own in LDS), then the sub-samples of the ping's samples
// by the one body (mosaic_scatter_footprints, dsss_mosaic_int.h).  A kernel of its own: dsss_mosaic_render keeps the one above.
__global__ __launch_bounds__(256) void mosaic_scatter_fp_kernel(const mosaic_job* __restrict__ jobs, int njobs, mosaic_win G, dsss_footprint_params F,
                                                                unsigned long long* __restrict__ acc)
{
    __shared__ double s_sc[8];
    mosaic_job J; int row; const double* P; const double* PP; bool last;
    if (!mosaic_ping_of(jobs, njobs, s_sc, J, row, P, &PP, &last)) return;
    mosaic_scatter_footprints(P, PP, last, s_sc, J, row, G, F, acc);
}

// accumulators -> the host layers' layout; flags a cell over the sample limit (also run with no outputs, as the check alone)
__global__ __launch_bounds__(256) void mosaic_unpack_kernel(const unsigned long long* __restrict__ acc, size_t n, uint32_t* __restrict__ sum,
                                                            uint32_t* __restrict__ cnt, uint8_t* __restrict__ img, int* __restrict__ flag)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const mosaic_acc a(acc[i]);
    if (a.over_limit()) *flag = 1;
    if (sum) sum[i] = a.s;
    if (cnt) cnt[i] = a.c;
    if (img) img[i] = a.c ? (uint8_t)a.mean() : (uint8_t)0;
}

// one frame's window folded into the three layers of the consistency map: one frame at a time, so plain stores
__global__ __launch_bounds__(256) void mosaic_fold_kernel(const unsigned long long* __restrict__ win, mosaic_win G, uint32_t* __restrict__ nfr,
                                                          uint32_t* __restrict__ s1, uint32_t* __restrict__ s2, int* __restrict__ flag)
{
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= (size_t)G.bw * G.bh) return;
    const mosaic_acc a(win[j]);
    if (a.c == 0) return;
    if (a.over_limit()) *flag = 1;
    const uint32_t m = a.mean();
    const int jy = (int)(j / G.bw), jx = (int)(j - (size_t)jy * G.bw);
    const size_t g = (size_t)(G.oy + jy) * G.W + (G.ox + jx);
    nfr[g] += 1; s1[g] += m; s2[g] += m * m;
}

// ---- range-gain statistics ("range-gain normalisation" and "altitude-banded range gain" in the header)
#define COLSTAT_COLS 4                     // consecutive columns a lane owns: one dword of a row
#define COLSTAT_LANES 64                   // lanes across a row at most: a wavefront reads 256 consecutive bytes of it (why: mosaic_gainstat_kernel's comment)
#define COLSTAT_ROWS 128                   // rows a lane walks: 128 x 255 < 2^16, far inside the u32 partials
#define COLSTAT_BATCH 8                    // rows a lane has in flight (two dwords each)
#define BAND_MAX 16                        // bands of a table

// a frame's workgroups: chunks of tpr x 4 columns x blocks of (256 / tpr) x COLSTAT_ROWS rows, tpr = the power of two of lanes that
// cover a row's groups of four columns, COLSTAT_LANES at most
__host__ __device__ inline int colstat_tpr(int M)
{
    const int groups = (M + COLSTAT_COLS - 1) / COLSTAT_COLS;
    int tpr = 1;
    while (tpr < groups && tpr < COLSTAT_LANES) tpr <<= 1;
    return tpr;
}
__host__ __device__ inline int colstat_chunks(int M) { const int tpr = colstat_tpr(M); return ((M + COLSTAT_COLS - 1) / COLSTAT_COLS + tpr - 1) / tpr; }

// one dword of image and one of mask into the partials of the lane's four columns
template <bool MASK> __device__ __forceinline__ void colstat_add(uint32_t v, uint32_t m, uint32_t (&s)[COLSTAT_COLS], uint32_t (&n)[COLSTAT_COLS])
{
#pragma unroll
    for (int k = 0; k < COLSTAT_COLS; ++k) {
        const bool keep = !MASK || ((m >> (8 * k)) & 0xffu) != 0;
        s[k] += keep ? (v >> (8 * k)) & 0xffu : 0u; n[k] += keep ? 1u : 0u;
    }
}

// the rows row0, row0 + rl, ... below row1 of the lane's dword column.  nmin (uniform per workgroup) = the rows every lane of the
// workgroup has, COLSTAT_ROWS but in a frame's last block: they go in batches whose trip count no lane disagrees about, so
// COLSTAT_BATCH rows are loaded before the first is used; what is left, at most COLSTAT_BATCH rows a lane, goes one by one.
template <bool MASK> __device__ __forceinline__ void colstat_words(const uint32_t* __restrict__ img, const uint32_t* __restrict__ msk, size_t M4, int row0, int row1, int rl,
                                                                   int nmin, uint32_t (&s)[COLSTAT_COLS], uint32_t (&n)[COLSTAT_COLS])
{
    const uint32_t* __restrict__ pi = img + (size_t)row0 * M4; const uint32_t* __restrict__ pm = msk + (size_t)row0 * M4;
    const size_t step = (size_t)rl * M4;
    const int nb = nmin - nmin % COLSTAT_BATCH;
    for (int i = 0; i < nb; i += COLSTAT_BATCH) {
        uint32_t v[COLSTAT_BATCH], m[COLSTAT_BATCH];
#pragma unroll
        for (int j = 0; j < COLSTAT_BATCH; ++j) { v[j] = pi[(size_t)(i + j) * step]; m[j] = MASK ? pm[(size_t)(i + j) * step] : 0u; }
#pragma unroll
        for (int j = 0; j < COLSTAT_BATCH; ++j) colstat_add<MASK>(v[j], m[j], s, n);
    }
    for (int row = row0 + nb * rl; row < row1; row += rl) colstat_add<MASK>(img[(size_t)row * M4], MASK ? msk[(size_t)row * M4] : 0u, s, n);
}

// a slot of the workgroup's table in LDS (mosaic_gainstat_kernel): tab[band][sum | count][k][lane across the row], u32 -- a workgroup
// sees rl x COLSTAT_ROWS <= 2^15 rows of a column, 2^15 x 255 < 2^32
__device__ __forceinline__ int bandstat_slot(int tpr, int band, int what, int k, int lt) { return ((band * 2 + what) * COLSTAT_COLS + k) * tpr + lt; }

// the lane's partials, which are those of `band`, into the workgroup's table (LDS atomics without return), and back to zero
__device__ __forceinline__ void bandstat_flush(uint32_t* __restrict__ tab, int tpr, int band, int lt, uint32_t (&s)[COLSTAT_COLS], uint32_t (&n)[COLSTAT_COLS])
{
#pragma unroll
    for (int k = 0; k < COLSTAT_COLS; ++k) {
        if (n[k]) { atomicAdd(&tab[bandstat_slot(tpr, band, 0, k, lt)], s[k]); atomicAdd(&tab[bandstat_slot(tpr, band, 1, k, lt)], n[k]); }
        s[k] = 0; n[k] = 0;
    }
}

// colstat_words where the rows of the workgroup lie in more than one band: band[i * rl] = the band of the lane's row i.  A batch whose
// rows all lie in the band the partials belong to (cur) goes as colstat_words' batch does; otherwise its rows go one by one, the
// partials leaving for the table wherever the band changes.
template <bool MASK> __device__ __forceinline__ void bandstat_words(const uint32_t* __restrict__ img, const uint32_t* __restrict__ msk, size_t M4, int row0, int row1, int rl,
                                                                    int nmin, const uint8_t* __restrict__ band, uint32_t* __restrict__ tab, int tpr, int lt, int& cur,
                                                                    uint32_t (&s)[COLSTAT_COLS], uint32_t (&n)[COLSTAT_COLS])
{
    const uint32_t* __restrict__ pi = img + (size_t)row0 * M4; const uint32_t* __restrict__ pm = msk + (size_t)row0 * M4;
    const size_t step = (size_t)rl * M4;
    const int nb = nmin - nmin % COLSTAT_BATCH;
    for (int i = 0; i < nb; i += COLSTAT_BATCH) {
        uint32_t v[COLSTAT_BATCH], m[COLSTAT_BATCH]; int b[COLSTAT_BATCH];
        bool same = true;
#pragma unroll
        for (int j = 0; j < COLSTAT_BATCH; ++j) {
            v[j] = pi[(size_t)(i + j) * step]; m[j] = MASK ? pm[(size_t)(i + j) * step] : 0u;
            b[j] = band[(i + j) * rl]; same = same && b[j] == cur;
        }
        if (same) {
#pragma unroll
            for (int j = 0; j < COLSTAT_BATCH; ++j) colstat_add<MASK>(v[j], m[j], s, n);
        } else {
#pragma unroll
            for (int j = 0; j < COLSTAT_BATCH; ++j) {
                if (b[j] != cur) { bandstat_flush(tab, tpr, cur, lt, s, n); cur = b[j]; }
                colstat_add<MASK>(v[j], m[j], s, n);
            }
        }
    }
    for (int i = nb, row = row0 + nb * rl; row < row1; row += rl, ++i) {
        const int b = band[i * rl];
        if (b != cur) { bandstat_flush(tab, tpr, cur, lt, s, n); cur = b; }
        colstat_add<MASK>(img[(size_t)row * M4], MASK ? msk[(size_t)row * M4] : 0u, s, n);
    }
}

// S[b][c] = sum of the kept samples of column c over the pings of band b, C[b][c] = their number, over all frames of the job table:
// out[b M + c] += S, out[(nbands + b) M + c] += C.  One band (the column statistics; gain_one_band()): out[c], out[M + c].  A streaming
// integer reduction, two bytes read per sample and nothing else.
// Lanes: a lane owns four consecutive columns; tpr lanes (a wavefront at most: the whole workgroup across a row took four times the
// atomics and 0.36 ms where this takes 0.22, DESIGN.md section 4, "Range-gain normalisation") lie across a row, so a wavefront reads
// consecutive dwords of it, and the 256 / tpr lanes that share a column group take rows `rl` apart -- four wavefronts four rows, and a
// narrow frame still fills the workgroup.  A lane walks COLSTAT_ROWS rows with the eight u32 partials of its columns in registers.
// Loads: rows are dword-aligned where M % 4 == 0 and the images are, and go COLSTAT_BATCH in flight (colstat_words, bandstat_words);
// otherwise (uniform per launch: all frames have one M) a lane reads its four bytes one by one, and the columns behind M are skipped.
// Bands: sixteen bands of eight partials do not fit a lane's registers, so a lane keeps the partials of ONE band, that of its last row.
// With more than one band the workgroup first writes the band of each of its rows into LDS (one f64 division a row, not one a lane and
// row) and learns with the same barrier whether they all lie in one band.  If so -- the rule on real data, where the altitude moves
// through a band over hundreds of pings, and always with one band, where J.alt is not read -- the lanes run colstat_words.  Otherwise
// a lane's partials leave for the table when its next row lies in another band: a band that changes on every ping costs eight LDS
// atomics a row and lane, and nothing global.
// Table: tab[band][sum | count][k][lane] in LDS, u32, is the one reduction across the lanes that share a column (ds_add without
// return); dynamic LDS is nbands x 8 x tpr words and, behind them, rows_wg bytes for the bands of the rows, 33 KB at most.
// Exit: the table leaves through 64-bit atomics without return, only for the entries that kept a sample.  Integers throughout, so the
// result depends on no order.
__global__ __launch_bounds__(256) void mosaic_gainstat_kernel(const mosaic_job* __restrict__ jobs, int njobs, int use_mask, unsigned long long* __restrict__ out)
{
    extern __shared__ uint32_t s_band_dyn[];
    const mosaic_job J = mosaic_job_of(jobs, njobs);
    const int M = J.M, tpr = colstat_tpr(M), rl = 256 / tpr, chunks = colstat_chunks(M), rows_wg = rl * COLSTAT_ROWS, nbands = J.bands.nbands;
    const int wg = (int)blockIdx.x - J.blk0;
    const int rb = wg / chunks, ch = wg - rb * chunks;
    const int lt = (int)threadIdx.x & (tpr - 1), col = (ch * tpr + lt) * COLSTAT_COLS;
    const int rbase = rb * rows_wg, row0 = rbase + (int)threadIdx.x / tpr, row1 = min(J.N, rbase + rows_wg);
    const int nmin = (row1 - rbase) / rl;                                          // rows every lane of the workgroup has
    uint32_t* __restrict__ tab = s_band_dyn;
    const int ntab = nbands * 2 * COLSTAT_COLS * tpr;
    uint8_t* __restrict__ s_band = reinterpret_cast<uint8_t*>(s_band_dyn + ntab);
    for (int e = (int)threadIdx.x; e < ntab; e += 256) tab[e] = 0;
    int cur = 0, differs = 0;
    if (nbands > 1) {                                                              // (uniform per launch; rbase < J.N with the host's blocks)
        cur = gain_band(J.bands, J.alt[rbase]);
        for (int r = rbase + (int)threadIdx.x; r < row1; r += 256) { const int b = gain_band(J.bands, J.alt[r]); s_band[r - rbase] = (uint8_t)b; differs |= b != cur; }
    }
    const bool mixed = __syncthreads_or(differs) != 0;                             // (uniform per workgroup)
    uint32_t s[COLSTAT_COLS] = { 0, 0, 0, 0 }, n[COLSTAT_COLS] = { 0, 0, 0, 0 };
    if (col < M) {
        if (M % 4 == 0 && (((uintptr_t)J.img | (uintptr_t)J.mask) & 3) == 0) {
            const uint32_t* img = reinterpret_cast<const uint32_t*>(J.img + col); const uint32_t* msk = reinterpret_cast<const uint32_t*>(J.mask + col);
            const size_t M4 = (size_t)(M / 4);
            if (!mixed) { if (use_mask) colstat_words<true>(img, msk, M4, row0, row1, rl, nmin, s, n); else colstat_words<false>(img, msk, M4, row0, row1, rl, nmin, s, n); }
            else if (use_mask) bandstat_words<true>(img, msk, M4, row0, row1, rl, nmin, s_band + (row0 - rbase), tab, tpr, lt, cur, s, n);
            else bandstat_words<false>(img, msk, M4, row0, row1, rl, nmin, s_band + (row0 - rbase), tab, tpr, lt, cur, s, n);
        } else {
            const int nc = min(COLSTAT_COLS, M - col);
            for (int row = row0; row < row1; row += rl) {
                const uint8_t* __restrict__ img = J.img + (size_t)row * M + col;
                const uint8_t* __restrict__ msk = J.mask + (size_t)row * M + col;
                if (mixed) { const int b = s_band[row - rbase]; if (b != cur) { bandstat_flush(tab, tpr, cur, lt, s, n); cur = b; } }
#pragma unroll
                for (int k = 0; k < COLSTAT_COLS; ++k) {
                    if (k >= nc) continue;
                    const bool keep = !use_mask || msk[k] != 0;
                    s[k] += keep ? (uint32_t)img[k] : 0u; n[k] += keep ? 1u : 0u;
                }
            }
        }
        bandstat_flush(tab, tpr, cur, lt, s, n);
    }
    __syncthreads();
    const int ncl = COLSTAT_COLS * tpr;                                            // the columns of the chunk, consecutive lanes consecutive columns
    for (int e = (int)threadIdx.x; e < nbands * ncl; e += 256) {
        const int b = e / ncl, cl = e - b * ncl, c = ch * ncl + cl;
        const uint32_t cnt = tab[bandstat_slot(tpr, b, 1, cl & 3, cl >> 2)];
        if (c >= M || cnt == 0) continue;
        atomicAdd(&out[(size_t)b * M + c], (unsigned long long)tab[bandstat_slot(tpr, b, 0, cl & 3, cl >> 2)]);
        atomicAdd(&out[(size_t)(nbands + b) * M + c], (unsigned long long)cnt);
    }
}

// The corrected waterfall of one frame: a streaming pass, one workgroup per ping, the band once per ping and the gain per column through
// mosaic_gain_apply -- the sample every entry that bins bins.  J.gain == null: the normalised image itself.
__global__ __launch_bounds__(256) void mosaic_correct_kernel(mosaic_job J, uint8_t* __restrict__ out)
{
    const int row = (int)blockIdx.x, M = J.M;
    if (row >= J.N) return;
    const uint16_t* __restrict__ gain = mosaic_gain_row(J, row);
    const uint8_t* __restrict__ img = J.img + (size_t)row * M;
    uint8_t* __restrict__ o = out + (size_t)row * M;
    for (int col = (int)threadIdx.x; col < M; col += 256) o[col] = (uint8_t)mosaic_gain_apply(img[col], gain, col);
}

} // namespace

// ---- host helpers shared with dsss_mosaic_reg.hip (dsss_mosaic_int.h)
int mosaic_check_frames(dsss_ctx* c, const int* ids, int n, const double* rpy6, const int* ping_off, bool need_img, size_t* rows)
{
    if (!ids || n < 1) DSSS_FAIL(c, DSSS_E_ARG, "mosaic: no frame ids");
    if (rpy6 && !ping_off) DSSS_FAIL(c, DSSS_E_ARG, "mosaic: a trajectory needs ping_off");
    std::vector<char> seen(c->max_frames, 0);
    size_t total = 0;
    for (int i = 0; i < n; ++i) {
        const int id = ids[i];
        if (id < 0 || id >= c->max_frames) DSSS_FAIL(c, DSSS_E_ARG, "frame id %d out of range [0,%d)", id, c->max_frames);
        if (seen[id]) DSSS_FAIL(c, DSSS_E_ARG, "mosaic: frame %d listed twice", id);
        seen[id] = 1;
        if (rpy6 && ping_off[i] < 0) DSSS_FAIL(c, DSSS_E_ARG, "mosaic: ping_off[%d] = %d", i, ping_off[i]);
        const dsss_frame& f = c->frames[id];
        if (!f.has_geom || !f.h_geo) DSSS_FAIL(c, DSSS_E_STATE, "frame %d has no geometry", id);
        if (need_img && (!f.has_norm || !f.lvl[0] || !f.mask)) DSSS_FAIL(c, DSSS_E_STATE, "frame %d not extracted yet", id);
        total += (size_t)f.N;
    }
    if (total > 0x7fffffffull) DSSS_FAIL(c, DSSS_E_ARG, "mosaic: %zu pings in one call", total);
    *rows = total;
    return DSSS_OK;
}

int mosaic_check_params(dsss_ctx* c, const dsss_mosaic_params* p)
{
    if (!p) DSSS_FAIL(c, DSSS_E_ARG, "mosaic: no grid");
    if (!(p->cell > 0.0) || !std::isfinite(p->cell)) DSSS_FAIL(c, DSSS_E_ARG, "mosaic: cell = %g", p->cell);
    if (p->W < 1 || p->H < 1 || (long long)p->W * p->H > MOSAIC_MAX_CELLS) DSSS_FAIL(c, DSSS_E_ARG, "mosaic: grid %d x %d", p->W, p->H);
    return DSSS_OK;
}

int mosaic_check_args(dsss_ctx* c, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params* p, size_t* rows)
{
    int rc = mosaic_check_frames(c, ids, n, rpy6, ping_off, true, rows); if (rc) return rc;
    rc = mosaic_check_params(c, p); if (rc) return rc;
    return mosaic_check_gain(c, ids, n);
}

bool footprint_params_ok(const dsss_footprint_params& F)
{
    return F.max_steps >= 1 && F.max_steps <= FP_MAX_STEPS && std::isfinite(F.max_gap) && F.max_gap > 0.0;
}

int mosaic_check_footprint(dsss_ctx* c, const int* ids, int n, const dsss_footprint_params* fp, dsss_footprint_params* out)
{
    dsss_footprint_params_default(out);
    if (fp) *out = *fp;
    out->pad_ = 0;
    if (!footprint_params_ok(*out)) DSSS_FAIL(c, DSSS_E_ARG, "footprint: max_steps %d, max_gap %g (1..%d; finite and > 0)", out->max_steps, out->max_gap, FP_MAX_STEPS);
    for (int i = 0; i < n; ++i) {
        const int M = c->frames[ids[i]].M;
        if (M < 4 || (M & 1)) DSSS_FAIL(c, DSSS_E_ARG, "footprint: frame %d has %d columns (even, at least 4)", ids[i], M);
    }
    return DSSS_OK;
}

// geo extremes of one frame under the given pose rows: x = px + g c is monotone in g for a fixed bearing, so only the smallest and the
// largest ground range of a side can be extreme (what geo_bbox_kernel evaluates).  On the host: two bearings per ping, off the hot
// path, and the same arithmetic bit for bit.  Non-finite points compare false and are left out.
void frame_extent(const dsss_frame& f, const double* rows, double* bb) { frame_extent_rows(f, rows, 0, f.N, bb); }

// the same over the pings [r0, r1) of the frame (the registration's segments)
void frame_extent_rows(const dsss_frame& f, const double* rows, int r0, int r1, double* bb)
{
    const double* gr = f.h_geo + (size_t)f.N * 7;
    const int M = f.M, half = M / 2;
    int col_min[2], col_max[2];      // columns of the smallest / largest ground range per side
    const double origin[6] = { 0, 0, 0, 0, 0, 0 };
    for (int side = 0; side < 2; ++side) {
        const int c_lo = side ? half : 0, c_hi = side ? M : half;
        int cmin = c_lo, cmax = c_lo; double gmin = INFINITY, gmax = -INFINITY;
        for (int col = c_lo; col < c_hi; ++col) {
            double g, unused; dsss_geo_bin(origin, gr, M, col, 0.0, 1.0, &g, &unused);      // the bin's ground range: pose 0, bearing 0
            if (g < gmin) { gmin = g; cmin = col; }
            if (g > gmax) { gmax = g; cmax = col; }
        }
        col_min[side] = cmin; col_max[side] = cmax;
    }
    for (int row = r0; row < r1; ++row) {
        const double* P = rows + (size_t)row * 6;
        for (int side = 0; side < 2; ++side) {
            double s, co; dsss_geo_side(P, side == 1, &s, &co);
            for (int e = 0; e < 2; ++e) {
                double x, y; dsss_geo_bin(P, gr, M, e ? col_max[side] : col_min[side], s, co, &x, &y);
                bb[0] = x < bb[0] ? x : bb[0]; bb[1] = x > bb[1] ? x : bb[1];
                bb[2] = y < bb[2] ? y : bb[2]; bb[3] = y > bb[3] ? y : bb[3];
            }
        }
    }
}

// cells [a, b] of one axis that the points lo .. hi can fall into; false when none of them lies on the grid
bool cell_range(double lo, double hi, double origin, double cell, int n, int* a, int* b)
{
    const double fl = floor((lo - origin) / cell), fh = floor((hi - origin) / cell);
    if (!(fh >= 0.0) || !(fl < (double)n)) return false;
    *a = fl < 0.0 ? 0 : (int)fl; *b = fh >= (double)n ? n - 1 : (int)fh;
    return true;
}

mosaic_win mosaic_grid_win(const dsss_mosaic_params* p) { return mosaic_win{ p->x0, p->y0, p->cell, p->W, p->H, 0, 0, p->W, p->H, p->use_mask != 0 }; }

// (grow = 0 leaves the point windows their bits: x - 0.0 is x for every double, and x + 0.0 differs from x in the sign of a zero alone,
// which cell_range's differences, comparisons and conversion do not see)
bool mosaic_window(const dsss_frame& f, const double* rows, int r0, int r1, const dsss_mosaic_params* p, mosaic_win* w, double grow)
{
    double bb[4] = { INFINITY, -INFINITY, INFINITY, -INFINITY };
    frame_extent_rows(f, rows, r0, r1, bb);
    int ax, bx, ay, by;
    if (!cell_range(bb[0] - grow, bb[1] + grow, p->x0, p->cell, p->W, &ax, &bx) ||
        !cell_range(bb[2] - grow, bb[3] + grow, p->y0, p->cell, p->H, &ay, &by)) return false;
    *w = mosaic_grid_win(p);
    w->ox = ax; w->oy = ay; w->bw = bx - ax + 1; w->bh = by - ay + 1;
    return true;
}

int mosaic_flag_down(dsss_ctx* c, const int* d_flag, const char* fmt, double cell)
{
    int flag = 0;
    HIPCHK(c, hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (flag) DSSS_FAIL(c, DSSS_E_CAPACITY, fmt, cell);
    return DSSS_OK;
}

// the caller's trajectory rows of the listed frames go up packed in the order of ids (neighbouring frames that are neighbours in
// rpy6 too share a copy); dev_rows[i] = where frame i reads its rows
int upload_rows(dsss_ctx* c, const int* ids, int n, const double* rpy6, const int* ping_off, double* d_rows, std::vector<const double*>& dev_rows)
{
    dev_rows.resize(n);
    if (!rpy6) { for (int i = 0; i < n; ++i) dev_rows[i] = c->frames[ids[i]].pose6; return DSSS_OK; }
    size_t off = 0;
    for (int i = 0; i < n;) {
        int j = i; size_t len = 0;
        do { dev_rows[j] = d_rows + (off + len) * 6; len += (size_t)c->frames[ids[j]].N; ++j; }
        while (j < n && (size_t)ping_off[j] == (size_t)ping_off[j - 1] + (size_t)c->frames[ids[j - 1]].N);
        HIPCHK(c, hipMemcpyAsync(d_rows + off * 6, rpy6 + (size_t)ping_off[i] * 6, len * 6 * sizeof(double), hipMemcpyHostToDevice, c->stream));
        off += len; i = j;
    }
    return DSSS_OK;
}

int mosaic_check_gain(dsss_ctx* c, const int* ids, int n)
{
    if (!c->mosaic_gain_M) return DSSS_OK;
    for (int i = 0; i < n; ++i)
        if (c->frames[ids[i]].M != c->mosaic_gain_M)
            DSSS_FAIL(c, DSSS_E_ARG, "mosaic: the range-gain table has %d columns, frame %d has %d", c->mosaic_gain_M, ids[i], c->frames[ids[i]].M);
    return DSSS_OK;
}

int mosaic_fill_jobs(dsss_ctx* c, const int* ids, int n, const double* rpy6, const int* ping_off, double* d_rows, std::vector<mosaic_job>& jobs)
{
    int rc = mosaic_check_gain(c, ids, n); if (rc) return rc;
    std::vector<const double*> dev_rows;
    rc = upload_rows(c, ids, n, rpy6, ping_off, d_rows, dev_rows); if (rc) return rc;
    const uint16_t* gain = c->mosaic_gain_M ? c->mosaic_gain.as<uint16_t>() : nullptr;
    jobs.resize(n);
    for (int i = 0; i < n; ++i) { const dsss_frame& f = c->frames[ids[i]]; jobs[i] = mosaic_job{ dev_rows[i], f.gr, f.lvl[0], f.mask, gain, f.N, f.M, 0, 0, f.alt, gain ? c->mosaic_bands : gain_one_band() }; }
    return DSSS_OK;
}

void launch_scatter(dsss_ctx* c, const mosaic_job* d_jobs, int njobs, int blocks, const mosaic_win& G, unsigned long long* acc)
{
    hipLaunchKernelGGL(mosaic_scatter_kernel, dim3((unsigned)blocks), dim3(256), 0, c->stream, d_jobs, njobs, G, acc);
}

void launch_scatter_seg(dsss_ctx* c, const mosaic_job* d_job, int blocks, const mosaic_win& G, unsigned long long* acc, const mosaic_seg* d_segs, int seg_pings)
{
    hipLaunchKernelGGL(mosaic_scatter_seg_kernel, dim3((unsigned)blocks), dim3(256), 0, c->stream, d_job, 1, G, acc, d_segs, seg_pings);
}

// The accumulators of a render, for the render entries and the profile (dsss_mosaic_profile.hip): acc and the flag cleared, the frames
// scattered (fp == null: as points, otherwise the sub-samples of their footprints), then the unpack into the layers given (null: the
// sample-limit check alone).  jobs = the host's table (mosaic_fill_jobs), whose blk0 are set here; d_jobs = room for it on the device.
int mosaic_render_acc(dsss_ctx* c, std::vector<mosaic_job>& jobs, mosaic_job* d_jobs, const dsss_mosaic_params* p,
                      const dsss_footprint_params* fp, unsigned long long* acc, int* d_flag, uint32_t* d_sum, uint32_t* d_cnt, uint8_t* d_img)
{
    const size_t cells = (size_t)p->W * p->H;
    HIPCHK(c, hipMemsetAsync(acc, 0, cells * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(d_flag, 0, sizeof(int), c->stream));
    const mosaic_win G = mosaic_grid_win(p);
    const unsigned ublocks = (unsigned)((cells + 255) / 256);
    // the sample limit is checked between the launches (mosaic_cut_launches' comment)
    for (const mosaic_launch& L : mosaic_cut_launches(jobs, fp)) {
        if (L.j0 > 0) { hipLaunchKernelGGL(mosaic_unpack_kernel, dim3(ublocks), dim3(256), 0, c->stream, acc, cells, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint8_t*)nullptr, d_flag); HIPCHK(c, hipGetLastError()); }
        HIPCHK(c, hipMemcpyAsync(d_jobs + L.j0, jobs.data() + L.j0, (size_t)(L.j1 - L.j0) * sizeof(mosaic_job), hipMemcpyHostToDevice, c->stream));
        if (!fp) launch_scatter(c, d_jobs + L.j0, L.j1 - L.j0, L.blocks, G, acc);
        else hipLaunchKernelGGL(mosaic_scatter_fp_kernel, dim3((unsigned)L.blocks), dim3(256), 0, c->stream, d_jobs + L.j0, L.j1 - L.j0, G, *fp, acc);
        HIPCHK(c, hipGetLastError());
    }
    hipLaunchKernelGGL(mosaic_unpack_kernel, dim3(ublocks), dim3(256), 0, c->stream, acc, cells, d_sum, d_cnt, d_img, d_flag);
    HIPCHK(c, hipGetLastError());
    return DSSS_OK;
}

extern "C" {

int dsss_mosaic_grid(const double* bbox4, double cell, dsss_mosaic_params* out)
{
    if (!bbox4 || !out) return DSSS_E_ARG;
    if (!(cell > 0.0) || !std::isfinite(cell)) return DSSS_E_ARG;
    for (int k = 0; k < 4; ++k) if (!std::isfinite(bbox4[k])) return DSSS_E_ARG;
    if (bbox4[1] < bbox4[0] || bbox4[3] < bbox4[2]) return DSSS_E_ARG;
    const double x0 = floor(bbox4[0] / cell) * cell, y0 = floor(bbox4[2] / cell) * cell;
    const double w = floor((bbox4[1] - x0) / cell) + 1.0, h = floor((bbox4[3] - y0) / cell) + 1.0;
    if (!(w >= 1.0) || !(h >= 1.0) || !(w * h <= (double)MOSAIC_MAX_CELLS)) return DSSS_E_ARG;
    out->x0 = x0; out->y0 = y0; out->cell = cell; out->W = (int32_t)w; out->H = (int32_t)h; out->use_mask = 1; out->pad_ = 0;
    return DSSS_OK;
}

int dsss_mosaic_bounds(dsss_ctx* c, const int* ids, int n, const double* rpy6, const int* ping_off, double* bbox4)
{
    if (!c || !bbox4) return DSSS_E_ARG;
    size_t rows = 0;
    int rc = mosaic_check_frames(c, ids, n, rpy6, ping_off, false, &rows); if (rc) return rc;
    double bb[4] = { INFINITY, -INFINITY, INFINITY, -INFINITY };
    for (int i = 0; i < n; ++i) {
        const dsss_frame& f = c->frames[ids[i]];
        frame_extent(f, rpy6 ? rpy6 + (size_t)ping_off[i] * 6 : f.h_geo, bb);
    }
    memcpy(bbox4, bb, sizeof bb);
    return DSSS_OK;
}

// The render behind the argument checks, for both entries: fp == null bins the samples as points (mosaic_scatter_kernel), otherwise the
// sub-samples of their footprints (mosaic_scatter_fp_kernel); jobs, arena, sample-limit check and download are the same.
static int render_run(dsss_ctx* c, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params* p, size_t rows,
                      const dsss_footprint_params* fp, uint32_t* sum_host, uint32_t* cnt_host, uint8_t* img_host)
{
    int rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t cells = (size_t)p->W * p->H;
    mosaic_arena A;
    const auto o_acc = A.take<unsigned long long>(cells);
    const mosaic_layers L(A, cells, sum_host, cnt_host, img_host);
    const auto o_jobs = A.take<mosaic_job>(n); const auto o_rows = A.take<double>(rpy6 ? rows * 6 : 0); const auto o_flag = A.take<int>(1);
    rc = A.reserve(c); if (rc) return rc;
    unsigned long long* acc = A.at(o_acc); mosaic_job* d_jobs = A.at(o_jobs); int* d_flag = A.at(o_flag);
    std::vector<mosaic_job> jobs;
    rc = mosaic_fill_jobs(c, ids, n, rpy6, ping_off, A.at(o_rows), jobs); if (rc) return rc;
    rc = mosaic_render_acc(c, jobs, d_jobs, p, fp, acc, d_flag, A.opt(L.o_sum), A.opt(L.o_cnt), A.opt(L.o_img)); if (rc) return rc;
    rc = mosaic_flag_down(c, d_flag, "mosaic: a cell received more than 2^24 samples (cell %g too coarse for these frames)", p->cell); if (rc) return rc;
    rc = L.down(c, A); if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DSSS_OK;
}

int dsss_mosaic_render(dsss_ctx* c, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params* p,
                       uint32_t* sum_host, uint32_t* cnt_host, uint8_t* img_host)
{
    if (!c) return DSSS_E_ARG;
    size_t rows = 0;
    const int rc = mosaic_check_args(c, ids, n, rpy6, ping_off, p, &rows); if (rc) return rc;
    return render_run(c, ids, n, rpy6, ping_off, p, rows, nullptr, sum_host, cnt_host, img_host);
}

// ---- footprint rendering
void dsss_footprint_params_default(dsss_footprint_params* p) { if (p) { p->max_steps = 4; p->pad_ = 0; p->max_gap = 1.0; } }

int dsss_mosaic_footprint_steps(const dsss_footprint_params* fp, double cell, double sx, double sy, int32_t* n)
{
    if (!fp || !n || !footprint_params_ok(*fp) || !(cell > 0.0) || !std::isfinite(cell)) return DSSS_E_ARG;
    *n = footprint_steps(*fp, cell, sx, sy);
    return DSSS_OK;
}

int dsss_mosaic_render_footprint(dsss_ctx* c, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params* p,
                                 const dsss_footprint_params* fp, uint32_t* sum_host, uint32_t* cnt_host, uint8_t* img_host)
{
    if (!c) return DSSS_E_ARG;
    size_t rows = 0;
    int rc = mosaic_check_args(c, ids, n, rpy6, ping_off, p, &rows); if (rc) return rc;
    dsss_footprint_params F;
    rc = mosaic_check_footprint(c, ids, n, fp, &F); if (rc) return rc;
    return render_run(c, ids, n, rpy6, ping_off, p, rows, &F, sum_host, cnt_host, img_host);
}

// ---- range-gain normalisation
void dsss_gain_params_default(dsss_gain_params* p) { if (p) { p->min_count = 256; p->smooth = 0; p->target = 0; p->pad_ = 0; } }

// the argument rules of the two statistics entries; *M = the columns of the listed frames
static int gain_stats_check(dsss_ctx* c, const int* ids, int n, const uint64_t* sum_host, const uint64_t* cnt_host, int* M)
{
    if (!sum_host || !cnt_host) DSSS_FAIL(c, DSSS_E_ARG, "gain: nowhere to write the column %s", sum_host ? "counts" : "sums");
    size_t rows = 0;
    int rc = mosaic_check_frames(c, ids, n, nullptr, nullptr, true, &rows); if (rc) return rc;
    *M = c->frames[ids[0]].M;
    if (*M < 2) DSSS_FAIL(c, DSSS_E_ARG, "gain: frames of %d columns", *M);
    for (int i = 1; i < n; ++i)
        if (c->frames[ids[i]].M != *M) DSSS_FAIL(c, DSSS_E_ARG, "gain: frame %d has %d columns, frame %d has %d", ids[0], *M, ids[i], c->frames[ids[i]].M);
    return DSSS_OK;
}

static bool gain_bands_ok(const dsss_gain_bands* b)
{
    return b && b->nbands >= 1 && b->nbands <= BAND_MAX && std::isfinite(b->alt0) && std::isfinite(b->dalt) && b->dalt > 0.0;
}

// the rule of a caller's bands, with its message: the two banded entries that take a context
static int gain_check_bands(dsss_ctx* c, const dsss_gain_bands* b)
{
    if (!gain_bands_ok(b)) DSSS_FAIL(c, DSSS_E_ARG, "gain: bands %s", b ? "outside the rules (nbands 1..16, alt0 and dalt finite, dalt > 0)" : "missing");
    return DSSS_OK;
}

// The statistics of the listed frames per band and column (mosaic_gainstat_kernel; the column entry passes gain_one_band()): the one job
// table, launch and download of both entries.  The statistics are those of the uncorrected samples whatever table is set: the jobs carry
// the images, and the frame's altitudes (which one band never reads) with the caller's bands, alone.
static int gain_stats_run(dsss_ctx* c, const int* ids, int n, int use_mask, dsss_gain_bands bands, int M, uint64_t* sum_host, uint64_t* cnt_host)
{
    HIPCHK(c, hipSetDevice(c->device));
    const size_t entries = (size_t)M * bands.nbands;
    mosaic_arena A;
    const auto o_out = A.take<unsigned long long>(entries * 2); const auto o_jobs = A.take<mosaic_job>(n);
    int rc = A.reserve(c); if (rc) return rc;
    unsigned long long* d_out = A.at(o_out); mosaic_job* d_jobs = A.at(o_jobs);
    std::vector<mosaic_job> jobs(n);
    const int tpr = colstat_tpr(M), chunks = colstat_chunks(M), rows_wg = (256 / tpr) * COLSTAT_ROWS;
    const size_t lds = ((size_t)bands.nbands * 2 * COLSTAT_COLS * tpr) * sizeof(uint32_t) + (size_t)rows_wg;      // the table, then a band per row
    long long blocks = 0;
    for (int i = 0; i < n; ++i) {
        const dsss_frame& f = c->frames[ids[i]];
        jobs[i] = mosaic_job{ nullptr, nullptr, f.lvl[0], f.mask, nullptr, f.N, f.M, (int)blocks, 0, f.alt, bands };
        blocks += (long long)chunks * ((f.N + rows_wg - 1) / rows_wg);
    }
    if (blocks > 0x7fffffffll) DSSS_FAIL(c, DSSS_E_ARG, "gain: %d frames of %d columns are more than one launch takes", n, M);
    HIPCHK(c, hipMemcpyAsync(d_jobs, jobs.data(), (size_t)n * sizeof(mosaic_job), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d_out, 0, entries * 16, c->stream));
    if (blocks) hipLaunchKernelGGL(mosaic_gainstat_kernel, dim3((unsigned)blocks), dim3(256), lds, c->stream, d_jobs, n, use_mask != 0, d_out);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(sum_host, d_out, entries * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(cnt_host, d_out + entries, entries * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DSSS_OK;
}

int dsss_mosaic_gain_stats(dsss_ctx* c, const int* ids, int n, int use_mask, uint64_t* sum_host, uint64_t* cnt_host)
{
    if (!c) return DSSS_E_ARG;
    int M = 0;
    const int rc = gain_stats_check(c, ids, n, sum_host, cnt_host, &M); if (rc) return rc;
    return gain_stats_run(c, ids, n, use_mask, gain_one_band(), M, sum_host, cnt_host);
}

int dsss_mosaic_gain_stats_banded(dsss_ctx* c, const int* ids, int n, int use_mask, const dsss_gain_bands* bands, uint64_t* sum_host, uint64_t* cnt_host)
{
    if (!c) return DSSS_E_ARG;
    int rc = gain_check_bands(c, bands); if (rc) return rc;
    int M = 0;
    rc = gain_stats_check(c, ids, n, sum_host, cnt_host, &M); if (rc) return rc;
    return gain_stats_run(c, ids, n, use_mask, *bands, M, sum_host, cnt_host);
}

int dsss_gain_band(const dsss_gain_bands* bands, double alt, int32_t* band)
{
    if (!gain_bands_ok(bands) || !band) return DSSS_E_ARG;
    *band = gain_band(*bands, alt);
    return DSSS_OK;
}

// ---- the table rule, said once for the column and the banded table (S, C: one row of M sums and counts)
typedef unsigned __int128 u128;
struct gain_window { u128 s, n; };      // S', C'

// S and C of the columns within `smooth` of c on c's side: the window never crosses the nadir at M / 2
static gain_window gain_window_of(const uint64_t* S, const uint64_t* C, int M, int smooth, int c)
{
    const int half = M / 2;
    const int lo = std::max(c - smooth, c < half ? 0 : half), hi = std::min(c + smooth, c < half ? half - 1 : M - 1);
    gain_window w = { 0, 0 };
    for (int k = lo; k <= hi; ++k) { w.s += S[k]; w.n += C[k]; }
    return w;
}

// a window that gets a gain of its own
static bool gain_eligible(const gain_window& w, int min_count) { return w.n >= (u128)min_count && w.s > 0; }

// the Q8 gain that takes an eligible window's mean S' / C' to T, to the nearest, 65535 at most
static uint16_t gain_q8_of(u128 T, const gain_window& w)
{
    const u128 g = (T * w.n * 256 + w.s / 2) / w.s;
    return g > 65535 ? (uint16_t)65535 : (uint16_t)g;
}

int dsss_mosaic_gain_table(const uint64_t* sum, const uint64_t* cnt, int M, const dsss_gain_params* gp, uint16_t* gain_q8, int32_t* target_out)
{
    dsss_gain_params P;
    dsss_gain_params_default(&P);
    if (gp) P = *gp;
    if (!sum || !cnt || !gain_q8 || M < 2) return DSSS_E_ARG;
    if (P.min_count < 1 || P.smooth < 0 || P.smooth > 16 || P.target < 0 || P.target > 255) return DSSS_E_ARG;
    std::vector<gain_window> win(M);
    u128 tS = 0, tC = 0;
    bool any = false;
    for (int c = 0; c < M; ++c) {
        win[c] = gain_window_of(sum, cnt, M, P.smooth, c);
        if (gain_eligible(win[c], P.min_count)) { any = true; tS += sum[c]; tC += cnt[c]; }
    }
    u128 T = 0;
    if (any) { if (P.target) T = (u128)P.target; else if (tC > 0) T = (tS + tC / 2) / tC; else any = false; }
    for (int c = 0; c < M; ++c) gain_q8[c] = any && gain_eligible(win[c], P.min_count) ? gain_q8_of(T, win[c]) : (uint16_t)256;
    if (target_out) *target_out = any ? (int32_t)std::min<u128>(T, 0x7fffffff) : 0;
    return DSSS_OK;
}

int dsss_mosaic_gain_table_banded(const uint64_t* sum, const uint64_t* cnt, int M, int nbands, const dsss_gain_params* gp, uint16_t* gain_q8, int32_t* target_out)
{
    dsss_gain_params P;
    dsss_gain_params_default(&P);
    if (gp) P = *gp;
    if (!sum || !cnt || !gain_q8 || M < 2 || nbands < 1 || nbands > BAND_MAX) return DSSS_E_ARG;
    std::vector<uint64_t> Sp(M, 0), Cp(M, 0);
    for (int b = 0; b < nbands; ++b)
        for (int c = 0; c < M; ++c) { Sp[c] += sum[(size_t)b * M + c]; Cp[c] += cnt[(size_t)b * M + c]; }
    std::vector<uint16_t> pooled(M);
    int32_t Tp = 0;
    const int rc = dsss_mosaic_gain_table(Sp.data(), Cp.data(), M, &P, pooled.data(), &Tp); if (rc) return rc;      // (the parameter rules are its)
    for (int b = 0; b < nbands; ++b)
        for (int c = 0; c < M; ++c) {
            const gain_window w = gain_window_of(sum + (size_t)b * M, cnt + (size_t)b * M, M, P.smooth, c);
            gain_q8[(size_t)b * M + c] = gain_eligible(w, P.min_count) && Tp > 0 ? gain_q8_of((u128)Tp, w) : pooled[c];      // a thin band: the pooled column
        }
    if (target_out) *target_out = Tp;
    return DSSS_OK;
}

// The new table goes into a block of its own and takes the old one's place only after its upload succeeded: an error leaves the old
// table in force.  (Every entry that reads the table synchronises before it returns, so no queued kernel still reads the old block.)
static int gain_install(dsss_ctx* c, const uint16_t* gain_q8_host, int M, const dsss_gain_bands& bands)
{
    if (!gain_q8_host) { c->mosaic_gain_M = 0; c->mosaic_bands = gain_one_band(); ++c->gain_epoch; return DSSS_OK; }
    if (M < 2) DSSS_FAIL(c, DSSS_E_ARG, "gain: a table of %d columns", M);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)M * bands.nbands * sizeof(uint16_t);
    dsss_buf nb{"mosaic_gain"};
    const int rc = nb.reserve(c, bytes); if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(nb.p, gain_q8_host, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->mosaic_gain = std::move(nb); c->mosaic_gain_M = M; c->mosaic_bands = bands; c->mosaic_bands.pad_ = 0; ++c->gain_epoch;
    return DSSS_OK;
}

int dsss_mosaic_gain_set(dsss_ctx* c, const uint16_t* gain_q8_host, int M)
{
    if (!c) return DSSS_E_ARG;
    return gain_install(c, gain_q8_host, M, gain_one_band());
}

int dsss_mosaic_gain_set_banded(dsss_ctx* c, const uint16_t* gain_q8_host, int M, const dsss_gain_bands* bands)
{
    if (!c) return DSSS_E_ARG;
    if (!gain_q8_host) return gain_install(c, nullptr, 0, gain_one_band());
    const int rc = gain_check_bands(c, bands); if (rc) return rc;
    return gain_install(c, gain_q8_host, M, *bands);
}

// the table in force, all its bands, read back from the device copy
static int gain_download(dsss_ctx* c, uint16_t* gain_q8_host, int cap)
{
    const long long need = (long long)c->mosaic_gain_M * c->mosaic_bands.nbands;
    if (!gain_q8_host || cap < need)
        DSSS_FAIL(c, DSSS_E_ARG, "gain: a table of %d bands x %d columns, room for %d gains", c->mosaic_bands.nbands, c->mosaic_gain_M, gain_q8_host ? cap : 0);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(gain_q8_host, c->mosaic_gain.p, (size_t)need * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DSSS_OK;
}

int dsss_mosaic_gain_get(dsss_ctx* c, uint16_t* gain_q8_host, int cap, int* M)
{
    if (!c) return DSSS_E_ARG;
    if (!M) DSSS_FAIL(c, DSSS_E_ARG, "gain: nowhere to write the number of columns");
    if (c->mosaic_gain_M && c->mosaic_bands.nbands > 1)
        DSSS_FAIL(c, DSSS_E_STATE, "gain: a table of %d bands is set (dsss_mosaic_gain_get_banded reads it)", c->mosaic_bands.nbands);
    *M = c->mosaic_gain_M;                                                      // also when there is no room for them: the caller learns how many
    if (!c->mosaic_gain_M) return DSSS_OK;
    return gain_download(c, gain_q8_host, cap);
}

int dsss_mosaic_gain_get_banded(dsss_ctx* c, uint16_t* gain_q8_host, int cap, int* M, dsss_gain_bands* bands)
{
    if (!c) return DSSS_E_ARG;
    if (!M || !bands) DSSS_FAIL(c, DSSS_E_ARG, "gain: nowhere to write the %s", M ? "bands" : "number of columns");
    *M = c->mosaic_gain_M; *bands = c->mosaic_bands;                            // also when there is no room for the gains
    if (!c->mosaic_gain_M) return DSSS_OK;
    return gain_download(c, gain_q8_host, cap);
}

int dsss_frame_get_corrected(dsss_ctx* c, int id, uint8_t* out_host)
{
    if (!c) return DSSS_E_ARG;
    if (!out_host) DSSS_FAIL(c, DSSS_E_ARG, "corrected waterfall: nowhere to write it");
    if (id < 0 || id >= c->max_frames) DSSS_FAIL(c, DSSS_E_ARG, "frame id %d out of range [0,%d)", id, c->max_frames);
    const dsss_frame& f = c->frames[id];
    if (!f.has_geom || !f.has_norm || !f.lvl[0] || !f.mask) DSSS_FAIL(c, DSSS_E_STATE, "frame %d not extracted yet", id);
    int rc = mosaic_check_gain(c, &id, 1); if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)f.N * f.M;
    mosaic_arena A;
    const auto o_out = A.take<uint8_t>(bytes);
    rc = A.reserve(c); if (rc) return rc;
    std::vector<mosaic_job> jobs;
    rc = mosaic_fill_jobs(c, &id, 1, nullptr, nullptr, nullptr, jobs); if (rc) return rc;
    hipLaunchKernelGGL(mosaic_correct_kernel, dim3((unsigned)f.N), dim3(256), 0, c->stream, jobs[0], A.at(o_out));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out_host, A.at(o_out), bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DSSS_OK;
}

int dsss_mosaic_consistency(dsss_ctx* c, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params* p,
                            uint32_t* nfr_host, uint32_t* s1_host, uint32_t* s2_host, double* score_host)
{
    if (!c) return DSSS_E_ARG;
    size_t rows = 0;
    int rc = mosaic_check_args(c, ids, n, rpy6, ping_off, p, &rows); if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t cells = (size_t)p->W * p->H;
    // every frame is rendered alone into a window of the grid: the cells its geo extremes can reach
    std::vector<mosaic_win> wins(n); std::vector<char> on_grid(n, 0);
    size_t win_cells = 1;
    for (int i = 0; i < n; ++i) {
        const dsss_frame& f = c->frames[ids[i]];
        if (!mosaic_window(f, rpy6 ? rpy6 + (size_t)ping_off[i] * 6 : f.h_geo, 0, f.N, p, &wins[i])) continue;
        on_grid[i] = 1;
        win_cells = std::max(win_cells, (size_t)wins[i].bw * wins[i].bh);
    }
    mosaic_arena A;
    const auto o_lay = A.take<uint32_t>(cells * 3); const auto o_win = A.take<unsigned long long>(win_cells);      // lay: nfr, s1, s2 behind one another
    const auto o_jobs = A.take<mosaic_job>(n); const auto o_rows = A.take<double>(rpy6 ? rows * 6 : 0); const auto o_flag = A.take<int>(1);
    rc = A.reserve(c); if (rc) return rc;
    uint32_t* d_nfr = A.at(o_lay); uint32_t* d_s1 = d_nfr + cells; uint32_t* d_s2 = d_s1 + cells;
    unsigned long long* d_win = A.at(o_win); mosaic_job* d_jobs = A.at(o_jobs); int* d_flag = A.at(o_flag);
    std::vector<mosaic_job> jobs;
    rc = mosaic_fill_jobs(c, ids, n, rpy6, ping_off, A.at(o_rows), jobs); if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(d_jobs, jobs.data(), (size_t)n * sizeof(mosaic_job), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d_nfr, 0, cells * 12, c->stream));
    HIPCHK(c, hipMemsetAsync(d_flag, 0, sizeof(int), c->stream));
    for (int i = 0; i < n; ++i) {
        if (!on_grid[i]) continue;
        const size_t wc = (size_t)wins[i].bw * wins[i].bh;
        HIPCHK(c, hipMemsetAsync(d_win, 0, wc * 8, c->stream));
        launch_scatter(c, d_jobs + i, 1, jobs[i].N, wins[i], d_win);
        hipLaunchKernelGGL(mosaic_fold_kernel, dim3((unsigned)((wc + 255) / 256)), dim3(256), 0, c->stream, d_win, wins[i], d_nfr, d_s1, d_s2, d_flag);
        HIPCHK(c, hipGetLastError());
    }
    rc = mosaic_flag_down(c, d_flag, "mosaic: a cell received more than 2^24 samples of one frame (cell %g too coarse)", p->cell); if (rc) return rc;
    // the score needs the three layers whether the caller wants them or not
    std::vector<uint32_t> own[3];
    uint32_t* host[3] = { nfr_host, s1_host, s2_host };
    if (!score_host && !nfr_host && !s1_host && !s2_host) return DSSS_OK;
    for (int k = 0; k < 3; ++k) {
        if (!host[k]) { if (!score_host) continue; own[k].resize(cells); host[k] = own[k].data(); }
        HIPCHK(c, hipMemcpyAsync(host[k], d_nfr + (size_t)k * cells, cells * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (score_host) {
        double num = 0.0, den = 0.0;
        for (size_t g = 0; g < cells; ++g) {
            const uint32_t k = host[0][g];
            if (k < 2) continue;
            const double a = (double)host[1][g];
            num += (double)host[2][g] - a * a / (double)k;
            den += (double)(k - 1);
        }
        *score_host = (den > 0.0 && num > 0.0) ? sqrt(num / den) : 0.0;
    }
    return DSSS_OK;
}

} // extern "C"

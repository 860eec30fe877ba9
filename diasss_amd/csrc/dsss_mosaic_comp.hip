// diasss_amd/csrc/dsss_mosaic_comp.hip -- the composite mosaic (include/dsss.h, "composite mosaic"): one winning sample per cell under
// a priority, with its source, and the fill of enclosed holes.  Three kernels: the scatter takes the minimum of the samples' keys per
// cell, the resolve turns a key back into value and source, the fill gives an enclosed hole its donor's.  Keys are integers and the
// minimum is associative and commutative, so the layers do not depend on the order of ids, of the atomics or of the call.
#include "dsss_mosaic_int.h"
#include "dsss_wave.h"
#include <algorithm>
#include <numeric>

namespace {

#define FILL_TX 32                         // a fill workgroup's tile of cells: 32 x 8, with a halo of R <= COMP_MAX_FILL
#define FILL_TY 8

// mosaic_scatter_kernel's launch shape: one workgroup per ping, the job table, the bearing of each side once per ping through LDS,
// and the sample is binned by the one body (mosaic_sample_cell).  All samples of a ping share g, so within a wavefront the order of
// two keys is that of (q, col): 31 bits.  Lanes that hit the cell of their neighbour form runs; the minimum of a run is taken with the
// segmented scan of the mean scatter (mosaic_run_reduce: min for +) and the last lane of the run issues ONE 64-bit atomicMin without return.
__global__ __launch_bounds__(256) void mosaic_composite_kernel(const mosaic_job* __restrict__ jobs, int njobs, mosaic_win G, int mode,
                                                               unsigned long long* __restrict__ keys)
{
    __shared__ double s_sc[4];
    mosaic_job J; int row; const double* P;
    if (!mosaic_ping_of(jobs, njobs, s_sc, J, row, P)) return;
    const int M = J.M;
    const uint8_t* __restrict__ img = J.img + (size_t)row * M;
    const uint8_t* __restrict__ mask = J.mask + (size_t)row * M;
    const unsigned long long gbits = (unsigned long long)(unsigned)(J.g0 + row) << 16;
    for (int c0 = 0; c0 < M; c0 += 256) {
        const int col = c0 + (int)threadIdx.x;
        unsigned unused;
        const int cell = mosaic_sample_cell(P, s_sc, J, img, mask, col, G, &unused);
        unsigned v = cell >= 0 ? ((unsigned)comp_rank(mode, M, col) << 16) | (unsigned)col : ~0u;      // q << 16 | col; ~0u: no sample
        const bool tail = mosaic_run_reduce(cell, v, [](unsigned a, unsigned b) { return min(a, b); });
        if (tail && cell >= 0) atomicMin(&keys[cell], ((unsigned long long)(v >> 16) << 47) | gbits | (v & 0xffffu));
    }
}

// The footprint form ("footprint rendering" in the header), in the same launch shape: the ping's prologue in the partner form, the
// sub-samples by the one body of the footprint kernels (mosaic_footprint_samples).  A sub-sample competes with its parent's q << 16 | col,
// so the sub-samples of one parent in a cell are one key: the minimum over a run and the atomicMin see them as one sample.
__global__ __launch_bounds__(256) void mosaic_composite_fp_kernel(const mosaic_job* __restrict__ jobs, int njobs, mosaic_win G, dsss_footprint_params F,
                                                                  int mode, unsigned long long* __restrict__ keys)
{
    __shared__ double s_sc[8];
    mosaic_job J; int row; const double* P; const double* PP; bool last;
    if (!mosaic_ping_of(jobs, njobs, s_sc, J, row, P, &PP, &last)) return;
    const int M = J.M;
    const unsigned long long gbits = (unsigned long long)(unsigned)(J.g0 + row) << 16;
    mosaic_footprint_samples(P, PP, last, s_sc, J, row, G, F,
        [&](int col) { return ((unsigned)comp_rank(mode, M, col) << 16) | (unsigned)col; },
        [&](int cell, unsigned k) {
            unsigned v = cell >= 0 ? k : ~0u;
            const bool tail = mosaic_run_reduce(cell, v, [](unsigned a, unsigned b) { return min(a, b); });
            if (tail && cell >= 0) atomicMin(&keys[cell], ((unsigned long long)(v >> 16) << 47) | gbits | (v & 0xffffu));
        });
}

// One thread per cell and RESOLVE_CELLS cells after one another per thread: the key back into the winner's value and source.  The frame
// of g by binary search over the jobs' g0, which the host sorts by frame id and hence by g0; ids[j] = the frame id of job j.  The g0 of up
// to RESOLVE_G0 jobs are staged in LDS; a longer table is searched where it lies (a search per cell on another key and from two places:
// its own two lines, not mosaic_job_of, which a key and an accessor as parameters would only obscure).  fill gets 0 / 255 here (mosaic_fill_kernel overwrites
// the holes it fills).  The cells that hold a sample are counted with a wave sum and one integer atomic per wavefront -- after its
// RESOLVE_CELLS cells, and into one of COMP_SLOTS counters the host adds up: with an atomic per 64 cells on ONE address the kernel ran at
// the rate of that address (6.9 ms for 41 M cells where this takes 0.2: DESIGN.md, "Composite mosaic").
#define RESOLVE_G0 1024
#define RESOLVE_CELLS 8
#define COMP_SLOTS 32                      // counts[0 .. COMP_SLOTS): cells that hold a sample; counts[COMP_SLOTS]: cells filled
__global__ __launch_bounds__(256) void mosaic_resolve_kernel(const unsigned long long* __restrict__ keys, size_t n, const mosaic_job* __restrict__ jobs,
                                                             const int* __restrict__ ids, int njobs, uint8_t* __restrict__ img, int32_t* __restrict__ src_frame,
                                                             int32_t* __restrict__ src_ping, int32_t* __restrict__ src_col, uint8_t* __restrict__ fill,
                                                             unsigned long long* __restrict__ counts)
{
    __shared__ int s_g0[RESOLVE_G0];
    const bool staged = njobs <= RESOLVE_G0;                                       // (uniform per launch)
    if (staged) {
        for (int j = (int)threadIdx.x; j < njobs; j += 256) s_g0[j] = jobs[j].g0;
        __syncthreads();
    }
    int held = 0;
    for (int c = 0; c < RESOLVE_CELLS; ++c) {
        const size_t i = ((size_t)blockIdx.x * RESOLVE_CELLS + c) * 256 + threadIdx.x;
        if (i >= n) break;
        const unsigned long long k = keys[i];
        const bool has = k != COMP_EMPTY;
        int v = 0, fr = -1, row = -1, col = -1;
        if (has) {
            const int g = (int)((k >> 16) & 0x7fffffffull);
            col = (int)(k & 0xffffull);
            int lo = 0, hi = njobs - 1;
            if (staged) while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (s_g0[mid] <= g) lo = mid; else hi = mid - 1; }
            else while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (jobs[mid].g0 <= g) lo = mid; else hi = mid - 1; }
            const mosaic_job& J = jobs[lo];
            row = g - J.g0; fr = ids[lo];
            if (img) v = (int)mosaic_gain_apply(J.img[(size_t)row * J.M + col], mosaic_gain_row(J, row), col);      // the band of the winning ping
            ++held;
        }
        if (img) img[i] = (uint8_t)v;
        if (src_frame) src_frame[i] = fr;
        if (src_ping) src_ping[i] = row;
        if (src_col) src_col[i] = col;
        if (fill) fill[i] = has ? (uint8_t)0 : (uint8_t)255;
    }
    const int total = dsss_wave_sum(held);
    if ((threadIdx.x & 63) == 0 && total) atomicAdd(&counts[blockIdx.x % COMP_SLOTS], (unsigned long long)total);
}

struct lds_valid {                         // the validity tile of mosaic_fill_kernel: (x, y) relative to the tile's first cell
    const uint8_t* s; int R, pitch;
    __device__ int operator()(int x, int y) const { return s[(y + R) * pitch + (x + R)]; }
};

// A workgroup owns a tile of FILL_TX x FILL_TY cells and stages the validity of the tile plus a halo of R in LDS: read from the KEYS,
// never from an output layer, so a hole's store is never another hole's input; cells outside the grid are staged as not valid.  An
// empty cell that is enclosed (comp_fill_rule) copies its donor's resolved value and source: the donor is a cell of V0, which this
// kernel never writes.  counts[COMP_SLOTS] += the cells filled: few, so one address serves; the cells left empty are what remains of W H
// (with an atomic per wavefront that holds an empty cell too, on one address, the kernel took 1.48 ms where this takes 0.25).
__global__ __launch_bounds__(256) void mosaic_fill_kernel(const unsigned long long* __restrict__ keys, int W, int H, int R, int tiles_x,
                                                          uint8_t* __restrict__ img, int32_t* __restrict__ src_frame, int32_t* __restrict__ src_ping,
                                                          int32_t* __restrict__ src_col, uint8_t* __restrict__ fill, unsigned long long* __restrict__ counts)
{
    __shared__ uint8_t s_valid[(FILL_TX + 2 * COMP_MAX_FILL) * (FILL_TY + 2 * COMP_MAX_FILL)];
    const int ty0 = ((int)blockIdx.x / tiles_x) * FILL_TY, tx0 = ((int)blockIdx.x % tiles_x) * FILL_TX;
    const int pitch = FILL_TX + 2 * R, rows = FILL_TY + 2 * R;
    for (int j = (int)threadIdx.x; j < pitch * rows; j += 256) {
        const int y = ty0 - R + j / pitch, x = tx0 - R + j % pitch;
        s_valid[j] = (x >= 0 && x < W && y >= 0 && y < H && keys[(size_t)y * W + x] != COMP_EMPTY) ? 1 : 0;
    }
    __syncthreads();
    const int lx = (int)threadIdx.x % FILL_TX, ly = (int)threadIdx.x / FILL_TX;
    const int ix = tx0 + lx, iy = ty0 + ly;
    const lds_valid valid{ s_valid, R, pitch };
    int filled = 0;
    if (ix < W && iy < H && !valid(lx, ly)) {
        int dx, dy;
        const int d2 = comp_fill_rule(valid, lx, ly, R, &dx, &dy);
        if (d2) {
            const size_t i = (size_t)iy * W + ix, j = (size_t)(iy + dy) * W + (ix + dx);
            if (img) img[i] = img[j];
            if (src_frame) src_frame[i] = src_frame[j];
            if (src_ping) src_ping[i] = src_ping[j];
            if (src_col) src_col[i] = src_col[j];
            if (fill) fill[i] = (uint8_t)d2;
            filled = 1;
        }
    }
    const int tot = dsss_wave_sum(filled);
    if ((threadIdx.x & 63) == 0 && tot) atomicAdd(&counts[COMP_SLOTS], (unsigned long long)tot);
}

struct host_valid {
    const uint8_t* v; int W, H;
    int operator()(int x, int y) const { return x >= 0 && x < W && y >= 0 && y < H && v[(size_t)y * W + x] != 0 ? 1 : 0; }
};

} // namespace

extern "C" {

void dsss_comp_params_default(dsss_comp_params* p) { if (p) { p->mode = DSSS_COMP_NEAR; p->fill_radius = 0; } }

int dsss_mosaic_comp_rank(int mode, int M, int col, int32_t* q)
{
    if (!q || mode < 0 || mode > DSSS_COMP_FIRST || M < 4 || (M & 1) || M > COMP_MAX_M || col < 0 || col >= M) return DSSS_E_ARG;
    *q = comp_rank(mode, M, col);
    return DSSS_OK;
}

int dsss_mosaic_fill_host(const uint8_t* valid, int W, int H, int R, int32_t* donor, uint8_t* fill)
{
    if (!valid || !donor || !fill || W < 1 || H < 1 || (long long)W * H > MOSAIC_MAX_CELLS || R < 0 || R > COMP_MAX_FILL) return DSSS_E_ARG;
    const host_valid V{ valid, W, H };
    for (int iy = 0; iy < H; ++iy)
        for (int ix = 0; ix < W; ++ix) {
            const size_t i = (size_t)iy * W + ix;
            if (valid[i]) { donor[i] = (int32_t)i; fill[i] = 0; continue; }
            int dx = 0, dy = 0;
            const int d2 = comp_fill_rule(V, ix, iy, R, &dx, &dy);
            if (d2) { donor[i] = (int32_t)((size_t)(iy + dy) * W + (ix + dx)); fill[i] = (uint8_t)d2; }
            else { donor[i] = -1; fill[i] = 255; }
        }
    return DSSS_OK;
}

// the argument rules of both composite entries: those of the mean render, then the composite's parameters (*P: the caller's or the
// defaults) and the frames' M; *rows = the pings of the listed frames
static int comp_check(dsss_ctx* c, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params* p,
                      const dsss_comp_params* cp, dsss_comp_params* P, size_t* rows)
{
    const int rc = mosaic_check_args(c, ids, n, rpy6, ping_off, p, rows); if (rc) return rc;
    dsss_comp_params_default(P);
    if (cp) *P = *cp;
    if (P->mode < 0 || P->mode > DSSS_COMP_FIRST) DSSS_FAIL(c, DSSS_E_ARG, "composite: mode %d", P->mode);
    if (P->fill_radius < 0 || P->fill_radius > COMP_MAX_FILL) DSSS_FAIL(c, DSSS_E_ARG, "composite: fill_radius %d outside 0..%d", P->fill_radius, COMP_MAX_FILL);
    for (int i = 0; i < n; ++i) {
        const int M = c->frames[ids[i]].M;
        if (M < 4 || (M & 1) || M > COMP_MAX_M) DSSS_FAIL(c, DSSS_E_ARG, "composite: frame %d has %d columns (even, 4..%d)", ids[i], M, COMP_MAX_M);
    }
    return DSSS_OK;
}

// The composite behind the argument checks, for both entries: fp == null scatters the samples as points (mosaic_composite_kernel),
// otherwise the sub-samples of their footprints (mosaic_composite_fp_kernel); resolve, fill, counts and downloads are the same.
static int comp_run(dsss_ctx* c, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params* p, size_t rows,
                    const dsss_comp_params& P, const dsss_footprint_params* fp, uint8_t* img_host, int32_t* src_frame_host, int32_t* src_ping_host,
                    int32_t* src_col_host, uint8_t* fill_host, dsss_comp_info* info_host)
{
    int rc;
    HIPCHK(c, hipSetDevice(c->device));
    // the canonical order: ascending frame id, whatever the order of ids; the job table is sorted by it and hence by g0 and blk0
    std::vector<int> order(n);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return ids[a] < ids[b]; });
    std::vector<int> sid(n), soff(n);
    for (int i = 0; i < n; ++i) { sid[i] = ids[order[i]]; soff[i] = rpy6 ? ping_off[order[i]] : 0; }
    const size_t cells = (size_t)p->W * p->H;
    const int R = P.fill_radius;
    // the fill copies a donor's resolved layers, so the layers asked for live on the device; nothing else does
    mosaic_arena A;
    const auto o_keys = A.take<unsigned long long>(cells);
    const auto o_img = A.take<uint8_t>(img_host ? cells : 0);
    const auto o_fr = A.take<int32_t>(src_frame_host ? cells : 0), o_pg = A.take<int32_t>(src_ping_host ? cells : 0), o_col = A.take<int32_t>(src_col_host ? cells : 0);
    const auto o_fill = A.take<uint8_t>(fill_host ? cells : 0);
    const auto o_jobs = A.take<mosaic_job>(n); const auto o_ids = A.take<int>(n); const auto o_rows = A.take<double>(rpy6 ? rows * 6 : 0);
    const auto o_cnt = A.take<unsigned long long>(COMP_SLOTS + 1);
    rc = A.reserve(c); if (rc) return rc;
    unsigned long long* d_keys = A.at(o_keys); mosaic_job* d_jobs = A.at(o_jobs); int* d_ids = A.at(o_ids); unsigned long long* d_cnt = A.at(o_cnt);
    uint8_t* d_img = A.opt(o_img); int32_t* d_fr = A.opt(o_fr); int32_t* d_pg = A.opt(o_pg); int32_t* d_col = A.opt(o_col); uint8_t* d_fill = A.opt(o_fill);
    std::vector<mosaic_job> jobs;
    rc = mosaic_fill_jobs(c, sid.data(), n, rpy6, soff.data(), A.at(o_rows), jobs); if (rc) return rc;
    int g0 = 0;                                                                    // (mosaic_check_frames: fewer than 2^31 pings in all)
    for (int i = 0; i < n; ++i) { jobs[i].blk0 = g0; jobs[i].g0 = g0; g0 += jobs[i].N; }
    HIPCHK(c, hipMemcpyAsync(d_jobs, jobs.data(), (size_t)n * sizeof(mosaic_job), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_ids, sid.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d_keys, 0xff, cells * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(d_cnt, 0, (COMP_SLOTS + 1) * sizeof(unsigned long long), c->stream));
    const mosaic_win G = mosaic_grid_win(p);
    if (g0 && !fp) hipLaunchKernelGGL(mosaic_composite_kernel, dim3((unsigned)g0), dim3(256), 0, c->stream, d_jobs, n, G, P.mode, d_keys);
    if (g0 && fp) hipLaunchKernelGGL(mosaic_composite_fp_kernel, dim3((unsigned)g0), dim3(256), 0, c->stream, d_jobs, n, G, *fp, P.mode, d_keys);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(mosaic_resolve_kernel, dim3((unsigned)((cells + 256 * RESOLVE_CELLS - 1) / (256 * RESOLVE_CELLS))), dim3(256), 0, c->stream, d_keys, cells, d_jobs, d_ids, n,
                       d_img, d_fr, d_pg, d_col, d_fill, d_cnt);
    HIPCHK(c, hipGetLastError());
    if (R > 0) {
        const int tiles_x = (p->W + FILL_TX - 1) / FILL_TX, tiles_y = (p->H + FILL_TY - 1) / FILL_TY;      // at most 2^28 / 256 + 2^23 + 2^25 + 1 tiles
        hipLaunchKernelGGL(mosaic_fill_kernel, dim3((unsigned)((size_t)tiles_x * tiles_y)), dim3(256), 0, c->stream, d_keys, p->W, p->H, R, tiles_x,
                           d_img, d_fr, d_pg, d_col, d_fill, d_cnt);
        HIPCHK(c, hipGetLastError());
    }
    unsigned long long cnt[COMP_SLOTS + 1] = { 0 };
    if (info_host) HIPCHK(c, hipMemcpyAsync(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
    if (img_host) HIPCHK(c, hipMemcpyAsync(img_host, d_img, cells, hipMemcpyDeviceToHost, c->stream));
    if (src_frame_host) HIPCHK(c, hipMemcpyAsync(src_frame_host, d_fr, cells * 4, hipMemcpyDeviceToHost, c->stream));
    if (src_ping_host) HIPCHK(c, hipMemcpyAsync(src_ping_host, d_pg, cells * 4, hipMemcpyDeviceToHost, c->stream));
    if (src_col_host) HIPCHK(c, hipMemcpyAsync(src_col_host, d_col, cells * 4, hipMemcpyDeviceToHost, c->stream));
    if (fill_host) HIPCHK(c, hipMemcpyAsync(fill_host, d_fill, cells, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (info_host) {
        unsigned long long direct = 0;
        for (int k = 0; k < COMP_SLOTS; ++k) direct += cnt[k];
        info_host->direct = (int64_t)direct; info_host->filled = (int64_t)cnt[COMP_SLOTS];
        info_host->empty = (int64_t)(cells - direct - cnt[COMP_SLOTS]);
    }
    return DSSS_OK;
}

int dsss_mosaic_composite(dsss_ctx* c, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params* p,
                          const dsss_comp_params* cp, uint8_t* img_host, int32_t* src_frame_host, int32_t* src_ping_host, int32_t* src_col_host,
                          uint8_t* fill_host, dsss_comp_info* info_host)
{
    if (!c) return DSSS_E_ARG;
    size_t rows = 0;
    dsss_comp_params P;
    const int rc = comp_check(c, ids, n, rpy6, ping_off, p, cp, &P, &rows); if (rc) return rc;
    return comp_run(c, ids, n, rpy6, ping_off, p, rows, P, nullptr, img_host, src_frame_host, src_ping_host, src_col_host, fill_host, info_host);
}

int dsss_mosaic_composite_footprint(dsss_ctx* c, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params* p,
                                    const dsss_comp_params* cp, const dsss_footprint_params* fp, uint8_t* img_host, int32_t* src_frame_host,
                                    int32_t* src_ping_host, int32_t* src_col_host, uint8_t* fill_host, dsss_comp_info* info_host)
{
    if (!c) return DSSS_E_ARG;
    size_t rows = 0;
    dsss_comp_params P;
    int rc = comp_check(c, ids, n, rpy6, ping_off, p, cp, &P, &rows); if (rc) return rc;
    dsss_footprint_params F;
    rc = mosaic_check_footprint(c, ids, n, fp, &F); if (rc) return rc;
    return comp_run(c, ids, n, rpy6, ping_off, p, rows, P, &F, img_host, src_frame_host, src_ping_host, src_col_host, fill_host, info_host);
}

} // extern "C"

// diasss_amd/csrc/dsss_mosaic_profile.hip -- per-ping disagreement profile (include/dsss_profile.h): every ping of a frame held against
// the mosaic of all other frames.  The one gather of the mosaic family: a frame's own accumulators A_f are scattered into its window of
// the grid by the scatter kernel as it is, and mosaic_profile_kernel bins the frame's samples once more, reads the map's accumulator
// and the frame's own at each sample's cell and forms the mosaic of the others as ONE 64-bit subtraction.  Integers throughout and no
// atomics in the gather, so the records depend on no order.
#include "dsss_mosaic_profile.h"
#include "dsss_wave.h"
#include <algorithm>

namespace {

// the windows of the frames of one batch share an arena of this many cells (256 MB of accumulators), or of the grid's cells where
// the grid is larger: a window is at most the grid
constexpr size_t PROFILE_ARENA_CELLS = (size_t)1 << 25;

// One workgroup per ping, 256 threads, in the launch shape of mosaic_scatter_kernel: job lookup and ping prologue by mosaic_ping_of,
// every sample binned by mosaic_sample_cell with the frame's window as G -- the mask, cell and gain rules stay in their one place.  The
// cell of the grid follows from the cell of the window.  A lane reads A[g] and A_f[key], subtracts them as one u64 (the frame's sum and
// count are each at most the map's: no borrow crosses the words; mosaic_acc takes the difference apart and forms the mean), tests the
// count of the others against min_count and forms d.
// A lane keeps the five integers of either side in registers over the c0 loop (M / 2 need not be a multiple of 256: a lane's column
// changes sides once, so both sets are live); sd is summed as u32, which is the i32 sum modulo 2^32.  The ten integers are summed over
// the wavefront (dsss_wave_sum), the four wavefronts through LDS, and ten lanes of the first wavefront store the ping's record with
// ordinary stores.  DIFF: the ping's row of the residual layer is written in the same loop, consecutive lanes consecutive int16.
template <bool DIFF>
__global__ __launch_bounds__(256) void mosaic_profile_kernel(const prof_job* __restrict__ jobs, int njobs, mosaic_win G, const unsigned long long* __restrict__ acc,
                                                             const unsigned long long* __restrict__ own, uint32_t min_count, dsss_ping_stat* __restrict__ stats,
                                                             int16_t* __restrict__ diff)
{
    __shared__ double s_sc[4];
    __shared__ uint32_t s_red[4][10];
    prof_job J; int row; const double* P;
    if (!mosaic_ping_of(jobs, njobs, s_sc, J, row, P)) return;
    G.ox = J.ox; G.oy = J.oy; G.bw = J.bw; G.bh = J.bh;                           // (bw = 0: no cell of the frame lies on the grid, every key is -1)
    own += J.woff;
    const int M = J.M, half = M / 2;
    const uint8_t* __restrict__ img = J.img + (size_t)row * M;
    const uint8_t* __restrict__ mask = J.mask + (size_t)row * M;
    int16_t* __restrict__ drow = DIFF ? diff + J.diff0 + (size_t)row * M : nullptr;
    uint32_t a0[5] = { 0, 0, 0, 0, 0 }, a1[5] = { 0, 0, 0, 0, 0 };                  // binned, n, sad, ssd, sd of port and of starboard
    for (int c0 = 0; c0 < M; c0 += 256) {
        const int col = c0 + (int)threadIdx.x;
        unsigned v = 0;
        const int key = mosaic_sample_cell(P, s_sc, J, img, mask, col, G, &v);
        uint32_t e[5] = { 0, 0, 0, 0, 0 };
        int d = DSSS_PROFILE_NONE;
        if (key >= 0) {
            const int iy = key / G.bw, ix = key - iy * G.bw;
            const mosaic_acc o(acc[(size_t)(G.oy + iy) * G.W + (G.ox + ix)] - own[key]);
            e[0] = 1;
            if (o.c >= min_count) {
                d = (int)v - (int)o.mean();
                e[1] = 1; e[2] = (uint32_t)(d < 0 ? -d : d); e[3] = (uint32_t)(d * d); e[4] = (uint32_t)d;
            }
        }
        const bool starboard = col >= half;
#pragma unroll
        for (int k = 0; k < 5; ++k) { a0[k] += starboard ? 0u : e[k]; a1[k] += starboard ? e[k] : 0u; }
        if (DIFF && col < M) drow[col] = (int16_t)d;
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 5; ++k) {                                                  // the record's order: binned[2], n[2], sad[2], ssd[2], sd[2]
        const uint32_t p = dsss_wave_sum(a0[k]), s = dsss_wave_sum(a1[k]);
        if (lane == 0) { s_red[w][2 * k] = p; s_red[w][2 * k + 1] = s; }
    }
    __syncthreads();
    if (threadIdx.x < 10) {
        uint32_t* __restrict__ out = reinterpret_cast<uint32_t*>(stats + J.ping0 + (size_t)row);
        out[threadIdx.x] = s_red[0][threadIdx.x] + s_red[1][threadIdx.x] + s_red[2][threadIdx.x] + s_red[3][threadIdx.x];
    }
}

static_assert(sizeof(dsss_ping_stat) == 40, "the kernel stores a record as ten u32");

} // namespace

int profile_check_params(dsss_ctx* c, const dsss_profile_params* pp, int* min_count)
{
    dsss_profile_params P;
    dsss_profile_params_default(&P);
    if (pp) P = *pp;
    if (P.min_count < 1 || P.min_count > DSSS_PROFILE_MAX_MIN_COUNT) DSSS_FAIL(c, DSSS_E_ARG, "profile: min_count %d (1..2^24)", P.min_count);
    *min_count = P.min_count;
    return DSSS_OK;
}

int profile_check_frame(dsss_ctx* c, int id)
{
    if (c->frames[id].M > DSSS_PROFILE_MAX_M) DSSS_FAIL(c, DSSS_E_ARG, "profile: frame %d has %d columns (at most %d: the sums of a side are 32 bits)", id, c->frames[id].M, DSSS_PROFILE_MAX_M);
    return DSSS_OK;
}

void profile_plan::take(mosaic_arena& A, size_t grid_cells)
{
    pings = 0; samples = 0;
    for (const profile_frame& f : frames) { pings += (size_t)f.job.N; samples += (size_t)f.job.N * f.job.M; }
    // a window is at most the grid, so every frame fits the arena, and the windows themselves are not needed yet
    arena_cells = std::max<size_t>(1, std::min(frames.size() * grid_cells, std::max(PROFILE_ARENA_CELLS, grid_cells)));
    o_win = A.take<unsigned long long>(arena_cells);
    o_sjobs = A.take<mosaic_job>(frames.size()); o_pjobs = A.take<prof_job>(frames.size());
    o_stats = A.take<dsss_ping_stat>(pings); o_diff = A.take<int16_t>(want_diff ? samples : 0);
}

int profile_plan::run(dsss_ctx* c, const mosaic_arena& A, const dsss_mosaic_params* p, const unsigned long long* acc,
                      dsss_ping_stat* stats_host, int16_t* diff_host, dsss_profile_info* info)
{
    const int nf = (int)frames.size();
    // the batches: frames in order while their windows fit the arena
    batch_end.clear();
    size_t cur = 0;
    for (int k = 0; k < nf; ++k) {
        const size_t wc = frames[k].on_grid ? (size_t)frames[k].w.bw * frames[k].w.bh : 0;
        if (cur && cur + wc > arena_cells) { batch_end.push_back(k); cur = 0; }
        cur += wc;
    }
    batch_end.push_back(nf);
    unsigned long long* d_win = A.at(o_win); mosaic_job* d_sjobs = A.at(o_sjobs); prof_job* d_pjobs = A.at(o_pjobs);
    dsss_ping_stat* d_stats = A.at(o_stats); int16_t* d_diff = A.opt(o_diff);
    // the two job tables: the scatter's (every frame a table of its own, blk0 = 0) and the profile's (blk0 ascending within a batch)
    std::vector<mosaic_job> sjobs(nf); std::vector<prof_job> pjobs(nf);
    std::vector<int> blocks(batch_end.size(), 0); std::vector<size_t> cells(batch_end.size(), 0);
    size_t ping0 = 0, diff0 = 0;
    for (int b = 0, k = 0; b < (int)batch_end.size(); ++b)
        for (; k < batch_end[b]; ++k) {
            const profile_frame& f = frames[k];
            sjobs[k] = f.job; sjobs[k].blk0 = 0;
            prof_job j; static_cast<mosaic_job&>(j) = f.job;
            j.blk0 = blocks[b]; j.ping0 = ping0; j.diff0 = diff0; j.woff = cells[b];
            if (f.on_grid) { j.ox = f.w.ox; j.oy = f.w.oy; j.bw = f.w.bw; j.bh = f.w.bh; cells[b] += (size_t)f.w.bw * f.w.bh; }
            pjobs[k] = j;
            blocks[b] += f.job.N; ping0 += (size_t)f.job.N; diff0 += (size_t)f.job.N * f.job.M;
        }
    HIPCHK(c, hipMemcpyAsync(d_sjobs, sjobs.data(), (size_t)nf * sizeof(mosaic_job), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_pjobs, pjobs.data(), (size_t)nf * sizeof(prof_job), hipMemcpyHostToDevice, c->stream));
    const mosaic_win G = mosaic_grid_win(p);
    for (int b = 0, k0 = 0; b < (int)batch_end.size(); k0 = batch_end[b], ++b) {
        const int k1 = batch_end[b];
        if (cells[b]) HIPCHK(c, hipMemsetAsync(d_win, 0, cells[b] * 8, c->stream));
        for (int k = k0; k < k1; ++k)
            if (frames[k].on_grid && frames[k].job.N > 0) launch_scatter(c, d_sjobs + k, 1, frames[k].job.N, frames[k].w, d_win + pjobs[k].woff);
        HIPCHK(c, hipGetLastError());
        if (blocks[b] > 0) {
            if (d_diff) hipLaunchKernelGGL(mosaic_profile_kernel<true>, dim3((unsigned)blocks[b]), dim3(256), 0, c->stream, d_pjobs + k0, k1 - k0, G, acc, d_win, (uint32_t)min_count, d_stats, d_diff);
            else hipLaunchKernelGGL(mosaic_profile_kernel<false>, dim3((unsigned)blocks[b]), dim3(256), 0, c->stream, d_pjobs + k0, k1 - k0, G, acc, d_win, (uint32_t)min_count, d_stats, d_diff);
            HIPCHK(c, hipGetLastError());
        }
    }
    // the records come down whenever the caller wants them or the info; the residual layers only when asked for
    std::vector<dsss_ping_stat> own;
    dsss_ping_stat* host = stats_host;
    if (!host && info) { own.resize(std::max<size_t>(pings, 1)); host = own.data(); }
    if (host && pings) HIPCHK(c, hipMemcpyAsync(host, d_stats, pings * sizeof(dsss_ping_stat), hipMemcpyDeviceToHost, c->stream));
    if (diff_host && samples) HIPCHK(c, hipMemcpyAsync(diff_host, d_diff, samples * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (info) dsss_profile_summary(host, (int64_t)pings, info);
    return DSSS_OK;
}

extern "C" {

void dsss_profile_params_default(dsss_profile_params* p) { if (p) { p->min_count = 1; p->pad_ = 0; } }

int dsss_profile_summary(const dsss_ping_stat* stats, int64_t npings, dsss_profile_info* info)
{
    if (!info || npings < 0 || (npings > 0 && !stats)) return DSSS_E_ARG;
    dsss_profile_info I; memset(&I, 0, sizeof I);
    I.pings = npings;
    for (int64_t i = 0; i < npings; ++i)
        for (int s = 0; s < 2; ++s) {
            I.binned += stats[i].binned[s]; I.n += stats[i].n[s]; I.sad += stats[i].sad[s]; I.ssd += stats[i].ssd[s]; I.sd += stats[i].sd[s];
        }
    I.rms = I.n ? sqrt((double)I.ssd / (double)I.n) : 0.0;
    *info = I;
    return DSSS_OK;
}

int dsss_profile_mosaic(dsss_ctx* c, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params* p,
                        const int* prof, int nprof, const dsss_profile_params* pp, dsss_ping_stat* stats_host, int16_t* diff_host, dsss_profile_info* info)
{
    if (!c) return DSSS_E_ARG;
    if (info) memset(info, 0, sizeof *info);
    size_t rows = 0;
    int rc = mosaic_check_args(c, ids, n, rpy6, ping_off, p, &rows); if (rc) return rc;
    if (prof && nprof < 1) DSSS_FAIL(c, DSSS_E_ARG, "profile: %d frames to profile", nprof);
    std::vector<int> which(prof ? nprof : n);
    std::vector<char> seen(n, 0);
    for (size_t k = 0; k < which.size(); ++k) {
        const int i = prof ? prof[k] : (int)k;
        if (i < 0 || i >= n) DSSS_FAIL(c, DSSS_E_ARG, "profile: prof[%zu] = %d outside the %d listed frames", k, i, n);
        if (seen[i]) DSSS_FAIL(c, DSSS_E_ARG, "profile: prof names the listed frame %d twice", i);
        seen[i] = 1; which[k] = i;
    }
    profile_plan plan;
    rc = profile_check_params(c, pp, &plan.min_count); if (rc) return rc;
    for (int i : which) { rc = profile_check_frame(c, ids[i]); if (rc) return rc; }
    HIPCHK(c, hipSetDevice(c->device));
    plan.want_stats = stats_host || info; plan.want_diff = diff_host != nullptr;
    const bool wanted = plan.want_stats || plan.want_diff;                         // nothing asked for: the render's checks alone
    if (wanted) {
        plan.frames.resize(which.size());
        for (size_t k = 0; k < which.size(); ++k) { const dsss_frame& f = c->frames[ids[which[k]]]; plan.frames[k].job.N = f.N; plan.frames[k].job.M = f.M; }      // (what take() reads)
    }
    const size_t cells = (size_t)p->W * p->H;
    mosaic_arena A;
    const auto o_acc = A.take<unsigned long long>(cells);
    const auto o_jobs = A.take<mosaic_job>(n); const auto o_rows = A.take<double>(rpy6 ? rows * 6 : 0); const auto o_flag = A.take<int>(1);
    if (wanted) plan.take(A, cells);
    rc = A.reserve(c); if (rc) return rc;
    unsigned long long* acc = A.at(o_acc); int* d_flag = A.at(o_flag);
    std::vector<mosaic_job> jobs;
    rc = mosaic_fill_jobs(c, ids, n, rpy6, ping_off, A.at(o_rows), jobs); if (rc) return rc;
    for (size_t k = 0; k < plan.frames.size(); ++k) plan.frames[k].job = jobs[which[k]];
    // A = the render's accumulators, by the render's launches and under its sample limit
    rc = mosaic_render_acc(c, jobs, A.at(o_jobs), p, nullptr, acc, d_flag, nullptr, nullptr, nullptr); if (rc) return rc;
    // the windows of the profiled frames, the cells their geo extremes can reach under the rows they are profiled with: host arithmetic,
    // two bearings per ping, BEHIND the render's launches so that it runs while the device scatters
    for (size_t k = 0; k < plan.frames.size(); ++k) {
        const int i = which[k];
        const dsss_frame& f = c->frames[ids[i]];
        plan.frames[k].on_grid = mosaic_window(f, rpy6 ? rpy6 + (size_t)ping_off[i] * 6 : f.h_geo, 0, f.N, p, &plan.frames[k].w);
    }
    rc = mosaic_flag_down(c, d_flag, "profile: a cell received more than 2^24 samples (cell %g too coarse for these frames)", p->cell); if (rc) return rc;
    if (!wanted) return DSSS_OK;
    return plan.run(c, A, p, acc, stats_host, diff_host, info);
}

} // extern "C"

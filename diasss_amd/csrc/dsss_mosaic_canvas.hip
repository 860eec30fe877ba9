// diasss_amd/csrc/dsss_mosaic_canvas.hip -- the mosaic canvas (include/dsss_canvas.h): the accumulators of one grid kept on the device
// between calls, frames added, moved and removed by signed scatters.  The accumulator of a cell is count << 32 | sum, filled by 64-bit
// atomic adds, so what a frame added is taken out again exactly by adding its two's complement, and the canvas always reads what a
// fresh render of its frames reads.  That holds because the canvas kernels run the render kernels' own prologue, sample loops and
// accumulator word (dsss_mosaic_int.h) with the sign of a job; what is written here is the fused move's loop and the window form of the
// unpack.
#include "dsss_mosaic_int.h"
#include "dsss_mosaic_profile.h"
#include "../../include/dsss_canvas.h"
#include <algorithm>
#include <map>

namespace {

// one job of a canvas launch: a mosaic_job whose pose rows lie in the canvas's row store, the sign it is scattered with (uniform per
// workgroup) and, for the fused move, the rows the frame moves to (pose: out, pose2: in)
struct canvas_job : mosaic_job { const double* pose2 = nullptr; int sign = 1, pad_ = 0; };

// the second row of the fused move's prologue (mosaic_ping_of's partner form): the row the ping moves to; no ping is the last
struct canvas_moved_row {
    __device__ __forceinline__ const double* operator()(const canvas_job& J, int row, bool& last) const { last = false; return J.pose2 + (size_t)row * 6; }
};

// The signed form of mosaic_scatter_kernel: its prologue and its body (mosaic_ping_of, mosaic_scatter_samples) with the sign of the
// job, which is uniform per workgroup.  Add jobs and remove jobs share a launch.
__global__ __launch_bounds__(256) void mosaic_canvas_kernel(const canvas_job* __restrict__ jobs, int njobs, mosaic_win G, unsigned long long* __restrict__ acc)
{
    __shared__ double s_sc[4];
    canvas_job J; int row; const double* P;
    if (!mosaic_ping_of(jobs, njobs, s_sc, J, row, P)) return;
    mosaic_scatter_samples<true>(P, s_sc, J, row, G, acc, J.sign < 0);
}

// The signed form of mosaic_scatter_fp_kernel: the prologue in the partner form, then the sub-samples by the one body
// (mosaic_scatter_footprints) with the sign of the job.
__global__ __launch_bounds__(256) void mosaic_canvas_fp_kernel(const canvas_job* __restrict__ jobs, int njobs, mosaic_win G, dsss_footprint_params F,
                                                               unsigned long long* __restrict__ acc)
{
    __shared__ double s_sc[8];
    canvas_job J; int row; const double* P; const double* PP; bool last;
    if (!mosaic_ping_of(jobs, njobs, s_sc, J, row, P, &PP, &last)) return;
    mosaic_scatter_footprints<true>(P, PP, last, s_sc, J, row, G, F, acc, J.sign < 0);
}

// The fused move of a point canvas: one workgroup per ping of a moved frame, the bearings of the old row (J.pose) and of the new one
// (J.pose2) in LDS as 8 doubles (the prologue's partner form with canvas_moved_row).  A lane bins its sample under both rows; the value
// is the same under both, because the mask, the gain column and the altitude band do not depend on the pose.  A sample whose cell is
// the same under both rows issues nothing -- the scatter runs at the rate of its atomics, and a centimetre-level correction leaves most
// samples where they were.  The others go through two run reductions (mosaic_run_add): the old keys are subtracted, the new keys are
// added.  A row that is not finite has key -1 on its side.  Two keys per sample and the skip are why this loop is its own.
__global__ __launch_bounds__(256) void mosaic_canvas_move_kernel(const canvas_job* __restrict__ jobs, int njobs, mosaic_win G, unsigned long long* __restrict__ acc)
{
    __shared__ double s_sc[8];
    canvas_job J; int row; const double* P0; const double* P1; bool last;      // (last: the partner form's, false for every ping here)
    if (!mosaic_ping_of(jobs, njobs, s_sc, J, row, P0, &P1, &last, canvas_moved_row())) return;
    const int M = J.M;
    const uint8_t* __restrict__ img = J.img + (size_t)row * M;
    const uint8_t* __restrict__ mask = J.mask + (size_t)row * M;
    for (int c0 = 0; c0 < M; c0 += 256) {
        const int col = c0 + (int)threadIdx.x;
        unsigned g0 = 0, g1 = 0;
        int k0 = mosaic_sample_cell(P0, s_sc, J, img, mask, col, G, &g0);
        int k1 = mosaic_sample_cell(P1, s_sc + 4, J, img, mask, col, G, &g1);
        const unsigned g = k0 >= 0 ? g0 : g1;
        if (k0 == k1) { k0 = -1; k1 = -1; }                                        // the sample stays in its cell (or is dropped under both rows)
        if (__ballot(k0 != k1) == 0ull) continue;                                  // no lane of the wavefront moved (uniform over the wavefront)
        const unsigned v0 = k0 >= 0 ? (1u << 16) | g : 0u, v1 = k1 >= 0 ? (1u << 16) | g : 0u;
        mosaic_run_add<true>(acc, k0, v0, true);
        mosaic_run_add<true>(acc, k1, v1, false);
    }
}

// The window form of mosaic_unpack_kernel: the layers of the window (ox, oy, bw, bh) of a grid W cells wide, packed bw x bh, and the
// sample-limit flag (also run with no outputs, as the check alone)
__global__ __launch_bounds__(256) void mosaic_canvas_unpack_kernel(const unsigned long long* __restrict__ acc, int W, int ox, int oy, int bw, int bh,
                                                                   uint32_t* __restrict__ sum, uint32_t* __restrict__ cnt, uint8_t* __restrict__ img, int* __restrict__ flag)
{
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= (size_t)bw * bh) return;
    const int jy = (int)(j / (size_t)bw), jx = (int)(j - (size_t)jy * bw);
    const mosaic_acc a(acc[(size_t)(oy + jy) * W + (ox + jx)]);
    if (a.over_limit()) *flag = 1;
    if (sum) sum[j] = a.s;
    if (cnt) cnt[j] = a.c;
    if (img) img[j] = a.c ? (uint8_t)a.mean() : (uint8_t)0;
}

// ---- the row store: the device copies of the frames' rows, the canvas's own memory (mosaic_buf is scratch that other mosaic entries
// reuse between canvas calls).  Chunks of device memory handed out in 256-byte aligned blocks; a block given back is handed out again to
// a request of its size (the frames of a survey have one N); clear starts over and keeps the chunks.
struct canvas_row_store {
    std::vector<dsss_buf> chunks; size_t cur = 0, off = 0;                         // off: bytes used of chunks[cur]
    std::vector<std::pair<double*, size_t>> free_blocks;
    static constexpr size_t CHUNK = (size_t)8 << 20;
    int take(dsss_ctx* c, size_t doubles, double** out)
    {
        for (size_t k = 0; k < free_blocks.size(); ++k)
            if (free_blocks[k].second == doubles) { *out = free_blocks[k].first; free_blocks[k] = free_blocks.back(); free_blocks.pop_back(); return DSSS_OK; }
        const size_t bytes = (doubles * sizeof(double) + 255) & ~(size_t)255;
        while (cur < chunks.size() && off + bytes > chunks[cur].cap) { ++cur; off = 0; }
        if (cur == chunks.size()) {
            chunks.emplace_back("canvas_rows");
            const int rc = chunks.back().reserve(c, std::max(bytes, CHUNK));
            if (rc) { chunks.pop_back(); return rc; }
            off = 0;
        }
        *out = reinterpret_cast<double*>(chunks[cur].as<char>() + off); off += bytes;
        return DSSS_OK;
    }
    void give(double* p, size_t doubles) { free_blocks.emplace_back(p, doubles); }
    void reset() { cur = 0; off = 0; free_blocks.clear(); }
};

// a frame of S: the epoch of the frame it was put at, its rows on the host and on the device and their window of the grid (a move and
// a remove need it again: two bearings per ping on the host are not free).  The device block holds two slots of N x 6 doubles; slot
// `cur` holds the stored rows, a move uploads into the other one and flips cur once the call has succeeded.
struct canvas_entry {
    unsigned long long epoch = 0; int N = 0, cur = 0;
    int32_t win[4] = { 0, 0, 0, 0 };
    std::vector<double> h_rows; double* d_rows = nullptr;
    size_t doubles() const { return (size_t)N * 12; }
    double* slot(int k) const { return d_rows + (size_t)k * N * 6; }
};

// one launch of a call: jobs [j0, j1) of the scatter table or of the fused-move table
struct canvas_launch { bool fused; int j0, j1, blocks; };

void win_none(int32_t* w) { w[0] = 0; w[1] = 0; w[2] = 0; w[3] = 0; }
void win_union(int32_t* w, const int32_t* a)
{
    if (a[2] <= 0) return;
    if (w[2] <= 0) { memcpy(w, a, 4 * sizeof(int32_t)); return; }
    const int x0 = std::min(w[0], a[0]), y0 = std::min(w[1], a[1]), x1 = std::max(w[0] + w[2], a[0] + a[2]), y1 = std::max(w[1] + w[3], a[1] + a[3]);
    w[0] = x0; w[1] = y0; w[2] = x1 - x0; w[3] = y1 - y0;
}

} // namespace

struct dsss_canvas {
    dsss_ctx* c = nullptr;
    dsss_mosaic_params grid{}; dsss_canvas_params par{};
    dsss_buf acc{"canvas_acc"};                                                    // W x H accumulators, the canvas's own
    canvas_row_store rows;
    std::map<int, canvas_entry> S;                                                 // ascending ids
    unsigned long long gain_epoch = 0;                                             // the context's when the first frame of S was put
    int32_t dirty[4] = { 0, 0, 0, 0 };
    bool broken = false;                                                           // a HIP error inside a call: only clear and destroy go on
    bool fused() const { return !par.footprint && par.move == DSSS_CANVAS_MOVE_AUTO; }
    size_t cells() const { return (size_t)grid.W * grid.H; }
};

namespace {

// the one refusal of a broken canvas: every entry but clear and destroy starts with it
int canvas_refuse_broken(const dsss_canvas* cv)
{
    if (cv->broken) DSSS_FAIL(cv->c, DSSS_E_STATE, "canvas: broken by an earlier HIP error (dsss_canvas_clear starts over)");
    return DSSS_OK;
}

// the window of a frame under `rows` on the canvas's grid (include/dsss_canvas.h, "Windows"); none: bw = 0
void canvas_window(const dsss_canvas* cv, const dsss_frame& f, const double* rows, int32_t* w)
{
    win_none(w);
    const double grow = cv->par.footprint ? 2.0 * cv->par.fp.max_gap : 0.0;        // a sub-sample lies within (7/8) 2 max_gap per axis of its parent
    mosaic_win mw;
    if (mosaic_window(f, rows, 0, f.N, &cv->grid, &mw, grow)) { w[0] = mw.ox; w[1] = mw.oy; w[2] = mw.bw; w[3] = mw.bh; }
}

void canvas_launch_jobs(dsss_canvas* cv, const canvas_launch& L, const canvas_job* d_jobs, const canvas_job* d_moves)
{
    dsss_ctx* c = cv->c;
    const mosaic_win G = mosaic_grid_win(&cv->grid);
    unsigned long long* acc = cv->acc.as<unsigned long long>();
    const int nj = L.j1 - L.j0;
    if (L.fused) hipLaunchKernelGGL(mosaic_canvas_move_kernel, dim3((unsigned)L.blocks), dim3(256), 0, c->stream, d_moves + L.j0, nj, G, acc);
    else if (cv->par.footprint) hipLaunchKernelGGL(mosaic_canvas_fp_kernel, dim3((unsigned)L.blocks), dim3(256), 0, c->stream, d_jobs + L.j0, nj, G, cv->par.fp, acc);
    else hipLaunchKernelGGL(mosaic_canvas_kernel, dim3((unsigned)L.blocks), dim3(256), 0, c->stream, d_jobs + L.j0, nj, G, acc);
}

// the launches of a table, the render's cut (mosaic_cut_launches); blk0 of every job is set
void canvas_plan(dsss_canvas* cv, std::vector<canvas_job>& tab, bool fused, std::vector<canvas_launch>& out)
{
    for (const mosaic_launch& L : mosaic_cut_launches(tab, cv->par.footprint ? &cv->par.fp : nullptr)) out.push_back({ fused, L.j0, L.j1, L.blocks });
}

// the same jobs with the signs flipped: a scatter job changes its sign, a fused move swaps the rows it moves between
canvas_job canvas_flip(canvas_job j, bool fused)
{
    if (fused) std::swap(j.pose, j.pose2); else j.sign = -j.sign;
    return j;
}

// The launches of one call: jobs = the signed scatter jobs, moves = the fused moves.  window(win) fills the call's window of the grid;
// it is asked for once, BEHIND the first launch, so the host arithmetic of the windows (two bearings per ping, 32 us for a frame of 2000
// pings: as long as the kernel takes for it) runs while the device scatters.  The sample limit is checked over the window between the
// launches and at the end; on DSSS_E_CAPACITY the launches issued so far are undone by the same jobs with the signs flipped, so the
// accumulators are those from before the call.  Returns with the stream synchronised.
template <class WINDOW>
int canvas_run(dsss_canvas* cv, std::vector<canvas_job>& jobs, std::vector<canvas_job>& moves, WINDOW window, int32_t* win, int64_t* pings)
{
    dsss_ctx* c = cv->c;
    std::vector<canvas_launch> L;
    canvas_plan(cv, jobs, false, L); canvas_plan(cv, moves, true, L);
    if (pings) *pings = 0;
    if (L.empty()) return DSSS_OK;
    mosaic_arena A;
    const auto o_jobs = A.take<canvas_job>(jobs.size()), o_moves = A.take<canvas_job>(moves.size());
    const auto o_ujobs = A.take<canvas_job>(jobs.size()), o_umoves = A.take<canvas_job>(moves.size());
    const auto o_flag = A.take<int>(1);
    int rc = A.reserve(c); if (rc) return rc;
    canvas_job* d_jobs = A.at(o_jobs); canvas_job* d_moves = A.at(o_moves); int* d_flag = A.at(o_flag);
    if (!jobs.empty()) HIPCHK(c, hipMemcpyAsync(d_jobs, jobs.data(), jobs.size() * sizeof(canvas_job), hipMemcpyHostToDevice, c->stream));
    if (!moves.empty()) HIPCHK(c, hipMemcpyAsync(d_moves, moves.data(), moves.size() * sizeof(canvas_job), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d_flag, 0, sizeof(int), c->stream));
    size_t wcells = 0; unsigned ublocks = 0;
    const unsigned long long* acc = cv->acc.as<unsigned long long>();
    for (size_t k = 0; k < L.size(); ++k) {
        canvas_launch_jobs(cv, L[k], d_jobs, d_moves);
        HIPCHK(c, hipGetLastError());
        if (pings) *pings += L[k].blocks;
        if (k == 0) { window(win); wcells = win[2] > 0 ? (size_t)win[2] * win[3] : 0; ublocks = (unsigned)((wcells + 255) / 256); }
        rc = DSSS_OK;
        if (wcells) {
            hipLaunchKernelGGL(mosaic_canvas_unpack_kernel, dim3(ublocks), dim3(256), 0, c->stream, acc, cv->grid.W, win[0], win[1], win[2], win[3],
                               (uint32_t*)nullptr, (uint32_t*)nullptr, (uint8_t*)nullptr, d_flag);
            HIPCHK(c, hipGetLastError());
            rc = mosaic_flag_down(c, d_flag, "canvas: a cell would hold more than 2^24 samples (cell %g too coarse for these frames); the call is undone", cv->grid.cell);
        } else if (k + 1 == L.size()) HIPCHK(c, hipStreamSynchronize(c->stream));
        if (rc == DSSS_E_CAPACITY) {
            const std::string msg = c->err;
            std::vector<canvas_job> uj(jobs.size()), um(moves.size());
            for (size_t i = 0; i < jobs.size(); ++i) uj[i] = canvas_flip(jobs[i], false);
            for (size_t i = 0; i < moves.size(); ++i) um[i] = canvas_flip(moves[i], true);
            canvas_job* d_uj = A.at(o_ujobs); canvas_job* d_um = A.at(o_umoves);
            if (!uj.empty()) HIPCHK(c, hipMemcpyAsync(d_uj, uj.data(), uj.size() * sizeof(canvas_job), hipMemcpyHostToDevice, c->stream));
            if (!um.empty()) HIPCHK(c, hipMemcpyAsync(d_um, um.data(), um.size() * sizeof(canvas_job), hipMemcpyHostToDevice, c->stream));
            for (size_t u = 0; u <= k; ++u) { canvas_launch_jobs(cv, L[u], d_uj, d_um); HIPCHK(c, hipGetLastError()); }
            HIPCHK(c, hipStreamSynchronize(c->stream));
            c->err = msg;
            return DSSS_E_CAPACITY;
        }
        if (rc) return rc;
    }
    return DSSS_OK;
}

// a job of frame `id` with the rows `pose` (device), the ONE place the frame's part of it is filled: mosaic_fill_jobs
int canvas_job_of(dsss_ctx* c, int id, const double* pose, const double* pose2, int sign, canvas_job* out)
{
    std::vector<mosaic_job> one;
    const int rc = mosaic_fill_jobs(c, &id, 1, nullptr, nullptr, nullptr, one); if (rc) return rc;
    canvas_job j; static_cast<mosaic_job&>(j) = one[0];
    j.pose = pose; j.pose2 = pose2; j.sign = sign; j.pad_ = 0;
    *out = j;
    return DSSS_OK;
}

// the checks every put and remove starts with, in the order the header gives
int canvas_check(dsss_canvas* cv, const int* ids, int n, const double* rpy6, const int* ping_off, bool must_be_in)
{
    dsss_ctx* c = cv->c;
    int rc = canvas_refuse_broken(cv); if (rc) return rc;
    size_t rows = 0;
    rc = mosaic_check_frames(c, ids, n, rpy6, ping_off, true, &rows); if (rc) return rc;
    if (cv->par.footprint) { dsss_footprint_params F; rc = mosaic_check_footprint(c, ids, n, &cv->par.fp, &F); if (rc) return rc; }
    rc = mosaic_check_gain(c, ids, n); if (rc) return rc;
    if (must_be_in)
        for (int i = 0; i < n; ++i)
            if (!cv->S.count(ids[i])) DSSS_FAIL(c, DSSS_E_ARG, "canvas: frame %d is not on the canvas", ids[i]);
    if (!cv->S.empty() && cv->gain_epoch != c->gain_epoch)
        DSSS_FAIL(c, DSSS_E_STATE, "canvas: the range-gain table changed since the frames were put (dsss_canvas_clear starts over)");
    for (int i = 0; i < n; ++i) {
        const auto it = cv->S.find(ids[i]);
        if (it != cv->S.end() && it->second.epoch != c->frames[ids[i]].epoch)
            DSSS_FAIL(c, DSSS_E_STATE, "canvas: frame %d was set or extracted again since it was put (dsss_canvas_clear starts over)", ids[i]);
    }
    return DSSS_OK;
}

int canvas_fail(dsss_canvas* cv, int rc) { if (rc == DSSS_E_HIP) cv->broken = true; return rc; }

void canvas_free(dsss_canvas* cv)
{
    dsss_ctx* c = cv->c;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    c->canvases.erase(std::remove(c->canvases.begin(), c->canvases.end(), cv), c->canvases.end());
    delete cv;
}

int canvas_put(dsss_canvas* cv, const int* ids, int n, const double* rpy6, const int* ping_off, dsss_canvas_put_info* info)
{
    dsss_ctx* c = cv->c;
    int rc = canvas_check(cv, ids, n, rpy6, ping_off, false); if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    // what becomes of every listed frame: 0 added, 1 moved, 2 skipped
    std::vector<int> what(n); std::vector<const double*> src(n); std::vector<double*> fresh(n, nullptr);
    std::vector<std::array<int32_t, 4>> wins(n);                                   // the windows of the new rows
    dsss_canvas_put_info I; memset(&I, 0, sizeof I);
    for (int i = 0; i < n; ++i) {
        const dsss_frame& f = c->frames[ids[i]];
        src[i] = rpy6 ? rpy6 + (size_t)ping_off[i] * 6 : f.h_geo;
        const auto it = cv->S.find(ids[i]);
        if (it == cv->S.end()) { what[i] = 0; ++I.added; }
        else if (memcmp(it->second.h_rows.data(), src[i], (size_t)f.N * 6 * sizeof(double)) == 0) { what[i] = 2; ++I.skipped; }
        else { what[i] = 1; ++I.moved; }
    }
    // the device blocks of the added frames; a failure gives back what was taken
    auto give_back = [&] { for (int i = 0; i < n; ++i) if (fresh[i]) cv->rows.give(fresh[i], (size_t)c->frames[ids[i]].N * 12); };
    for (int i = 0; i < n; ++i) {
        if (what[i] != 0) continue;
        rc = cv->rows.take(c, (size_t)c->frames[ids[i]].N * 12, &fresh[i]);
        if (rc) { give_back(); return rc; }
    }
    std::vector<canvas_job> jobs, moves;
    auto run = [&]() -> int {
        for (int i = 0; i < n; ++i) {
            if (what[i] == 2) continue;
            const dsss_frame& f = c->frames[ids[i]];
            const size_t bytes = (size_t)f.N * 6 * sizeof(double);
            canvas_job j;
            if (what[i] == 0) {
                HIPCHK(c, hipMemcpyAsync(fresh[i], src[i], bytes, hipMemcpyHostToDevice, c->stream));
                int r = canvas_job_of(c, ids[i], fresh[i], nullptr, +1, &j); if (r) return r;
                jobs.push_back(j);
                continue;
            }
            const canvas_entry& e = cv->S.find(ids[i])->second;
            const double* d_old = e.slot(e.cur); double* d_new = e.slot(1 - e.cur);
            HIPCHK(c, hipMemcpyAsync(d_new, src[i], bytes, hipMemcpyHostToDevice, c->stream));
            if (cv->fused()) { int r = canvas_job_of(c, ids[i], d_old, d_new, +1, &j); if (r) return r; moves.push_back(j); }
            else {
                int r = canvas_job_of(c, ids[i], d_old, nullptr, -1, &j); if (r) return r; jobs.push_back(j);
                r = canvas_job_of(c, ids[i], d_new, nullptr, +1, &j); if (r) return r; jobs.push_back(j);
            }
        }
        // the call's window: the new rows' windows, and the stored ones of the frames that move
        const int r = canvas_run(cv, jobs, moves, [&](int32_t* w) {
            for (int i = 0; i < n; ++i) {
                if (what[i] == 2) continue;
                canvas_window(cv, c->frames[ids[i]], src[i], wins[i].data()); win_union(w, wins[i].data());
                if (what[i] == 1) win_union(w, cv->S.find(ids[i])->second.win);
            }
        }, I.win, &I.pings);
        if (r) return r;
        return hipStreamSynchronize(c->stream) == hipSuccess ? DSSS_OK : DSSS_E_HIP;  // (the uploads of a call that launched nothing)
    };
    rc = run();
    if (rc) { give_back(); if (info) memset(info, 0, sizeof *info); return canvas_fail(cv, rc); }
    // the call succeeded: S and the stored rows follow
    if (cv->S.empty()) cv->gain_epoch = c->gain_epoch;
    for (int i = 0; i < n; ++i) {
        if (what[i] == 2) continue;
        const dsss_frame& f = c->frames[ids[i]];
        canvas_entry& e = cv->S[ids[i]];
        if (what[i] == 0) { e.epoch = f.epoch; e.N = f.N; e.cur = 0; e.d_rows = fresh[i]; }
        else e.cur = 1 - e.cur;
        e.h_rows.assign(src[i], src[i] + (size_t)f.N * 6);
        memcpy(e.win, wins[i].data(), sizeof e.win);
    }
    win_union(cv->dirty, I.win);
    if (info) *info = I;
    return DSSS_OK;
}

int canvas_remove(dsss_canvas* cv, const int* ids, int n)
{
    dsss_ctx* c = cv->c;
    int rc = canvas_check(cv, ids, n, nullptr, nullptr, true); if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<canvas_job> jobs, moves;
    int32_t win[4]; win_none(win);
    for (int i = 0; i < n; ++i) {
        const canvas_entry& e = cv->S.find(ids[i])->second;
        canvas_job j;
        rc = canvas_job_of(c, ids[i], e.slot(e.cur), nullptr, -1, &j); if (rc) return rc;
        jobs.push_back(j);
    }
    rc = canvas_run(cv, jobs, moves, [&](int32_t* w) { for (int i = 0; i < n; ++i) win_union(w, cv->S.find(ids[i])->second.win); }, win, nullptr);
    if (rc) return canvas_fail(cv, rc);
    for (int i = 0; i < n; ++i) {
        const auto it = cv->S.find(ids[i]);
        cv->rows.give(it->second.d_rows, it->second.doubles());
        cv->S.erase(it);
    }
    win_union(cv->dirty, win);
    return DSSS_OK;
}

} // namespace

void dsss_canvas_free_all(dsss_ctx* c)
{
    while (!c->canvases.empty()) canvas_free(c->canvases.back());
}

extern "C" {

void dsss_canvas_params_default(dsss_canvas_params* p)
{
    if (!p) return;
    p->footprint = 0; p->move = DSSS_CANVAS_MOVE_AUTO;
    dsss_footprint_params_default(&p->fp);
}

int dsss_canvas_create(dsss_ctx* c, const dsss_mosaic_params* grid, const dsss_canvas_params* params, dsss_canvas** out)
{
    if (!c) return DSSS_E_ARG;
    if (!out) DSSS_FAIL(c, DSSS_E_ARG, "canvas: nowhere to write the canvas");
    *out = nullptr;
    int rc = mosaic_check_params(c, grid); if (rc) return rc;
    dsss_canvas_params P;
    dsss_canvas_params_default(&P);
    if (params) P = *params;
    P.fp.pad_ = 0; P.footprint = P.footprint != 0;
    if (P.move != DSSS_CANVAS_MOVE_AUTO && P.move != DSSS_CANVAS_MOVE_SPLIT) DSSS_FAIL(c, DSSS_E_ARG, "canvas: move mode %d", P.move);
    if (P.footprint && !footprint_params_ok(P.fp)) DSSS_FAIL(c, DSSS_E_ARG, "canvas: footprint max_steps %d, max_gap %g (1..%d; finite and > 0)", P.fp.max_steps, P.fp.max_gap, FP_MAX_STEPS);
    HIPCHK(c, hipSetDevice(c->device));
    dsss_canvas* cv = new dsss_canvas();
    cv->c = c; cv->grid = *grid; cv->grid.pad_ = 0; cv->par = P; cv->gain_epoch = c->gain_epoch;
    rc = cv->acc.reserve(c, cv->cells() * 8);
    if (rc) { delete cv; return rc; }
    hipError_t e = hipMemsetAsync(cv->acc.p, 0, cv->cells() * 8, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { delete cv; return dsss_hip_fail(c, e, __FILE__, __LINE__, "clearing the accumulators of a canvas"); }
    c->canvases.push_back(cv);
    *out = cv;
    return DSSS_OK;
}

int dsss_canvas_destroy(dsss_canvas* cv)
{
    if (!cv) return DSSS_E_ARG;
    canvas_free(cv);
    return DSSS_OK;
}

int dsss_canvas_put(dsss_canvas* cv, const int* ids, int n, const double* rpy6, const int* ping_off, dsss_canvas_put_info* info)
{
    if (!cv) return DSSS_E_ARG;
    if (info) memset(info, 0, sizeof *info);
    return canvas_put(cv, ids, n, rpy6, ping_off, info);
}

int dsss_canvas_remove(dsss_canvas* cv, const int* ids, int n)
{
    if (!cv) return DSSS_E_ARG;
    return canvas_remove(cv, ids, n);
}

int dsss_canvas_clear(dsss_canvas* cv)
{
    if (!cv) return DSSS_E_ARG;
    dsss_ctx* c = cv->c;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemsetAsync(cv->acc.p, 0, cv->cells() * 8, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    cv->S.clear(); cv->rows.reset(); cv->broken = false; cv->gain_epoch = c->gain_epoch;
    cv->dirty[0] = 0; cv->dirty[1] = 0; cv->dirty[2] = cv->grid.W; cv->dirty[3] = cv->grid.H;
    return DSSS_OK;
}

int dsss_canvas_read(dsss_canvas* cv, const int32_t* win4, uint32_t* sum, uint32_t* cnt, uint8_t* img)
{
    if (!cv) return DSSS_E_ARG;
    dsss_ctx* c = cv->c;
    int rc = canvas_refuse_broken(cv); if (rc) return rc;
    int32_t w[4] = { 0, 0, cv->grid.W, cv->grid.H };
    if (win4) memcpy(w, win4, sizeof w);
    if (w[0] < 0 || w[1] < 0 || w[2] < 1 || w[3] < 1 || (long long)w[0] + w[2] > cv->grid.W || (long long)w[1] + w[3] > cv->grid.H)
        DSSS_FAIL(c, DSSS_E_ARG, "canvas: the window %d, %d, %d x %d leaves the grid %d x %d", w[0], w[1], w[2], w[3], cv->grid.W, cv->grid.H);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t cells = (size_t)w[2] * w[3];
    mosaic_arena A;
    const mosaic_layers L(A, cells, sum, cnt, img); const auto o_flag = A.take<int>(1);
    rc = A.reserve(c); if (rc) return rc;
    if (L.any()) {
        hipLaunchKernelGGL(mosaic_canvas_unpack_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, c->stream, cv->acc.as<unsigned long long>(), cv->grid.W,
                           w[0], w[1], w[2], w[3], A.opt(L.o_sum), A.opt(L.o_cnt), A.opt(L.o_img), A.at(o_flag));
        HIPCHK(c, hipGetLastError());
        rc = L.down(c, A); if (rc) return rc;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DSSS_OK;
}

int dsss_canvas_dirty(dsss_canvas* cv, int32_t* win4, int reset)
{
    if (!cv) return DSSS_E_ARG;
    const int rc = canvas_refuse_broken(cv); if (rc) return rc;
    if (!win4) DSSS_FAIL(cv->c, DSSS_E_ARG, "canvas: nowhere to write the dirty window");
    memcpy(win4, cv->dirty, sizeof cv->dirty);
    if (reset) win_none(cv->dirty);
    return DSSS_OK;
}

int dsss_canvas_frames(const dsss_canvas* cv, int* ids_host, int cap, int* n)
{
    if (!cv) return DSSS_E_ARG;
    dsss_ctx* c = cv->c;
    const int rc = canvas_refuse_broken(cv); if (rc) return rc;
    if (!n) DSSS_FAIL(c, DSSS_E_ARG, "canvas: nowhere to write the number of frames");
    *n = (int)cv->S.size();                                                        // also when there is no room for them: the caller learns how many
    if (cv->S.empty()) return DSSS_OK;
    if (!ids_host || cap < *n) DSSS_FAIL(c, DSSS_E_CAPACITY, "canvas: %d frames, room for %d ids", *n, ids_host ? cap : 0);
    int k = 0;
    for (const auto& kv : cv->S) ids_host[k++] = kv.first;
    return DSSS_OK;
}

int dsss_canvas_rows(dsss_canvas* cv, int id, double* rows_host)
{
    if (!cv) return DSSS_E_ARG;
    dsss_ctx* c = cv->c;
    const int rc = canvas_refuse_broken(cv); if (rc) return rc;
    if (!rows_host) DSSS_FAIL(c, DSSS_E_ARG, "canvas: nowhere to write the rows");
    const auto it = cv->S.find(id);
    if (it == cv->S.end()) DSSS_FAIL(c, DSSS_E_ARG, "canvas: frame %d is not on the canvas", id);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(rows_host, it->second.slot(it->second.cur), (size_t)it->second.N * 6 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DSSS_OK;
}

int dsss_canvas_frame_window(dsss_canvas* cv, int id, const double* rows, int32_t* win4)
{
    if (!cv) return DSSS_E_ARG;
    dsss_ctx* c = cv->c;
    const int rc = canvas_refuse_broken(cv); if (rc) return rc;
    if (!win4) DSSS_FAIL(c, DSSS_E_ARG, "canvas: nowhere to write the window");
    if (id < 0 || id >= c->max_frames) DSSS_FAIL(c, DSSS_E_ARG, "frame id %d out of range [0,%d)", id, c->max_frames);
    const dsss_frame& f = c->frames[id];
    if (!rows) {
        const auto it = cv->S.find(id);
        if (it == cv->S.end()) DSSS_FAIL(c, DSSS_E_ARG, "canvas: frame %d is not on the canvas and no rows are given", id);
        if (it->second.epoch != f.epoch) DSSS_FAIL(c, DSSS_E_STATE, "canvas: frame %d was set or extracted again since it was put", id);
        memcpy(win4, it->second.win, sizeof it->second.win);
        return DSSS_OK;
    }
    if (!f.has_geom || !f.h_geo) DSSS_FAIL(c, DSSS_E_STATE, "frame %d has no geometry", id);
    canvas_window(cv, f, rows, win4);
    return DSSS_OK;
}

// The per-ping profile of frames of S against the canvas (include/dsss_profile.h), beside struct dsss_canvas because it reads the
// accumulators and the row store: the canvas's accumulators are A, every listed frame is profiled under the device copy of its stored
// rows with its stored window, and the launches are those of dsss_profile_mosaic (profile_plan).  Nothing of the canvas is written.
int dsss_profile_canvas(dsss_canvas* cv, const int* ids, int n, const dsss_profile_params* pp, dsss_ping_stat* stats_host, int16_t* diff_host,
                        dsss_profile_info* info)
{
    if (!cv) return DSSS_E_ARG;
    dsss_ctx* c = cv->c;
    if (info) memset(info, 0, sizeof *info);
    int rc = canvas_refuse_broken(cv); if (rc) return rc;
    if (cv->par.footprint) DSSS_FAIL(c, DSSS_E_ARG, "profile: a footprint canvas cannot be profiled");
    rc = canvas_check(cv, ids, n, nullptr, nullptr, true); if (rc) return rc;
    profile_plan plan;
    rc = profile_check_params(c, pp, &plan.min_count); if (rc) return rc;
    for (int i = 0; i < n; ++i) { rc = profile_check_frame(c, ids[i]); if (rc) return rc; }
    plan.want_stats = stats_host || info; plan.want_diff = diff_host != nullptr;
    if (!plan.want_stats && !plan.want_diff) return DSSS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    plan.frames.resize(n);
    for (int i = 0; i < n; ++i) {
        const canvas_entry& e = cv->S.find(ids[i])->second;
        canvas_job j;
        rc = canvas_job_of(c, ids[i], e.slot(e.cur), nullptr, +1, &j); if (rc) return rc;
        profile_frame& f = plan.frames[i];
        f.job = j; f.w = mosaic_grid_win(&cv->grid); f.on_grid = e.win[2] > 0;
        if (f.on_grid) { f.w.ox = e.win[0]; f.w.oy = e.win[1]; f.w.bw = e.win[2]; f.w.bh = e.win[3]; }
    }
    mosaic_arena A;
    plan.take(A, cv->cells());
    rc = A.reserve(c); if (rc) return rc;
    return canvas_fail(cv, plan.run(c, A, &cv->grid, cv->acc.as<unsigned long long>(), stats_host, diff_host, info));
}

} // extern "C"

// diasss_amd/csrc/dsss_internal.h -- shared state of libdsss.so (MI355X / gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <cmath>
#include <cassert>
#include <array>
#include <string>
#include <utility>
#include <vector>
#include "../../include/dsss.h"

#define DSSS_MAX_LEVELS 8
#define DSSS_PI_REF 3.14159265359   // the reference's PI macro (frame.cpp:16, FEAmatcher.cpp:11, optimizer.cpp:19)

struct dsss_ctx;
int dsss_hip_fail(dsss_ctx* c, hipError_t e, const char* file, int line, const char* call);      // what HIPCHK does on a failure: fills c->err, returns DSSS_E_HIP
int dsss_alloc_fail(dsss_ctx* c, hipError_t e, const char* name, const char* step, size_t bytes);   // the same for a failed growth: names the buffer, the step and the size

// ---- ownership of the memory a context keeps between calls: ONE rule, written here once.
// Growing a buffer: synchronise the context's stream (a queued kernel or copy may still use the old block; nothing can use a block that
// does not exist, so a first allocation does not synchronise), free, null the pointer and zero the capacity, allocate, and publish the
// capacity only after the allocation succeeded.  A failed allocation leaves a null pointer and capacity 0 -- never what hipMalloc left in
// its output -- so the next call starts over and destruction is safe.
inline hipError_t dsss_mem_alloc(void** p, size_t bytes, bool pinned) { return pinned ? hipHostMalloc(p, bytes, hipHostMallocDefault) : hipMalloc(p, bytes); }
inline void dsss_mem_free(void* p, bool pinned) { if (p) { if (pinned) (void)hipHostFree(p); else (void)hipFree(p); } }

// one buffer: pointer, capacity in bytes; its name (for dsss_last_error) and its kind, device or page-locked, are fixed where it is declared.
// Move-only -- an assignment moves the block between two buffers of ONE kind and leaves name and kind alone; the destructor frees.
// How much slack to allocate stays with the caller: reserve() takes the bytes needed and the bytes to allocate when those do not suffice.
struct dsss_buf {
    void* p = nullptr; size_t cap = 0; const char* const name; const bool pinned;
    explicit dsss_buf(const char* name_, bool pinned_ = false) : name(name_), pinned(pinned_) {}
    dsss_buf(dsss_buf&& o) noexcept : p(o.p), cap(o.cap), name(o.name), pinned(o.pinned) { o.p = nullptr; o.cap = 0; }
    dsss_buf& operator=(dsss_buf&& o) noexcept { assert(pinned == o.pinned); if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
    dsss_buf(const dsss_buf&) = delete; dsss_buf& operator=(const dsss_buf&) = delete;
    ~dsss_buf() { release(); }
    void release() { dsss_mem_free(p, pinned); p = nullptr; cap = 0; }
    template <class T> T* as() const { return static_cast<T*>(p); }
    explicit operator bool() const { return p != nullptr; }
    int reserve(dsss_ctx* c, size_t need_bytes, size_t alloc_bytes);
    int reserve(dsss_ctx* c, size_t bytes) { return reserve(c, bytes, bytes); }
    int reserve_keep(dsss_ctx* c, size_t need_bytes, size_t alloc_bytes, size_t keep_bytes);      // ... and carries the first keep_bytes over (device memory)
};
constexpr bool DSSS_PINNED = true;

// a family: several typed pointers that live and die under ONE capacity (the feature store, the matcher's result sets, a frame's
// d_pack / h_pack).  The members stay named, typed pointers, because kernels and getters read them by name; the owner lists them as slots.
struct dsss_fam_slot { void** pp; size_t bytes; bool pinned; };
// (the member's address as void**, the form hipMalloc itself takes: every T* here has the representation of void*, and the member is only
// ever written through this view with a pointer the runtime returned, or null)
template <class T> inline dsss_fam_slot dsss_slot(T*& p, size_t bytes = 0, bool pinned = false) { return { reinterpret_cast<void**>(&p), bytes, pinned }; }
template <class Fam> inline void dsss_family_release(size_t& cap, const Fam& fam) { cap = 0; for (const dsss_fam_slot& s : fam) { dsss_mem_free(*s.pp, s.pinned); *s.pp = nullptr; } }
template <class Fam> int dsss_family_alloc(dsss_ctx* c, const char* name, size_t& cap, size_t new_cap, const Fam& fam);      // the rule above for every member; on ANY failure all are freed and null, cap == 0

struct dsss_frame {
    int N = 0, M = 0;
    bool has_geom = false, has_raw = false, has_feat = false, has_norm = false;
    bool has_sift = false;            // the frame's rows of desc128 are valid (extracted with DSSS_DESC_SIFT128 or imported)
    unsigned long long epoch = 0;     // bumped wherever has_norm is cleared or set, never reset: what a mosaic canvas recorded of the frame is stale once it differs
    const void* raw = nullptr;        // device; borrowed when the caller passed a device pointer
    int raw_type = DSSS_RAW_F64;      // element type of raw (dsss_raw_type)
    dsss_buf raw_owned{"raw_owned"};  // device; owned copy of a host image (at least raw_bytes(): a re-set with a wider type regrows it, a narrower one keeps the block)
    const void* raw_host = nullptr;   // page-locked host image whose upload is still pending (dsss_extract_many streams it in under the kernels)
    bool raw_pending = false;
    size_t raw_bytes() const { return (size_t)N * M * dsss_raw_type_size(raw_type); }
    double* pose6 = nullptr;          // device N x 6
    double* alt = nullptr;            // device N
    double* gr = nullptr;             // device M/2
    double* h_pack = nullptr;         // pinned host copy [pose6 N*6 | alt N | gr M/2] (also the pose-graph DR input)
    double* d_pack = nullptr;         // device copy, pose6 / alt / gr point into it
    size_t pack_cap = 0;              // doubles of the d_pack / h_pack family
    hipEvent_t pack_ev = nullptr;     // recorded after the upload of h_pack: the staging area is reusable once it fired
    const double* h_geo = nullptr;    // host view of [pose6 | alt | gr]: h_pack, or a slice of a dsss_frames_set batch
    int gbatch = -1;                  // batch of dsss_frames_set the geometry lives in, -1: own d_pack / h_pack
    uint8_t* mask = nullptr;          // device N x M
    uint8_t* lvl[DSSS_MAX_LEVELS] = {nullptr};  // image pyramid, lvl[0] = normalised image
    int lrows[DSSS_MAX_LEVELS] = {0}, lcols[DSSS_MAX_LEVELS] = {0};
    size_t img_cap = 0;               // bytes allocated for mask / lvl[0]
    int nkp = 0;
    double bbox[4] = {0, 0, 0, 0};
    bool has_bbox = false, bbox_async = false;
    // FAST candidates of the last extraction, per level (host, for the stage tap)
    std::vector<float> cand_x[DSSS_MAX_LEVELS], cand_y[DSSS_MAX_LEVELS], cand_r[DSSS_MAX_LEVELS];
};

// geometry of a whole dsss_frames_set call: one pinned staging area, one device buffer, ONE upload
struct dsss_geo_batch { double* d = nullptr; double* h = nullptr; size_t cap = 0; /* family: doubles of d (device) and h (pinned) */ int refs = 0; hipEvent_t ev = nullptr; };

struct dsss_comm;                        // dsss_comm.hip

struct dsss_prof {
    bool on = false;
    double ms[DSSS_K_COUNT] = {0};
    int64_t launches[DSSS_K_COUNT] = {0};
    double work[DSSS_K_COUNT] = {0};      // algorithmic bytes / flops (include/dsss.h)
    hipEvent_t e0 = nullptr, e1 = nullptr;
    // event pairs of the scopes that have been recorded but not read yet: reading them without a host synchronisation per
    // scope keeps the kernels back to back on the stream, so a short launch is timed as it runs in production (a synchronised
    // scope adds the idle-queue dispatch latency, 5-10 us, to every launch)
    struct rec { int k, nl; hipEvent_t e0, e1; };
    std::vector<rec> pending;
    std::vector<hipEvent_t> pool;
};
void dsss_prof_flush(dsss_ctx* c);       // synchronises the stream and folds the pending event pairs into ms[] / launches[]

struct dsss_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t xs[4] = {nullptr, nullptr, nullptr, nullptr};   // extra streams: frames of one extraction batch overlap on them
    hipEvent_t xev[4] = {nullptr, nullptr, nullptr, nullptr}; hipEvent_t xev_main = nullptr;
    hipEvent_t ex_lev_ev[DSSS_MAX_LEVELS] = {}, ex_cmp_ev[DSSS_MAX_LEVELS] = {}; hipEvent_t ex_side_ev[3] = {};    // extraction: FAST of level group g done (main stream), its candidate offsets known (side stream); quadtrees of a side stream done; [2]: the batch tables uploaded
    std::string err;
    dsss_mask_params mp;
    dsss_orb_params op;
    dsss_match_params mt;
    dsss_pg_params pg;
    int max_frames = 0;
    int kcap = 0;                       // per-frame feature capacity (multiple of 64)
    std::vector<dsss_frame> frames;
    // feature store, device, frame-major with stride kcap
    size_t store_cap = 0;               // the store family (kps, desc, geo, nkp_dev, rows_dev, cols_dev, bbox_dev): max_frames * kcap it was built for, 0 = none
    dsss_kp* kps = nullptr;             // [F][kcap]
    uint8_t* desc = nullptr;            // [F][kcap][32]
    dsss_buf desc128{"desc128"};                   // [F][kcap][128]: the integer-valued floats of DSSS_DESC_SIFT128 kept as bytes; allocated on first use
    dsss_buf sift_w{"sift_w"};                    // Gaussian window table of the SIFT descriptor, exp(-k / 512) (dsss_sift.hip)
    double* geo = nullptr;              // [F][kcap][2]
    int* nkp_dev = nullptr;             // [F]
    int* rows_dev = nullptr;            // [F] pings per frame
    int* cols_dev = nullptr;            // [F]
    double* bbox_dev = nullptr;         // [F][4]
    dsss_buf bbox_pinned{"bbox_pinned", DSSS_PINNED};  // [F][4] pinned host mirror, filled asynchronously
    bool bbox_pending = false;          // frames whose box has not been launched yet
    bool bbox_inflight = false; std::vector<int> bbox_inflight_ids; dsss_buf bbox_jobs_pinned{"bbox_jobs_pinned", DSSS_PINNED};      // boxes queued on the stream (dsss_bboxes_enqueue), not yet copied into dsss_frame::bbox
    dsss_buf bbox_jobs_dev{"bbox_jobs_dev"};             // [max_frames] job records of dsss_sync_bboxes (a hipMalloc / hipFree pair per call cost 0.15 ms)
    // extraction scratch (grown on demand)
    dsss_buf ex_scratch{"ex_scratch"}, ex_pinned{"ex_pinned", DSSS_PINNED};
    bool ex_tab_uploaded = false;      // ex_side_ev[2] has been recorded: the upload of the pinned batch tables may be waited for
    // extraction started by dsss_frames_set (everything but the kernel that needs the geometry): for which frames, under which parameters
    bool ex_eager_valid = false; std::vector<int> ex_eager_ids; dsss_orb_params ex_eager_op; dsss_mask_params ex_eager_mp;
    std::vector<dsss_geo_batch> gbatches;
    // pose-graph solver arena: device chunks kept between solves (dsss_pg.hip), bump-allocated, reset per solve
    std::vector<std::pair<void*, size_t>> pg_chunks; size_t pg_chunk_cur = 0, pg_chunk_off = 0;
    // matcher state
    dsss_buf mt_aux{"mt_aux"};                                   // per-frame pointer tables + cv::RNG stream
    const double** d_ptrs = nullptr;                   // [3][max_frames]: alt, gr, pose6 device pointers
    int npairs = 0, nactive = 0;
    std::vector<int> pair_s, pair_t, pair_active;   // pair_active[p] = active index or -1
    int* act_s = nullptr; int* act_t = nullptr;     // device [nactive]; with kp7_off the per-pair index family (pair_idx_cap): both dsss_match_pairs and dsss_lc_solve_pairs fill it
    int32_t* corres_nn = nullptr;       // [2*nactive][kcap]
    int32_t* corres = nullptr;          // [2*nactive][kcap]
    int* scc_hist = nullptr; int* scc_count = nullptr; double* scc_model = nullptr; // [2*nactive]
    int* row_cnt = nullptr; int* kp7_cnt = nullptr; int* row_off = nullptr; int* kp7_off = nullptr; // [nactive(+1)]
    std::vector<int> h_row_off, h_kp7_off;
    double* rows6 = nullptr; double* kp7 = nullptr; int* kp7_pair = nullptr; uint8_t* kp7_flip = nullptr;
    int total_rows = 0, total_kp7 = 0;
    size_t pair_idx_cap = 0, match_cap_pairs = 0, rows_cap = 0;   // pairs of act_s / act_t / kp7_off; of the matcher's own per-pair buffers; rows of rows6 / kp7 / kp7_pair / kp7_flip
    bool corres_valid = false;          // corres_nn / corres / scc_* belong to the current result set (dsss_match_pairs', not dsss_lc_solve_pairs')
    // geo grid of the matcher: keypoints of the active pairs' frames sorted by cell (geo, descriptor, original index), cell offsets + tables
    double* mt_gs_geo = nullptr; uint8_t* mt_gs_desc = nullptr; int* mt_gs_idx = nullptr; size_t mt_gs_cap = 0;
    dsss_buf mt_cells{"mt_cells"}; unsigned long long mt_evals_host = 0;
    // LC results
    dsss_buf lcs{"lcs"}; bool has_lc = false;  // dsss_lc[total_kp7 (+ 1024)]
    // per-geometry extraction tables (dsss_extract.hip owns the type; freed through geoms_free by dsss_destroy)
    void* geoms = nullptr; void (*geoms_free)(void*) = nullptr;
    dsss_comm* comm = nullptr;          // ranks of one job (dsss_comm_init): null = single process
    int pg_parts = 0;                   // pose-graph partitions (0: one per rank); > ranks only to exercise the interface logic on few GPUs
    dsss_buf tmp_dev{"tmp_dev"};                   // 64 ints of device scratch for one-value results (dsss_descriptor_distance)
    dsss_buf ag_buf{"ag_buf"};                                            // staging of dsss_features_allgather: world x (frames per rank) packed records, kept between calls
    dsss_buf ag_host{"ag_host", DSSS_PINNED};                              // page-locked landing place of the gathered headers (keypoint counts, boxes, sizes) and of the verdict on them
    dsss_buf ag_home{"ag_home"};                                          // its device twin: ag_check_kernel writes it before the unpack pass runs, ONE download brings it home
    dsss_buf xch_dev{"xch_dev"};                                           // device scratch of the loop-closure exchange between ranks (dsss_posegraph_solve)
    dsss_buf pg_edges_host{"pg_edges_host", DSSS_PINNED};                        // page-locked staging of the selected LC edges (dsss_posegraph_solve)
    dsss_buf pg_ab_host{"pg_ab_host", DSSS_PINNED};                     // their end points as packed (a, b) pairs
    dsss_buf xch_host{"xch_host", DSSS_PINNED};                             // page-locked landing place of the gathered edge records of all ranks (bytes)
    dsss_buf pg_scal_host{"pg_scal_host", DSSS_PINNED};                         // page-locked landing place of the LM trial's scalars (8 doubles)
    std::vector<int> pg_last_levels;                            // schedule of the last solve, four ints per panel level: items, widest panel (scalar columns), tallest rows below, this rank's or the interface's (dsss_posegraph_schedule_get)
    int pg_last_trials = 0;                                     // factorisations of the last solve
    dsss_buf pg_stage{"pg_stage", DSSS_PINNED};                             // page-locked staging of the analysis tables: one upload per solve (pg_dev::flush)
    // online use (dsss_posegraph_update): the estimate of the previous update stays on the device, the LC edges accumulate
    dsss_buf pg_warm{"pg_warm"}; int pg_warm_n = 0;   // pose_t[pg_warm_n]
    std::vector<dsss_lc_edge> pg_inc_edges; unsigned long long lc_gen = 0, pg_inc_gen = 0;    // lc_gen counts LC result sets; the last one consumed
    dsss_buf mosaic_buf{"mosaic_buf"};                                        // device scratch of dsss_mosaic_*: accumulators, output layers, job table, trajectory rows (kept between calls)
    dsss_buf mosaic_pinned{"mosaic_pinned", DSSS_PINNED};                     // page-locked landing area of the segment registration: the records of mosaic_peak_kernel, or on the host path the table of sums (140 MB at the headline size: a pageable copy into fresh memory cost more than the kernels)
    dsss_buf mosaic_gain{"mosaic_gain"}; int mosaic_gain_M = 0;              // the range-gain table (dsss_mosaic_gain_set, _set_banded): nbands x M u16 gains, Q8, on the device; M = 0: none set
    dsss_gain_bands mosaic_bands{0.0, 1.0, 1, 0};                             // the altitude bands of that table (dsss_mosaic_gain_set_banded): nbands rows of M gains; one band: the column table
    unsigned long long gain_epoch = 0;                                        // bumped by every change of that table (gain_install): a mosaic canvas records it
    std::vector<struct dsss_canvas*> canvases;                                // the mosaic canvases of this context (dsss_mosaic_canvas.hip); dsss_destroy frees what is left
    dsss_reg_call_info reg_info{0, 0, 0, 0};                                  // what the last registration call that returned DSSS_OK did (dsss_mosaic_register_info)
    dsss_buf pgr_buf{"pgr_buf"};                                           // device scratch of dsss_posegraph_edge_report (dsss_pg_report.hip), kept between calls
    dsss_prof prof;
};

#define DSSS_FAIL(ctx, code, ...) do { char _b[512]; snprintf(_b, sizeof _b, __VA_ARGS__); (ctx)->err = _b; return (code); } while (0)
#define HIPCHK(ctx, call) do { hipError_t _e = (call); if (_e != hipSuccess) return dsss_hip_fail((ctx), _e, __FILE__, __LINE__, #call); } while (0)
inline int dsss_hip_fail(dsss_ctx* c, hipError_t e, const char* file, int line, const char* call)
{
    char b[512]; snprintf(b, sizeof b, "%s:%d %s -> %s", file, line, call, hipGetErrorString(e));
    c->err = b; return DSSS_E_HIP;
}

inline int dsss_alloc_fail(dsss_ctx* c, hipError_t e, const char* name, const char* step, size_t bytes)
{
    char b[512]; snprintf(b, sizeof b, "%s: %s (%zu bytes) -> %s", name, step, bytes, hipGetErrorString(e));
    c->err = b; return DSSS_E_HIP;
}

inline int dsss_buf::reserve(dsss_ctx* c, size_t need_bytes, size_t alloc_bytes)
{
    if (cap >= need_bytes) return DSSS_OK;
    hipError_t e = p ? hipStreamSynchronize(c->stream) : hipSuccess;
    if (e != hipSuccess) { release(); return dsss_alloc_fail(c, e, name, "hipStreamSynchronize before the old block goes", alloc_bytes); }
    release();                                              // whatever fails from here on leaves p == nullptr, cap == 0
    void* q = nullptr;
    if ((e = dsss_mem_alloc(&q, alloc_bytes, pinned)) != hipSuccess) return dsss_alloc_fail(c, e, name, pinned ? "hipHostMalloc" : "hipMalloc", alloc_bytes);
    p = q; cap = alloc_bytes;
    return DSSS_OK;
}
// the new block is complete before the old one goes: a failure leaves the buffer as it was
inline int dsss_buf::reserve_keep(dsss_ctx* c, size_t need_bytes, size_t alloc_bytes, size_t keep_bytes)
{
    if (cap >= need_bytes) return DSSS_OK;
    hipError_t e = p ? hipStreamSynchronize(c->stream) : hipSuccess;
    if (e != hipSuccess) return dsss_alloc_fail(c, e, name, "hipStreamSynchronize before the old block goes", alloc_bytes);
    dsss_buf nw(name, pinned);
    if ((e = dsss_mem_alloc(&nw.p, alloc_bytes, pinned)) != hipSuccess) { nw.p = nullptr; return dsss_alloc_fail(c, e, name, pinned ? "hipHostMalloc" : "hipMalloc", alloc_bytes); }
    nw.cap = alloc_bytes;
    if (keep_bytes > 0 && p && (e = hipMemcpy(nw.p, p, keep_bytes, hipMemcpyDeviceToDevice)) != hipSuccess) return dsss_alloc_fail(c, e, name, "copy of the kept prefix", keep_bytes);      // (nw frees itself)
    *this = std::move(nw);
    return DSSS_OK;
}
template <class Fam> int dsss_family_alloc(dsss_ctx* c, const char* name, size_t& cap, size_t new_cap, const Fam& fam)
{
    bool any = false;
    for (const dsss_fam_slot& s : fam) any = any || *s.pp != nullptr;
    hipError_t e = any ? hipStreamSynchronize(c->stream) : hipSuccess;
    dsss_family_release(cap, fam);
    if (e != hipSuccess) return dsss_alloc_fail(c, e, name, "hipStreamSynchronize before the old blocks go", 0);
    for (const dsss_fam_slot& s : fam) {
        void* q = nullptr;
        if ((e = dsss_mem_alloc(&q, s.bytes, s.pinned)) != hipSuccess) { dsss_family_release(cap, fam); return dsss_alloc_fail(c, e, name, s.pinned ? "hipHostMalloc" : "hipMalloc", s.bytes); }
        *s.pp = q;
    }
    cap = new_cap;
    return DSSS_OK;
}

// kernel-family timing with HIP events on the context stream (dsss_profile_*)
struct dsss_scope {
    dsss_ctx* c; int k; int nl; hipEvent_t e0 = nullptr, e1 = nullptr;     // own event pair: scopes may nest (pose-graph solve)
    static hipEvent_t take(dsss_ctx* c) {
        hipEvent_t e = nullptr;
        if (!c->prof.pool.empty()) { e = c->prof.pool.back(); c->prof.pool.pop_back(); } else hipEventCreate(&e);
        return e;
    }
    dsss_scope(dsss_ctx* c_, int k_, double work = 0, int launches = 1) : c(c_), k(k_), nl(launches) {
        if (c->prof.on) { c->prof.work[k] += work; e0 = take(c); e1 = take(c); hipEventRecord(e0, c->stream); }
    }
    ~dsss_scope() {
        if (e0) {
            hipEventRecord(e1, c->stream);
            c->prof.pending.push_back({ k, nl, e0, e1 });
            if (c->prof.pending.size() >= 16384) dsss_prof_flush(c);
        }
    }
};

// The DSSS_* environment switches outside the pose graph (those: pg_switches, dsss_pg_sym.h).  Read ONCE PER CALL by the C entry that
// needs them (dsss_frames_set, dsss_extract, dsss_extract_many, dsss_match_pairs, the four dsss_mosaic_register* entries) and handed down: one process may flip them between calls.
struct dsss_switches {
    size_t ex_scratch_mb = 24576;            // DSSS_EX_SCRATCH_MB: bound of the extraction's batch scratch, max(1, atoi)
    int ex_upload_batch = 8;                 // DSSS_EX_UPLOAD_BATCH: frames per batch while host images are still streamed in, max(1, atoi)
    bool ex_verbose = false;                 // DSSS_EX_VERBOSE: set at all
    int fs_threads = 0;                      // DSSS_FS_THREADS: atoi; not above 0 = dsss_frames_set's own rule
    bool mt_grid = true;                     // DSSS_MT_GRID: off only when set and atoi == 0
    const char* sift_hist_dump = nullptr;    // DSSS_SIFT_HIST_DUMP: the path
    bool reg_peaks_host = false;             // DSSS_REG_PEAKS: on only when set to "host" (the registration decides its peaks on the host even without sums_host)
};
dsss_switches dsss_switches_read();      // dsss_ctx.hip

void dsss_extract_eager(dsss_ctx* c, const int* ids, int n, const dsss_switches& sw);      // dsss_frames_set: start extracting the frames whose images are in HBM
int dsss_ensure_store(dsss_ctx* c);                 // allocate the feature store for the current kcap
int dsss_ensure_sift_store(dsss_ctx* c);            // ... and the 128-byte rows + the window table (DSSS_DESC_SIFT128)
struct ex_frame;
void dsss_launch_sift_desc(dsss_ctx* c, hipStream_t st, const ex_frame* d_exf, int kcap, int nb, const char* hist_dump);      // dsss_sift.hip; hist_dump: dsss_switches::sift_hist_dump
int dsss_frame_geo_bbox(dsss_ctx* c, int id);       // device computation of the geo bounding box (asynchronous)
int dsss_bboxes_enqueue(dsss_ctx* c);               // queue the pending boxes on the context's stream (no synchronisation)
int dsss_sync_bboxes(dsss_ctx* c);                  // make dsss_frame::bbox valid on the host
int dsss_frame_kp_geo(dsss_ctx* c, int id, int n);  // geo lookup of the stored keypoints (frame.cpp:126-165)
// the device buffers of a pair result set have ONE owner, dsss_match.hip: each reserve grows one family (synchronise, free + null, allocate, then publish the capacity)
int dsss_mt_reserve_pair_index(dsss_ctx* c, size_t npairs);   // act_s, act_t, kp7_off: what lc_kernel and dsss_posegraph_select read per pair
int dsss_mt_reserve_pair_match(dsss_ctx* c, size_t npairs);   // corres_nn, corres, scc_*, row_cnt, kp7_cnt, row_off: the matcher's own, 2 * npairs * kcap correspondences
int dsss_mt_reserve_rows(dsss_ctx* c, size_t n);              // rows6, kp7, kp7_pair, kp7_flip for n rows (+ 1024 when it grows)
int dsss_mt_upload_ptr_tables(dsss_ctx* c);                   // grows mt_aux, sets d_ptrs and queues the upload of the [3][max_frames] pointer tables
void dsss_mt_clear_results(dsss_ctx* c);                      // the EMPTY result set: no pairs, no rows, has_lc = false
void dsss_mt_free(dsss_ctx* c);                               // every buffer above and the geo grid's, and the result set they held (dsss_destroy, dsss_set_params)
void dsss_pg_free(dsss_ctx* c);
void dsss_comm_free(dsss_ctx* c);
void dsss_canvas_free_all(dsss_ctx* c);      // dsss_mosaic_canvas.hip: the canvases dsss_canvas_destroy has not freed
int dsss_comm_rank(const dsss_ctx* c);
int dsss_comm_world(const dsss_ctx* c);
int dsss_comm_allreduce(dsss_ctx* c, double* dev, size_t n, hipStream_t st);
int dsss_comm_allgather(dsss_ctx* c, void* recv_dev, size_t bytes_per_rank, hipStream_t st);    // own slice in place at rank * bytes   // in-place sum over the ranks, ordered on st

// deterministic sin/cos shared by every kernel that must agree with the oracle bit for bit:
// Cody-Waite reduction + fdlibm kernel polynomials, plain IEEE mul/add only (library built -ffp-contract=off)
__host__ __device__ inline void dsss_sincos(double x, double* s, double* c)
{
    const double invpio2 = 6.36619772367581382433e-01;
    const double pio2_1 = 1.57079632673412561417e+00;
    const double pio2_1t = 6.07710050650619224932e-11;
    double k = rint(x * invpio2);
    double r = (x - k * pio2_1) - k * pio2_1t;
    double z = r * r;
    double ps = 1.58969099521155010221e-10;
    ps = ps * z + -2.50507602534068634195e-08;
    ps = ps * z + 2.75573137070700676789e-06;
    ps = ps * z + -1.98412698298579493134e-04;
    ps = ps * z + 8.33333333332248946124e-03;
    ps = ps * z + -1.66666666666666324348e-01;
    double sr = r + (r * z) * ps;
    double pc = -1.13596475577881948265e-11;
    pc = pc * z + 2.08757232129817482790e-09;
    pc = pc * z + -2.75573143513906633035e-07;
    pc = pc * z + 2.48015872894767294178e-05;
    pc = pc * z + -1.38888888888741095749e-03;
    pc = pc * z + 4.16666666666666019037e-02;
    double cr = (1.0 - 0.5 * z) + (z * z) * pc;
    long long q = ((long long)k) & 3;
    if (q == 0) { *s = sr; *c = cr; }
    else if (q == 1) { *s = cr; *c = -sr; }
    else if (q == 2) { *s = -sr; *c = -cr; }
    else { *s = -cr; *c = sr; }
}

// Frame::GetGeoImg for one bin (frame.cpp:126-165); port column 0 clamps the one-past-the-end read.  In two steps, because the bearing of
// a side is the same for every bin of a ping: a kernel that walks a whole ping (dsss_mosaic.hip) takes the first step once per side.
__host__ __device__ inline void dsss_geo_side(const double* P, bool starboard, double* s, double* c)      // P: the ping's pose row
{
    dsss_sincos(starboard ? P[2] + DSSS_PI_REF / 2 : P[2] - DSSS_PI_REF / 2, s, c);
}
// the ground-range index of a column: the bins of a side counted from the nadir (the port columns 0 and 1 share the last one)
__host__ __device__ inline int dsss_geo_index(int M, int col)
{
    int half = M / 2, idx;
    if (col >= half) idx = col - half;
    else { idx = half - col; if (idx > half - 1) idx = half - 1; }
    return idx;
}
__host__ __device__ inline void dsss_geo_bin(const double* P, const double* gr, int M, int col, double s, double c, double* x, double* y)
{
    const int idx = dsss_geo_index(M, col);
    *x = (P[3] - 0.0) + gr[idx] * c;
    *y = (P[4] - 0.0) + gr[idx] * s;
}
__host__ __device__ inline void dsss_geo_at(const double* pose6, const double* gr, int M, int row, int col,
                                            double* x, double* y)
{
    const double* P = pose6 + (size_t)row * 6;
    double s, c;
    dsss_geo_side(P, col >= M / 2, &s, &c);
    dsss_geo_bin(P, gr, M, col, s, c, x, y);
}
// One ping of a segment rotated by theta about the pivot (cx, cy) (include/dsss.h, "dense loop closures with a yaw fan"): s, c =
// dsss_sincos(theta).  The only place this arithmetic is written: mosaic_scatter_fan_kernel, the windows of rotated segments and
// dsss_register_rotate_rows call it.  theta == 0 copies the row, so the unrotated angle is the existing registration bit for bit.
__host__ __device__ inline void dsss_rotate_row(const double* row, double cx, double cy, double theta, double s, double c, double* out)
{
    out[0] = row[0]; out[1] = row[1]; out[5] = row[5];
    if (theta == 0.0) { out[2] = row[2]; out[3] = row[3]; out[4] = row[4]; return; }
    const double dx = row[3] - cx, dy = row[4] - cy;
    out[3] = cx + (c * dx - s * dy);
    out[4] = cy + (s * dx + c * dy);
    out[2] = row[2] + theta;
}
// a DR yaw that switches the sticky pi-yaw compensation of LoopClosingTFs on (optimizer.cpp:697-703)
__host__ __device__ inline bool dsss_yaw_flips(double yaw) { return fabs(yaw) > 2 * DSSS_PI_REF / 3; }

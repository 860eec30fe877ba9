/*
 * include/dsss.h -- C ABI of the MI355X-native diasss hot path (libdsss.so).
 *
 * The reference (halajun/diasss) has no plugin/FFI layer: its boundary is the C++ API that
 * src/diasss2.cpp compiles against (Frame, FEAmatcher, Optimizer, Util).  The host-side mirror of those
 * classes lives in diasss_amd/host/ and calls ONLY the entry points declared here; every entry point cites
 * the reference interface it replaces (path:line under /root/reference).
 *
 * Conventions
 *   - plain C: opaque context, plain pointers and sizes, no C++/torch types;
 *   - return 0 (DSSS_OK) or a negative DSSS_E_* code, never throws; dsss_last_error() has the detail;
 *   - the context owns all device memory and HIP streams; one context per (host thread, device);
 *   - every input pointer may be a HOST or a DEVICE pointer (copied with hipMemcpyDefault);
 *     output pointers named *_host are host memory;
 *   - frames are identified by their img_id (0..F-1), which is also the index diasss2.cpp:84 uses;
 *   - there is NO CPU fallback: without a HIP device dsss_create fails with DSSS_E_NODEVICE.
 *   - ORDER.  The work of a context is ordered on its own stream (dsss_stream), which does not synchronise with the null stream; one thread
 *     at a time calls into a context, and contexts of different threads share nothing a caller can see.  Three kinds of entry:
 *       * entries that return with device work QUEUED, asynchronous until dsss_sync or the next entry that downloads: dsss_frame_set[_typed]
 *         and dsss_frames_set[_typed] (the geometry upload and the geo boxes; for images in HBM dsss_frames_set also the started extraction),
 *         and dsss_lc_solve_all and dsss_lc_solve_pairs, which ends in it (the mini-LM launch);
 *       * entries that answer from host state and neither queue nor wait: the parameter and partition setters (dsss_set_params waits only
 *         when the keypoint capacity changes), dsss_posegraph_reset / _online_edges / _schedule_get, dsss_frame_raw_info, dsss_comm_stats,
 *         dsss_comm_frame_owner, dsss_mosaic_bounds, dsss_mosaic_register_info, dsss_mosaic_register_edges[_yaw], and the getters where
 *         they are asked for a count alone;
 *       * every other entry has synchronised the stream before it returns: its *_host outputs are complete, and an error it reports covers
 *         everything it queued (dsss_mosaic_render and its kin therefore synchronise even with every output NULL: DSSS_E_CAPACITY is read back).
 *     A caller relies on the outputs and on the list of the first kind; whether an entry of the third kind waits once or several times, and
 *     where, is not part of the contract.
 *     An entry may be called whatever the stream still holds -- work of earlier entries, or the caller's own work queued on dsss_stream:
 *     every copy into memory that queued work reads or writes is ordered on the stream.
 *   - CALLER BUFFERS.  A PAGEABLE host input (images, geometry, features, records, edges, trajectory rows, tables) has been copied, to the
 *     device or to a staging area of the context, when the call returns: the caller may reuse or free it at once, also after the entries
 *     that return with work queued.  Page-locked raw images and device pointers are the two exceptions, stated at dsss_frame_set.
 *     What is tested (tests/test_gpu_inflight.py): every entry called with the stream held back gives the bytes it gives on an idle stream,
 *     dsss_frames_set over images in HBM returns before the stream has caught up, dsss_mosaic_render does not.  The three kinds are not
 *     told apart entry by entry there, and no test overwrites a pageable input straight after the call: that rule stands by the code, where
 *     every such input is copied by a host-blocking copy, or into a staging area, before the entry returns.
 */
#ifndef DSSS_H
#define DSSS_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSSS_OK            0
#define DSSS_E_NODEVICE   -1   /* no HIP device / hipSetDevice failed */
#define DSSS_E_ARG        -2   /* bad argument (null, range, size) */
#define DSSS_E_HIP        -3   /* a HIP runtime call failed */
#define DSSS_E_STATE      -4   /* call order violated (e.g. match before features exist) */
#define DSSS_E_CAPACITY   -5   /* a caller buffer or an internal fixed-capacity buffer is too small */
#define DSSS_E_NUMERIC    -6   /* linear system not positive definite / non-finite value */
#define DSSS_E_COMM       -7   /* RCCL not available / a collective failed */

typedef struct dsss_ctx dsss_ctx;

/* cv::KeyPoint subset that the path touches (ORBextractor.cpp:840-847,1103-1109) */
typedef struct { float x, y, size, angle, response; int32_t octave; } dsss_kp;

/* hard-coded locals of the reference gathered per stage ("Config / flags") */
typedef struct {                 /* frame.cpp:59,85-86 */
    double factor;  int32_t width, r, side;
} dsss_mask_params;
#define DSSS_DESC_ORB      0      /* rotated BRIEF, 256 bits (ORBextractor.cpp:1034-1041,1097: the configuration north_star names) */
#define DSSS_DESC_SIFT128  1      /* ... AND the 128-float descriptor of the live SIFT call site (ORBextractor.cpp:1043-1047,1098) as its
                                     author evidently meant it: 4 x 4 x 8 gradient-orientation histogram on the blurred level image the
                                     keypoint was found on, at its IC angle (definition: oracle/orc_sift.c)            */
typedef struct {                 /* frame.cpp:180: ORBextractor(2000, 1.2, 6, 12, 7) */
    int32_t nfeatures; float scale; int32_t nlevels, ini_th, min_th;
    int32_t descriptor;          /* DSSS_DESC_* (default DSSS_DESC_ORB) */
} dsss_orb_params;
typedef struct {                 /* FEAmatcher.cpp:63-66,108-110,143-147,189-190,329 */
    /* use_l2: 0 = the Hamming branch (:141-176) on the ORB rows; 1 = the L2 branch (:106-139, USE_SIFT) on the 32 ORB bytes the shipped
     * reference feeds it; 2 = the L2 branch on the 128-float rows of DSSS_DESC_SIFT128 (needs features extracted in that mode) */
    int32_t use_l2; double radius; int32_t bound_same, bound_diff; double l2_bound, ratio;
    int32_t scc_iters; double pix_err, merge_thr;
} dsss_match_params;
typedef struct {                 /* GTSAM LevenbergMarquardtParams() defaults + optimizer.cpp:154-160 */
    int32_t max_iters; double rel_tol, abs_tol, lambda0, lambda_factor, lambda_max, min_fidelity;
    int32_t add_noise;
} dsss_pg_params;
typedef struct { double rel[12]; double var[6]; double score; int32_t iters; int32_t pad_; double err0, err1; } dsss_lc;
typedef struct { int32_t a, b; double rel[12]; double var[6]; } dsss_lc_edge;

void dsss_mask_params_default(dsss_mask_params*);
void dsss_orb_params_default(dsss_orb_params*);
void dsss_match_params_default(dsss_match_params*);
void dsss_pg_params_default(dsss_pg_params*);

/* ------------------------------------------------------------------ context */
int  dsss_create(int device, int max_frames, dsss_ctx** out);
void dsss_destroy(dsss_ctx*);
const char* dsss_strerror(int code);
const char* dsss_last_error(const dsss_ctx*);
int  dsss_sync(dsss_ctx*);                       /* hipStreamSynchronize of the context stream */
void* dsss_stream(dsss_ctx*);                    /* hipStream_t, for event timing by the caller */
int  dsss_set_params(dsss_ctx*, const dsss_mask_params*, const dsss_orb_params*, const dsss_match_params*,
                     const dsss_pg_params*);     /* NULL keeps the current (default = reference) values */

/* ------------------------------------------------------------------ ranks (new: the reference is one process, one thread)
 * One process per GPU.  A context that joined a communicator shards the pose-graph solve of dsss_posegraph_solve[_edges]:
 * contiguous blocks of frames (poses) per rank, every rank eliminates its own block, and ONE all-reduce per LM trial sums the
 * reduced Hessian on the interface poses ([interface blocks | Schur complements | gradient]) before the small replicated
 * interface solve.  Every rank must make the same calls with the same frames and the same (all-gathered) LC edges.
 * dsss_comm_init: RCCL (ncclCommInitRank with the 128-byte id of dsss_comm_unique_id, distributed by the caller's launcher);
 * dsss_comm_init_callback: the caller sums a host buffer in place (tests on a one-GPU box, e.g. over gloo).               */
/* op 0: in-place sum over the ranks of n doubles in host_buf.  op 1: all-gather, host_buf holds world x n bytes, the caller's
 * own n bytes are in place at rank * n, the others are to be filled in.  Return 0 on success.                          */
typedef int (*dsss_comm_fn)(void* user, int op, void* host_buf, size_t n);
int dsss_comm_unique_id(void* id128_out);
int dsss_comm_init(dsss_ctx*, const void* id128, int rank, int world);
int dsss_comm_init_callback(dsss_ctx*, int rank, int world, dsss_comm_fn fn, void* user);
/* The same two operations on the DEVICE buffer itself, to be ordered on `stream` (a hipStream_t): for callers whose transport moves
 * device memory (another collective library), and for timing ONE rank of an N-rank job on a single GPU by replaying the sums a
 * lock-step run of all ranks recorded (tools/emulate_ranks.py, bench.py --emulate-rank).  op 0: n doubles at dev_buf, summed in
 * place; op 1: world x n bytes at dev_buf, own slice in place.                                                              */
typedef int (*dsss_comm_dev_fn)(void* user, int op, void* dev_buf, size_t n, void* stream);
int dsss_comm_init_device_callback(dsss_ctx*, int rank, int world, dsss_comm_dev_fn fn, void* user);
int dsss_comm_destroy(dsss_ctx*);
int dsss_comm_stats(dsss_ctx*, int* rank, int* world, double* allreduce_bytes, int64_t* allreduce_calls);
/* frames are owned in contiguous blocks: rank r owns frames [nframes r / world, nframes (r+1) / world)                     */
int dsss_comm_frame_owner(const dsss_ctx*, int nframes, int frame);
/* after every rank extracted the frames it owns: exchange the per-frame feature records (C1 of SURVEY.md 2a, one all-gather)
 * so that every rank holds the features of all nframes frames.  Refusals: an owned frame without features -- or, under
 * DSSS_DESC_SIFT128, without SIFT rows -- is DSSS_E_STATE before anything is sent; a gathered record whose count lies outside
 * [0, capacity] is DSSS_E_CAPACITY, one whose N x M is not the geometry this context holds for the frame DSSS_E_ARG, and then
 * NO frame has changed, on the device or on the host: the headers are judged before a record is unpacked.                   */
int dsss_features_allgather(dsss_ctx*, int nframes);
/* number of pose-graph partitions (default 0 = one per rank); more partitions than ranks only exercise the interface path */
int dsss_set_pg_partitions(dsss_ctx*, int nparts);

/* ------------------------------------------------------------------ Frame (frame.h:19-20, frame.cpp:18-55)
 * Frame::Frame(id, img CV_64F NxM, pose CV_64F Nx6 [roll pitch yaw x y z], altitudes[N], ground_ranges[M/2], anno)
 * raw may stay resident in HBM (device pointer): nothing is copied back to the host.
 * LIFETIME OF raw (the reference's Frame keeps a ref-counted cv::Mat, frame.cpp:23-28; a C pointer has no such thing):
 *   - device pointer: borrowed, must stay valid and unchanged until the frame is set again or the context is destroyed;
 *   - pageable host pointer: copied before the call returns, free to reuse afterwards;
 *   - PAGE-LOCKED host pointer (hipHostMalloc / hipHostRegister / torch pin_memory): NOT copied by this call -- the upload is
 *     deferred to dsss_extract / dsss_extract_many, which stream the images in on a copy stream under the kernels of the
 *     frames before them.  The buffer must stay valid and unchanged until the dsss_extract* call that covers this frame has
 *     RETURNED (with or without an error: error exits drain the copy stream first).  Setting the frame again, or
 *     destroying the context, before extracting it drops the pending upload without reading the buffer.
 * pose6 / alt / grange are copied before the call returns.                                                 */
int dsss_frame_set(dsss_ctx*, int id, const double* raw, int N, int M,
                   const double* pose6, const double* alt, const double* grange);
/* the same for n frames in one call (arrays of per-frame arguments; raw[i] may be NULL; ids distinct).  The
 * geometry of the whole call is staged once and uploaded with ONE copy; N and M must be below 65536.
 * As the reference's constructor normalises, masks and runs DetectFeature itself (frame.cpp:45-52), this call STARTS the extraction
 * of the frames whose raw image is a device pointer (asynchronously, with the parameters set at that moment) while it packs the
 * geometry; dsss_extract_many over the same frames then only finishes it.  Nothing observable changes: parameters set in between, another
 * list of frames or dsss_extract make the extraction run again from the start.                                                          */
int dsss_frames_set(dsss_ctx*, int n, const int* ids, const double* const* raw, const int* N, const int* M,
                    const double* const* pose6, const double* const* alt, const double* const* grange);
/* TYPED WATERFALLS.  Side-scan samples are 8- or 16-bit integers, or floats: the raw image may be handed over as it is instead of
 * widened to double on the host.  Results are those of the double path on (double)sample, bit for bit (every widening is exact; NaN and
 * infinities of a float behave as their doubles do).  dsss_frame_set / dsss_frames_set are the DSSS_RAW_F64 case of these; residency,
 * lifetime and the eager start are the same for every type, and one dsss_frames_set_typed call may mix types.  A device pointer need only
 * be aligned to its element.  An unknown raw_type is DSSS_E_ARG before anything is touched.                                             */
typedef enum { DSSS_RAW_F64 = 0, DSSS_RAW_F32 = 1, DSSS_RAW_U16 = 2, DSSS_RAW_U8 = 3 } dsss_raw_type;
size_t dsss_raw_type_size(int raw_type);                       /* 8, 4, 2, 1; 0 for anything else.  Needs no context */
int dsss_frame_set_typed(dsss_ctx*, int id, const void* raw, int raw_type, int N, int M,
                         const double* pose6, const double* alt, const double* grange);
int dsss_frames_set_typed(dsss_ctx*, int n, const int* ids, const void* const* raw, const int* raw_type /* n; NULL: all DSSS_RAW_F64 */,
                          const int* N, const int* M, const double* const* pose6, const double* const* alt,
                          const double* const* grange);
/* what the context holds for a frame (any output may be NULL): the type, where the image lives (0 none, 1 borrowed device pointer,
 * 2 owned device copy, 3 owned device copy whose upload from a page-locked host image is still pending), the bytes of the owned copy,
 * N M dsss_raw_type_size (0 when borrowed or none)                                                                                      */
int dsss_frame_raw_info(dsss_ctx*, int id, int* raw_type, int* where, size_t* owned_bytes);
/* mean and minimum of the raw image as the extraction computes them (the fixed summation tree), on demand, off the hot path:
 * stats2_host = { mean, min }.  DSSS_E_STATE while the frame has no image or its upload is still pending.                               */
int dsss_frame_raw_stats(dsss_ctx*, int id, double* stats2_host);
/* GetNormalizeSSS + GetFilteredMask + DetectFeature (frame.cpp:57-124,167-203) with the ORB descriptor
 * configuration of thirdparty/ORBextractor.cpp (operator() :1049-1113).  Features stay on the device.
 * Accepted geometries: N, M below 65536, N M below 2^31, every pyramid level at least 69 px each way (DSSS_E_ARG otherwise).  The
 * quadtree of a level starts with max(1, round(W / H)) nodes for a FAST range of W x H, as the reference has it, whatever that
 * number is (a frame of 69 pings has one per 37 bins); no level is culled by another tree for its width.  The first pass divides every
 * root whatever the quota is, so a level of R roots can keep 4 R keypoints: a frame for which the sum over its levels of
 * max(quota + 3, 4 R) exceeds the keypoint store of the ORB parameters in force, ((nfeatures + 3 nlevels + 63) / 64 + 1) 64, is
 * refused with DSSS_E_ARG (raise nfeatures).                                                                                          */
int dsss_extract(dsss_ctx*, int id, int* n_kp_host);
int dsss_extract_many(dsss_ctx*, const int* ids, int n);      /* same, pipelined over frames */
/* stage taps for parity tests (host outputs; any may be NULL) */
int dsss_frame_get_norm(dsss_ctx*, int id, uint8_t* norm_host, uint8_t* mask_host);            /* Frame::norm_img, flt_mask */
int dsss_frame_get_level(dsss_ctx*, int id, int level, uint8_t* img_host, int* rows, int* cols);/* mvImagePyramid[level] */
int dsss_frame_get_candidates(dsss_ctx*, int id, int level, float* x_host, float* y_host, float* resp_host,
                              int cap, int* n);                                                /* vToDistributeKeys */
/* ORBextractor::DistributeOctTree (ORBextractor.cpp:539-763) as a HOST routine: the hot path runs the device version
 * (dsss_quadtree.hip); this one exists so the CPU test-suite can pin the list semantics against the oracle without a
 * GPU.  keep_idx_host needs n entries.                                                                          */
int dsss_host_quadtree(const float* x_host, const float* y_host, const float* resp_host, int n,
                       int minX, int maxX, int minY, int maxY, int quota, int32_t* keep_idx_host, int* n_keep);
/* Frame::kps / Frame::dst (+ the geo_img samples FEAmatcher.cpp:81-82 reads) */
int dsss_features_get(dsss_ctx*, int id, dsss_kp* kps_host, uint8_t* desc_host, double* geo_host, int cap, int* n);
/* Frame::dst as the SIFT call site would fill it (N x 128 CV_32F, integer-valued 0..255): the rows of DSSS_DESC_SIFT128, in the order of
 * dsss_features_get.  DSSS_E_STATE when the frame was extracted without them.  dsss_features_set_sift imports such rows for a frame whose
 * other features were given with dsss_features_set (values are rounded and clamped to 0..255: the device keeps them as bytes).          */
int dsss_features_get_sift(dsss_ctx*, int id, float* desc128_host, int cap, int* n);
int dsss_features_set_sift(dsss_ctx*, int id, const float* desc128_host, int n);
/* import features computed elsewhere (another rank's all-gather, or a test); geo/bbox may be NULL when the
 * frame geometry was given with dsss_frame_set (they are then recomputed on the device)                     */
int dsss_features_set(dsss_ctx*, int id, int N, int M, const dsss_kp* kps, const uint8_t* desc,
                      const double* geo, const double* bbox, int n);
/* geo bounding box = the minMaxLoc pairs of FEAmatcher.cpp:71-72 / util.cpp:21-26: xmin,xmax,ymin,ymax */
int dsss_frame_bbox(dsss_ctx*, int id, double* bbox_host);
/* Frame::geo_img in full -- frame.cpp:126-165 GetGeoImg, the two N x M CV_64F matrices (x, then y; row-major) of frame.h:40.  The hot
 * path never builds them (it uses dsss_frame_bbox and the geo samples of dsss_features_get); this is for callers that read the field. */
int dsss_frame_get_geo(dsss_ctx*, int id, double* x_host, double* y_host);
/* Util::ComputeIntersection (util.h:25, util.cpp:13-43) */
int dsss_overlap(dsss_ctx*, int id_s, int id_t, float* iou_host);
/* packed per-frame feature record for collectives (all-gather over RCCL): size and (de)serialisation */
size_t dsss_features_pack_bytes(const dsss_ctx*);
int dsss_features_pack(dsss_ctx*, int id, void* dev_or_host_buf);
int dsss_features_unpack(dsss_ctx*, int id, const void* dev_or_host_buf);

/* ------------------------------------------------------------------ FEAmatcher (FEAmatcher.h:20-33)
 * One call = FEAmatcher::RobustMatching for every listed (source,target) pair, batched on the device:
 * GeoNearNeighSearch both directions (:52-321) + ConsistentCheck (:323-405) + the rows RobustMatching appends
 * to Frame::corres_kps (:35-45) + Optimizer::GetKpsPairs (optimizer.cpp:575-639) on those rows.
 * Results stay on the device; the getters copy one pair out.
 * The RESULT SET of a context (pairs, rows, kp7 lists, LC results) is replaced as a whole by dsss_match_pairs and by dsss_lc_solve_pairs:
 * either call first empties it, builds the new one aside and publishes it last.  A call that is refused (DSSS_E_ARG, DSSS_E_STATE, ...) or
 * fails after its argument check therefore leaves an EMPTY set: every getter answers DSSS_E_ARG ("pair out of range"), dsss_match_total
 * gives (0, 0) and dsss_lc_solve_all launches nothing.                                                       */
int dsss_match_pairs(dsss_ctx*, const int* src_ids, const int* tgt_ids, int npairs);
int dsss_match_get_dir(dsss_ctx*, int pair, int dir /*0: s->t, 1: t->s*/, int32_t* corres_nn_host,
                       int32_t* corres_host, int cap, int* scc_hist, int* scc_count, double* scc_model);
int dsss_match_get_rows(dsss_ctx*, int pair, double* rows6_host, int cap, int* nrows);   /* [id_s,id_t,y_s,x_s,y_t,x_t] */
int dsss_match_get_kp7(dsss_ctx*, int pair, double* kp7_host, int cap, int* n);          /* Vector7 of optimizer.cpp:625 */
int dsss_match_total(dsss_ctx*, int* total_rows, int* total_kp7);
/* (dsss_match_get_dir: DSSS_E_STATE for an active pair when the result set is dsss_lc_solve_pairs', which has no correspondences;
 * dsss_match_get_rows then gives zero rows.)
 * 0 when the geo bounding boxes of the pair are disjoint: every keypoint is then skipped by FEAmatcher.cpp:84, no kernel runs */
int dsss_match_pair_active(dsss_ctx*, int pair, int* active_host);
/* FEAmatcher::DescriptorDistance (FEAmatcher.h:33) on device-resident descriptors of two frames */
int dsss_descriptor_distance(dsss_ctx*, int id_a, int ia, int id_b, int ib, int* dist_host);

/* ------------------------------------------------------------------ Optimizer (optimizer.h:43-67)
 * LoopClosingTFs (optimizer.cpp:641-982) for every kp pair produced by dsss_match_pairs.                   */
int dsss_lc_solve_all(dsss_ctx*);
int dsss_lc_get(dsss_ctx*, int pair, dsss_lc* out_host, int cap, int* n);
/* stand-alone form: kp7 given by the caller (Optimizer::LoopClosingTFs of ONE pair, optimizer.h:61-67)     */
int dsss_lc_solve(dsss_ctx*, int id_s, int id_t, const double* kp7, int n, dsss_lc* out_host);
/* the same for the kp7 lists of MANY pairs in one launch (the pair loop of TrajOptimizationAll, optimizer.cpp:35-97,
 * with kp7 built by the caller's GetKpsPairs from corres_kps or -- USE_ANNO = 1, optimizer.cpp:26,42-53 -- anno_kps).
 * kp7: pair_off[npairs] x 7 (host or device); pair_off: npairs + 1 ascending offsets (host).  Results stay on the device
 * as after dsss_match_pairs + dsss_lc_solve_all: dsss_lc_get / dsss_posegraph_select / dsss_posegraph_solve follow.
 * It replaces the result set under the rule stated at dsss_match_pairs (empty after a refused call); every listed pair is active, with
 * its kp7 rows, no matcher rows and no correspondences.  pair_off[0] must be 0.                                          */
int dsss_lc_solve_pairs(dsss_ctx*, const int* src_ids, const int* tgt_ids, int npairs, const double* kp7, const int* pair_off_host);
/* LMTriaFactor + Optimizer::TriangulateOneLandmark (LMtriangulatefactor.cpp:10-27; optimizer.h:56-59, optimizer.cpp:984-1021)
 * for every kp7 row of one pair, as LoopClosingTFs calls it (optimizer.cpp:907-921: yaw-compensated DR poses, landmark
 * initialised as in :789-795).  out7_host: n x 7 = [x y z | |range_s err| |plane_s| |range_t err| |plane_t|]          */
int dsss_triangulate(dsss_ctx*, int id_s, int id_t, const double* kp7, int n, double* out7_host);
/* the same with the caller's poses and start point (the literal signature of optimizer.h:56-59, Ts = identity):
 * in27: n x [Tp_s R(9) t(3) | Tp_t R(9) t(3) | lm_ini(3)]; of kp7 only the slant ranges [2], [5] are read          */
int dsss_triangulate_poses(dsss_ctx*, const double* kp7, const double* in27, int n, double* out7_host);
/* TrajOptimizationAll (optimizer.h:43; optimizer.cpp:101-279): LC selection + batch LM over every ping of
 * every frame 0..nframes-1 (frames must have been given with dsss_frame_set). poses12_host: total x 12
 * (R row-major, t); rpy6_host: total x 6 "r p y x y z" as SaveTrajactoryAll writes (:1164-1214), may be NULL.
 * Page-locked output buffers make the download run at PCIe speed.                                             */
int dsss_posegraph_select(dsss_ctx*, int nframes, dsss_lc_edge* edges_host, int cap, int* n_edges);
int dsss_posegraph_solve(dsss_ctx*, int nframes, double* poses12_host, double* rpy6_host, double* stats4_host);
/* N3, the online use (optimizer.cpp:134-139, 262-272: one ISAM2 object, isam.update as pings arrive, calculateEstimate):
 * dsss_posegraph_update solves frames 0..nframes-1 like dsss_posegraph_solve, but (a) starts from the estimate the previous
 * update of this context left for the pings it covered (new pings start at DR o noise as in the reference), and (b) works on
 * the ACCUMULATED loop closures: every LC result set (dsss_lc_solve_all / dsss_lc_solve_pairs) is consumed once, by the next
 * update; its pairs must lie within the nframes frames.  dsss_posegraph_reset forgets estimate and edges.  Single rank.     */
int dsss_posegraph_update(dsss_ctx*, int nframes, double* poses12_host, double* rpy6_host, double* stats4_host);
/* The INCREMENTAL form (round 6): the same bookkeeping, but only the last `window_frames` frames are solved -- their pings and the loop
 * closures that end in them -- CONDITIONED on the estimate the earlier updates left for everything before: the window's first ping is pinned
 * there, a loop closure from a frozen ping into the window keeps its exact residual with the frozen end folded into its measurement, closures
 * between frozen pings drop out.  Cost of an update: the window, whatever the length of the survey (the global form re-analyses and
 * re-factorises the whole graph, O(F) per update, O(F^2) over a survey).  The frozen part is NOT revisited: what iSAM2 does for variables
 * below its relinearisation threshold (optimizer.cpp:134-137) done by age -- a later dsss_posegraph_update (global, warm-started from these
 * estimates: one or two LM trials) gives the batch optimum, which is all the reference ever reads (calculateEstimate after the loop, :279).
* poses12_host / rpy6_host (either may be NULL: nothing is downloaded) receive ALL pings of frames 0 .. nframes-1.  Falls back to the global
 * form while there is no frozen part (nframes <= window_frames); a window that would start in frames no update has covered (window_frames = 1:
 * the new frame alone) is extended backwards to the last frame that has an estimate, which anchors it.  Loop closures must end in the later ping (the pipeline's do).
 * The window is its own LM problem: its prior (sigma 1e-6) measures the PREVIOUS ESTIMATE of its first ping, not that ping's dead-reckoned
 * pose; pings no update has covered start at DR o noise and draw their noise by WINDOW-LOCAL index (ping i of the window takes the draws
 * 6 i .. 6 i + 5 of the one normal stream, as ping i of a batch solve does).                                                          */
int dsss_posegraph_update_window(dsss_ctx*, int nframes, int window_frames, double* poses12_host, double* rpy6_host, double* stats4_host);
int dsss_posegraph_reset(dsss_ctx*);
int dsss_posegraph_online_edges(dsss_ctx*);      /* loop closures accumulated so far (>= 0) */
/* Instrumentation (no reference counterpart: GTSAM keeps its elimination tree to itself): the panel levels of the last solve of this
 * context, four ints per level in launch order -- panel steps on the level, scalar columns of its widest panel, scalar rows below its
 * tallest one, 1 for a level of the replicated interface tree -- and the number of factorisations (LM trials) that solve ran.        */
int dsss_posegraph_schedule_get(dsss_ctx*, int* levels4_host, int cap_levels, int* n_levels, int* n_trials);
/* stand-alone form: explicit DR chain + edges.  total >= 2: a graph of one pose has nothing to solve and is refused with DSSS_E_ARG, as an
 * edge out of range or with a == b is, before anything is launched.  A variance that is not finite and positive is DSSS_E_NUMERIC, found later,
 * once the dead reckoning is on the device and the analysis has started, but before any factor is linearised.  Any variance that is finite and positive is taken; one so small that the
 * normal equations are not finite makes every trial's factorisation fail: lambda walks to lambda_max and the start values come back
 * (stats4 = { 0, err0, err0, lambda }).                                                                          */
int dsss_posegraph_solve_edges(dsss_ctx*, const double* dr6, int total, const dsss_lc_edge* edges, int ne,
                               double* poses12_host, double* stats4_host);

/* ------------------------------------------------------------------ loop-closure residual report and chi-square gated solve (new: the
 * reference hands every selected closure to the optimiser, optimizer.cpp:203-258, and never asks whether it agrees with the result)
 * every factor of the pose graph (dr6 chain + edges, exactly the graph dsss_posegraph_solve_edges builds) evaluated at poses12
 * (total x 12, R row-major | t; host or device pointer).  chi2_host[ne], r6_host[ne x 6] (may be NULL),
 * sums3_host (may be NULL) = { 0.5 sum over the chain factors, 0.5 sum over the loop closures, their sum = the LM objective }.
 * r6[e][a] = Log(rel_e^-1 X_a^-1 X_b)[a] / sqrt(var_e[a]), chi2[e] = sum_a r6[e][a]^2 (a = 0..5 in order).  The sums are fixed-order
 * trees: identical from call to call.  total >= 1, ne == 0 is valid.  DSSS_E_ARG: an edge index out of range or a == b, a variance that is
 * not positive and finite, a rel that is not finite.  Single rank (DSSS_E_STATE with a communicator of more than one rank).          */
int dsss_posegraph_edge_report(dsss_ctx*, const double* dr6, int total, const dsss_lc_edge* edges, int ne,
                               const double* poses12, double* chi2_host, double* r6_host, double* sums3_host);

/* The gated solve.  All edges start kept; repeat: (1) dsss_posegraph_solve_edges on the kept edges, compacted in their original order;
 * (2) report the kept edges at the result, m = their largest chi2 (a non-finite one counts as +inf); (3) m <= gate, or this was solve
 * number max_solves: stop; (4) drop every kept edge with chi2 > max(gate, m / decade), go to (1).  (m = +inf drops nothing and stops.)
 * poses12_host and stats4_host are those of the last solve, keep_host the final mask, chi2_host ALL ne edges (dropped ones included) at
 * the returned trajectory, n_solves_host the number of solves; with every edge dropped the last solve is the chain alone.
 * params NULL: the defaults.  DSSS_E_ARG: gate not above 0, decade not above 1, max_solves < 1, and what the report rejects.  Single rank. */
typedef struct { double gate, decade; int32_t max_solves, pad_; } dsss_pg_gate_params;
void dsss_pg_gate_params_default(dsss_pg_gate_params*);   /* gate 22.458 (chi-square, 6 dof, p = 0.999), decade 10, max_solves 8 */
int dsss_posegraph_solve_gated(dsss_ctx*, const double* dr6, int total, const dsss_lc_edge* edges, int ne,
                               const dsss_pg_gate_params*, double* poses12_host, double* stats4_host,
                               uint8_t* keep_host /* ne */, double* chi2_host /* ne, may be NULL */, int* n_solves_host);

/* Host twin of the pose-graph linear solve (ordering + symbolic analysis + multifrontal factorisation of the reduced
 * system, diasss_amd/csrc/dsss_pg_sym.cpp) so that the CPU test-suite can pin the analysis the device kernels run on without
 * a GPU; the hot path runs the numeric phase in dsss_pg.hip.  Matrix: ns block variables (6x6 blocks); value index v < ns is
 * the diagonal block of variable v, ns + e the block H(edge_a[e], edge_b[e]); the first ns-1 edges must be the chain (e, e+1).
 * part (may be NULL): rank of every variable, non-decreasing.  x: ns x 6.  stats8: nnz(L) blocks, fronts, panels, levels,
 * front arena doubles, comm doubles, binned columns, largest front (block rows).                                          */
int dsss_host_pg_solve(int ns, const int32_t* edge_a, const int32_t* edge_b, int nedges, const double* cx, const double* cy,
                       const int32_t* part, int nparts, const double* aval36, const double* rhs6, double* x6_host, int64_t* stats8);
/* the same for the analysis ONE RANK of several runs (dsss_pg.hip, rank-local mode): its own variables plus the interface
 * variables iface_last (ascending), which are eliminated last as one dense front whatever their edges.  Any edge list (no
 * chain prefix).  stats8[5]: original values that land in the interface front.                                            */
int dsss_host_pg_solve_local(int ns, const int32_t* edge_a, const int32_t* edge_b, int nedges, const double* cx, const double* cy,
                             const int32_t* iface_last, int nlast, const double* aval36, const double* rhs6, double* x6_host, int64_t* stats8);
/* the same for ONE rank analysed BY PARTS (pg_symbolic_parts: K parts of equal size in the chain order, each ordered and analysed on
 * its own with the interface between the parts as the last, dense front, the results joined into one set of tables); the first
 * ns-1 edges must be the chain.                                                                                               */
int dsss_host_pg_solve_parts(int ns, const int32_t* edge_a, const int32_t* edge_b, int nedges, const double* cx, const double* cy,
                             int K, const double* aval36, const double* rhs6, double* x6_host, int64_t* stats8);
/* What the binned subtrees of the analysis look like to pg_factor_subtree_kernel (the one-graph analysis with the device solve's
 * bin cost, as dsss_pg.hip runs it below 1 500 variables): which branches of the kernel a graph reaches.  prof12: bins; binned columns;
 * bins of one column; columns without updates directly after one with updates; columns whose predecessor in the bin is one of their
 * sources; columns with updates whose predecessor is none; most updates of a column NOT counting such a predecessor; most blocks of a
 * column; most roots of a bin; pairs of consecutive columns of a bin that both add to the same root's update matrix; most columns
 * of a bin; most updates of a column.                                                                                         */
int dsss_host_pg_bins_profile(int ns, const int32_t* edge_a, const int32_t* edge_b, int nedges, const double* cx, const double* cy, int64_t* prof12);

/* ------------------------------------------------------------------ mosaic (new: the reference ends at the trajectory file,
 * optimizer.cpp:1164-1214, and has no mosaic -- there is no reference line to cite for anything in this section)
 * The frames' normalised waterfalls (Frame::norm_img) binned into one georeferenced grid under a trajectory, and the disagreement of
 * overlapping frames about a cell as a trajectory-quality measure that needs neither an oracle run nor annotations.
 * Grid: cell (ix, iy) covers [x0 + ix cell, x0 + (ix+1) cell) x [y0 + iy cell, y0 + (iy+1) cell), layers are H x W row-major (index
 * iy W + ix), W H <= 2^28.  A pixel (row, col) of a frame lies at dsss_frame_get_geo's point for the given pose rows and falls into
 * ix = floor((x - x0) / cell), iy = floor((y - y0) / cell), evaluated and range-tested in f64: points outside the grid and non-finite
 * ones are dropped.  use_mask != 0 drops the pixels the filter mask rejects (flt_mask == 0, where DetectFeature drops keypoints).
 * Trajectory: rpy6 = HOST rows "r p y x y z" as dsss_posegraph_solve writes to rpy6_host, frame ids[i] reads the N_i rows from row
 * ping_off[i]; rpy6 == NULL: the pose6 the frames were set with (ping_off may then be NULL).  Altitudes are not used.
 * Every accumulator is an integer: results do not depend on the order of ids and are identical from call to call.  Single rank: a
 * rank renders the frames whose images it holds (after dsss_extract*; DSSS_E_STATE otherwise).  ids must be distinct.                */
typedef struct { double x0, y0, cell; int32_t W, H; int32_t use_mask; int32_t pad_; } dsss_mosaic_params;
/* the grid that covers bbox4 = xmin,xmax,ymin,ymax with cells of edge `cell`: x0 = floor(xmin / cell) cell, W = floor((xmax - x0) / cell) + 1,
 * the same in y, use_mask = 1.  Pure host arithmetic, no context.  DSSS_E_ARG: cell <= 0 or not finite, a box that is not finite, W H > 2^28 */
int dsss_mosaic_grid(const double* bbox4, double cell, dsss_mosaic_params* out);
/* union of the frames' geo extremes (the minMaxLoc pairs of dsss_frame_bbox) under the given trajectory: xmin,xmax,ymin,ymax */
int dsss_mosaic_bounds(dsss_ctx*, const int* ids, int n, const double* rpy6, const int* ping_off, double* bbox4_host);
/* sum: sum of the normalised u8 values that fell into the cell, cnt: their number (uint32, H x W); img = cnt ? (sum + cnt / 2) / cnt : 0
 * (uint8, H x W).  Any output may be NULL (all NULL: the mosaic is rendered on the device and nothing is downloaded).
 * DSSS_E_CAPACITY when a cell received more than 2^24 samples (below that the uint32 sum cannot wrap).                              */
int dsss_mosaic_render(dsss_ctx*, const int* ids, int n, const double* rpy6, const int* ping_off,
                       const dsss_mosaic_params*, uint32_t* sum_host, uint32_t* cnt_host, uint8_t* img_host);
/* every frame rendered alone, m_f = (sum_f + cnt_f / 2) / cnt_f where cnt_f > 0; per cell nfr = frames with cnt_f > 0, s1 = sum of m_f,
 * s2 = sum of m_f^2 (uint32, H x W; any may be NULL).  score = sqrt(sum_{nfr >= 2} (s2 - s1^2 / nfr) / sum_{nfr >= 2} (nfr - 1)): the pooled
 * standard deviation, in grey levels, of what overlapping frames say about a cell (f64, cells in index order; 0 without overlap).    */
int dsss_mosaic_consistency(dsss_ctx*, const int* ids, int n, const double* rpy6, const int* ping_off,
                            const dsss_mosaic_params*, uint32_t* nfr_host, uint32_t* s1_host, uint32_t* s2_host,
                            double* score_host);

/* ---- range-gain normalisation: a per-column gain table that takes the sensor-fixed profile across the swath (beam pattern, residual
 * time-varied gain; port and starboard differ) out of every sample before it is binned.  Estimated on the device, held by the context,
 * applied inside the scatter of every entry that bins samples.  All arithmetic is integer: results stay independent of frame, pair, tile
 * and atomic order and identical from call to call.  Nothing changes while no table is set.
 * Column statistics, over the listed frames, which all have the same M: S[c] = sum of norm[row, c], C[c] = the number of samples, over
 *   the kept samples of column c; a sample is kept iff use_mask == 0 or flt_mask[row, c] != 0.  Both uint64 and exact for any number of
 *   pings the mosaic accepts (total < 2^31).
 * Table (pure host arithmetic, no context, as dsss_mosaic_register_peak): parameters min_count (>= 1, default 256), smooth (0..16,
 *   default 0), target (0..255, default 0).  S'[c], C'[c] = the sums of S, C over the columns c' with |c' - c| <= smooth, 0 <= c' < M, on
 *   the same side as c (c' < M/2 iff c < M/2: the window never crosses the nadir).  Column c is eligible iff C'[c] >= min_count and
 *   S'[c] > 0.  T = target where target != 0, else (sum S + (sum C) / 2) / sum C over the UNsmoothed S, C of the eligible columns, floor
 *   division; with no eligible column (or, under smooth > 0 and target == 0, none that holds a sample of its own: sum C = 0) every gain
 *   is 256 and T = 0.  gain[c] = min(65535, (T C'[c] 256 + S'[c] / 2) / S'[c]) for an eligible column, 256 otherwise.  Gains are
 *   uint16, Q8; every intermediate value fits 64 bits for counts up to 2^31 (the function itself computes in 128).
 * Corrected sample: v' = min(255, (v gain[c] + 128) >> 8).  A gain of 256 returns v exactly, so a table of 256s reproduces the layers
 *   without a table bit for bit; v' <= 255, so the 2^24-samples-per-cell rule holds unchanged.
 * Where the table applies: dsss_mosaic_render, _consistency, _register, _register_segments, _register_segments_yaw and
 *   _register_segments_pyr, and with them the segment rows the _edges entries read.  Extraction, matching and the solves do not see it.
 * Errors.  DSSS_E_ARG: ids the mosaic entries reject, frames of differing M in one stats call, M < 2, a NULL output, parameters out of
 *   range, cap < M; and from every entry above, before anything is launched or cleared, when a table is set and a listed frame has
 *   another M.  DSSS_E_STATE: frames not extracted (the rule of dsss_mosaic_render).  Every error leaves the context usable and a table
 *   that was set in place.  Estimation and installation are two calls on purpose: a caller may install a calibrated table.
 * One row per altitude band instead of one for all pings, and the corrected waterfall as an output: "altitude-banded range gain" below. */
typedef struct { int32_t min_count, smooth, target, pad_; } dsss_gain_params;
void dsss_gain_params_default(dsss_gain_params*);
/* S -> sum_host[M], C -> cnt_host[M] of the listed frames (mosaic_gainstat_kernel at one band: one launch for all frames) */
int  dsss_mosaic_gain_stats(dsss_ctx*, const int* ids, int n, int use_mask, uint64_t* sum_host /* M */, uint64_t* cnt_host /* M */);
int  dsss_mosaic_gain_table(const uint64_t* sum, const uint64_t* cnt, int M, const dsss_gain_params* /* NULL: defaults */,
                            uint16_t* gain_q8 /* M */, int32_t* target_out /* may be NULL */);
int  dsss_mosaic_gain_set(dsss_ctx*, const uint16_t* gain_q8_host, int M);      /* NULL: clear (M ignored) */
int  dsss_mosaic_gain_get(dsss_ctx*, uint16_t* gain_q8_host, int cap, int* M);  /* *M = 0: none set; read back from the device copy */

/* ---- altitude-banded range gain: the table above with one row per altitude BAND.  A column is a slant range, a beam pattern is fixed
 * to the grazing angle, and column c looks at atan(gr[c] / h) from the altitude h: one profile per column is right only while the
 * altitude hardly moves.  A banded table holds nbands rows of M gains; a ping is corrected with the row of its altitude's band.
 * Integer arithmetic throughout, as above.  While no banded table is set, every layer of every entry is the byte it was.
 * Bands: nbands in 1..16, alt0 finite, dalt finite and > 0.  The band of an altitude a: t = floor((a - alt0) / dalt) in f64; band = 0
 *   when !(t >= 0) (NaN, -inf and altitudes below alt0), nbands - 1 when t >= nbands, (int)t otherwise; the comparisons are made on the
 *   f64 values before any conversion, as in the cell arithmetic.  dsss_gain_band evaluates it on the host (no context): the one body
 *   the kernels run.  The altitude of a sample is alt[row] as the frame was set, never a row of the trajectory passed to an entry.
 * Statistics: S[b][c], C[b][c] = the sum and the number of the kept samples of column c over the pings whose band is b (nbands x M
 *   uint64 each; mosaic_gainstat_kernel, one launch for all frames).  Kept-sample rule, frame rules and errors are those of
 *   dsss_mosaic_gain_stats, and summed over b the result is exactly its output.
 * Table (pure host arithmetic, no context): Sp[c] = sum_b S[b][c], Cp likewise; gp[c] and T = exactly what dsss_mosaic_gain_table
 *   returns on (Sp, Cp) with the same parameters.  S'_b, C'_b = the same-side smoothing window of that rule within band b.  Entry (b, c)
 *   is eligible iff C'_b[c] >= min_count and S'_b[c] > 0 and T > 0; then gain[b][c] = min(65535, (T C'_b[c] 256 + S'_b[c] / 2) / S'_b[c]),
 *   otherwise gain[b][c] = gp[c]: a thin band falls back to the pooled column, never to 256.  nbands == 1 reproduces
 *   dsss_mosaic_gain_table exactly.
 * Installation: dsss_mosaic_gain_set_banded installs nbands x M gains with their bands (NULL table: clear); dsss_mosaic_gain_set
 *   installs a one-band table as before.  dsss_mosaic_gain_get is DSSS_E_STATE while a table of more than one band is set, and writes
 *   nothing; dsss_mosaic_gain_get_banded reads any table back (*M = 0: none set; cap counts gains: nbands x M are needed; the bands of
 *   a table set through dsss_mosaic_gain_set read alt0 0, dalt 1, nbands 1).
 * Corrected sample: v' = min(255, (v gain[band(alt[row])][c] + 128) >> 8), in every entry the column table applies to and in the
 *   composite; the rule that every listed frame has the table's M is unchanged.
 * Corrected waterfall: dsss_frame_get_corrected returns the frame's normalised image (N x M uint8) under the table in force -- banded,
 *   one-band or none (then the normalised image itself) -- by mosaic_correct_kernel.  DSSS_E_STATE: the frame is not extracted;
 *   DSSS_E_ARG: a NULL output, a table of another M.
 * Errors of the new entries, DSSS_E_ARG before anything is reserved or launched: nbands outside 1..16, alt0 or dalt not finite,
 *   dalt <= 0, a NULL pointer, and whatever the column entries refuse.  An error leaves the context usable and the table in place.  */
typedef struct { double alt0, dalt; int32_t nbands, pad_; } dsss_gain_bands;
int  dsss_gain_band(const dsss_gain_bands*, double alt, int32_t* band);
int  dsss_mosaic_gain_stats_banded(dsss_ctx*, const int* ids, int n, int use_mask, const dsss_gain_bands*,
                                   uint64_t* sum_host /* nbands x M */, uint64_t* cnt_host /* nbands x M */);
int  dsss_mosaic_gain_table_banded(const uint64_t* sum, const uint64_t* cnt, int M, int nbands, const dsss_gain_params* /* NULL: defaults */,
                                   uint16_t* gain_q8 /* nbands x M */, int32_t* target_out /* may be NULL */);
int  dsss_mosaic_gain_set_banded(dsss_ctx*, const uint16_t* gain_q8_host /* nbands x M; NULL: clear */, int M, const dsss_gain_bands*);
int  dsss_mosaic_gain_get_banded(dsss_ctx*, uint16_t* gain_q8_host, int cap, int* M, dsss_gain_bands* bands);
int  dsss_frame_get_corrected(dsss_ctx*, int id, uint8_t* out_host /* N x M */);

/* ---- composite mosaic: the deliverable picture.  dsss_mosaic_render's img is the mean of every sample of a cell: right for the
 * consistency score and the ZNCC, but a blend of frames that see a patch from opposite sides.  Here a cell holds ONE sample, the winner
 * under a stated priority, with its source (frame, ping, column); enclosed holes are optionally filled from the nearest cell that holds a
 * sample.  Integer work only: independent of the order of ids, of atomic order and of the call.  No existing entry changes.
 * Samples: exactly those of dsss_mosaic_render (frames, rpy6 / ping_off, grid, use_mask, the f64 cell arithmetic and range test).  A
 *   sample's value is the normalised u8, corrected by the context's gain table when one is set (v' = min(255, (v gain[c] + 128) >> 8)).
 * Ground-range index of a column, as in the geometry of a bin: half = M / 2; col >= half: idx = col - half; otherwise
 *   idx = min(half - col, half - 1) (the port columns 0 and 1 share an index).
 * Priority rank q, smaller wins, an integer in [0, 32766]: DSSS_COMP_NEAR: idx (nearest to the track); DSSS_COMP_FAR: half - 1 - idx;
 *   DSSS_COMP_MID: |2 idx - (half - 1)| (mid-swath); DSSS_COMP_FIRST: 0 (the first line on top).
 * Canonical ping number g: the listed frames ordered by ascending frame id, NOT by their position in ids; g = the sum of N over the
 *   listed frames of a smaller id, plus the ping's row.  The mosaic refuses 2^31 pings or more in a call, so g < 2^31.
 * Winner of a cell: the sample with the smallest (q, g, col), compared lexicographically.  The triple is unique per sample, so the winner
 *   is unique and depends neither on the order of ids nor on the order of execution.  A cell with no sample is empty.
 * Frames: every listed frame has an even M, 4 <= M <= 65534 (q and col have 15 and 16 bits of the device's key).
 * Outputs, H x W row-major, any may be NULL: img (u8) the winner's value, 0 where empty; src_frame (int32) its frame id, src_ping (int32)
 *   its row in that frame, src_col (int32) its column, each -1 where empty; fill (u8) below; info: the cells that hold a sample, the
 *   cells filled, the cells left empty (direct + filled + empty = W H).
 * Gap fill, fill_radius R in 0..4 (0: none).  V0 = the cells that hold a sample; cells outside the grid are not in V0.  An empty cell
 *   (ix, iy) is enclosed iff there are a, b in [1, R] with (ix - a, iy) and (ix + b, iy) both in V0, or the same along y.  An enclosed
 *   cell takes the value and the source of its donor: the cell of V0 in the square |dx|, |dy| <= R that minimises (dx^2 + dy^2, dy, dx),
 *   the registration's tie order; one always exists.  fill = 0 for a cell of V0, dx^2 + dy^2 of the donor (1..32; in fact at most R^2,
 *   since an enclosed cell has a cell of V0 on one of its axes within R) for a filled cell, 255
 *   for a cell left empty.  Donors come from V0 only, never from filled cells: the result does not depend on the order the holes are
 *   visited in, and nothing is extrapolated beyond the covered area.
 * Errors.  DSSS_E_ARG, before anything is reserved, cleared or launched: everything dsss_mosaic_render refuses (a gain table of another
 *   M included), a frame whose M is odd or outside [4, 65534], a mode outside 0..3, fill_radius outside 0..4; for the host functions a NULL
 *   pointer, M < 4 or odd or above 65534, col outside [0, M), W or H < 1, W H > 2^28, R outside 0..4.  DSSS_E_STATE: as dsss_mosaic_render.
 *   There is no sample limit per cell: nothing is summed, DSSS_E_CAPACITY does not occur.  Every error leaves the context usable and a
 *   gain table that was set in place.  With all outputs NULL the mosaic is built on the device and nothing is downloaded.            */
#define DSSS_COMP_NEAR  0
#define DSSS_COMP_FAR   1
#define DSSS_COMP_MID   2
#define DSSS_COMP_FIRST 3
typedef struct { int32_t mode, fill_radius; } dsss_comp_params;      /* defaults DSSS_COMP_NEAR, 0 */
typedef struct { int64_t direct, filled, empty; } dsss_comp_info;
void dsss_comp_params_default(dsss_comp_params*);
/* pure host arithmetic, no context: the rank of a column; the fill rule on a layer of validity flags */
int  dsss_mosaic_comp_rank(int mode, int M, int col, int32_t* q);
int  dsss_mosaic_fill_host(const uint8_t* valid /* H x W, != 0: in V0 */, int W, int H, int R,
                           int32_t* donor /* cell index iy W + ix of the donor; own index in V0; -1 left empty */, uint8_t* fill);
int  dsss_mosaic_composite(dsss_ctx*, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params*,
                           const dsss_comp_params* /* NULL: defaults */, uint8_t* img_host, int32_t* src_frame_host,
                           int32_t* src_ping_host, int32_t* src_col_host, uint8_t* fill_host, dsss_comp_info* info_host);

/* ---- footprint rendering: mosaics without holes between pings and bins.  The entries above bin every sample as a point, so a cell
 * edge at or below the ping spacing or the bin spacing leaves empty rows between pings and empty columns between bins.  Here a sample
 * stands for its footprint, the area up to the next ping and the next bin, and is binned at up to max_steps x max_steps sub-samples of
 * it.  Integer work behind the f64 cell arithmetic, as everywhere in this section: independent of the order of ids, of execution and
 * of the call.  No existing entry changes.
 * Parameters: max_steps in 1..8 (default 4), max_gap in metres, finite and > 0 (default 1.0).  Neither default has been tuned on any
 *   data, as the registration's defaults have not.
 * Points: P(r, c) = (x, y) = dsss_frame_get_geo's point of ping r and column c under the rows in force (rpy6 / ping_off, or the frame's
 *   own pose6).  idx = the ground-range index of c ("composite mosaic" above), half = M / 2, N = the frame's pings.
 * Along step A(r, c), each component ONE f64 subtraction: r < N - 1: P(r + 1, c) - P(r, c); the last ping: P(N - 1, c) - P(N - 2, c),
 *   the step before it, so that consecutive frames of a leg leave no stripe between them; N == 1: (0, 0).
 * Across step B(r, c), outward on the sample's own side: idx < half - 1: P(r, c+) - P(r, c), c+ = the column of the same side with
 *   index idx + 1 (c + 1 on starboard, c - 1 on port); the outermost index (starboard M - 1, and port 0 and 1, which share it):
 *   P(r, c) - P(r, c-), c- = the same side's point of index idx - 1 (column M - 2 on starboard, 2 on port; with M == 4 the port side
 *   has no column of index 0 and the point is gr[0] under the port bearing).
 * Step count n(S) of a step S = (sx, sy), every comparison on the f64 values before any conversion: sx or sy not finite: 1;
 *   l = the larger of |sx| and |sy| (per axis, so consecutive sub-samples move at most one cell on either axis); l > max_gap: 1 (a jump
 *   is not bridged); t = ceil(l / cell); n = 1 if t < 1, max_steps if t > max_steps, (int)t otherwise.  dsss_mosaic_footprint_steps
 *   evaluates it on the host (no context): the one body the kernels run.
 * Sub-samples of a sample (r, c).  The parent is kept iff use_mask == 0 or flt_mask[r, c] != 0: the only test on the parent, which need
 *   not lie on the grid itself.  na = n(A), nc = n(B); for i in [0, na), j in [0, nc): X = x; if i > 0: X = X + ((double)i / (double)na) Ax;
 *   if j > 0: X = X + ((double)j / (double)nc) Bx; Y the same with the same two quotients.  Every operation is a single unfused IEEE
 *   operation in exactly this order; sub-sample (0, 0) is the point itself and is never recomputed.  Each sub-sample is binned and
 *   range-tested on its own by the f64 cell arithmetic above.  Its value is the parent's normalised u8, corrected by the gain table in
 *   force with the parent's column and the parent's altitude band.
 * dsss_mosaic_render_footprint: sum, cnt and img of dsss_mosaic_render over the sub-samples (mosaic_scatter_fp_kernel).  The 2^24 rule
 *   counts sub-samples; DSSS_E_CAPACITY as there.
 * dsss_mosaic_composite_footprint: the layers and info of dsss_mosaic_composite over the sub-samples (mosaic_composite_fp_kernel).  A
 *   sub-sample competes with its parent's key (q, g, col) and carries its parent's value and source (frame, ping, col); several
 *   sub-samples of one parent in a cell are one key and one value, so the winner stays unique and order-free.  V0 = the cells that hold
 *   a sub-sample; fill and the gap fill work on that V0 unchanged.
 * Consequences: with max_steps == 1 both entries equal dsss_mosaic_render / dsss_mosaic_composite bit for bit in every layer; for any
 *   parameters cnt of the footprint render >= cnt of the point render in every cell.
 * Out of scope: dsss_mosaic_consistency and every registration entry keep point samples (their mean layers are defined on one another,
 *   and a footprint would change the ZNCC tables); the strip between port index 1 and starboard index 0, the nadir, where a frame holds
 *   no sample, is not covered; values are not blended between pings (the value is the parent's, so the composite's source layers stay
 *   true); the extrapolated step of a frame's last ping may reach beyond dsss_mosaic_bounds: such sub-samples are off the grid and are
 *   dropped.
 * Errors.  DSSS_E_ARG, before anything is reserved, cleared or launched: whatever the point entry refuses (a gain table of another M
 *   included), max_steps outside 1..8, max_gap not finite or <= 0, a listed frame whose M is odd or below 4 (both entries: the across
 *   step needs index half - 2); for the host function a NULL pointer, a cell <= 0 or not finite, parameters out of range.  DSSS_E_STATE
 *   as dsss_mosaic_render.  Every error leaves the context usable and a gain table that was set in place.                            */
typedef struct { int32_t max_steps, pad_; double max_gap; } dsss_footprint_params;      /* defaults 4, 1.0: not tuned on any data */
void dsss_footprint_params_default(dsss_footprint_params*);
/* pure host arithmetic, no context: the step count n(S), the one body the kernels run */
int  dsss_mosaic_footprint_steps(const dsss_footprint_params*, double cell, double sx, double sy, int32_t* n);
int  dsss_mosaic_render_footprint(dsss_ctx*, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params*,
                                  const dsss_footprint_params* /* NULL: defaults */, uint32_t* sum_host, uint32_t* cnt_host, uint8_t* img_host);
int  dsss_mosaic_composite_footprint(dsss_ctx*, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params*,
                                     const dsss_comp_params* /* NULL: defaults */, const dsss_footprint_params* /* NULL: defaults */,
                                     uint8_t* img_host, int32_t* src_frame_host, int32_t* src_ping_host, int32_t* src_col_host,
                                     uint8_t* fill_host, dsss_comp_info* info_host);

/* ---- overlap registration: how far, in metres and in which direction, frame b lies from where its overlap with frame a says it belongs.
 * An independent, metric, per-pair measure of a trajectory (the consistency score has no unit of length, the edge report measures the
 * loop closures against the trajectory they produced).  All quantities are integers up to the final score, so results do not depend on
 * the order of frames, pairs, tiles or atomics and are identical from call to call.
 * Mean layer: for a frame f under the given trajectory and grid, cnt_f, sum_f and m_f = (sum_f + cnt_f / 2) / cnt_f are exactly those
 *   of dsss_mosaic_consistency (same binning, same mask rule).  A cell is valid for f iff cnt_f > 0; cells outside the grid are invalid.
 * Shift sums: for a pair (a, b) and a shift (dx, dy), |dx|, |dy| <= radius, V = the grid cells (ix, iy) where a is valid at (ix, iy) and
 *   b is valid at (ix + dx, iy + dy).  Six uint64 sums over V, in this order: n = |V|, Sa = sum m_a, Sb = sum m_b, Sab = sum m_a m_b,
 *   Saa = sum m_a^2, Sbb = sum m_b^2, with m_b taken at the shifted cell.  Shifts are ordered dy-major: index
 *   (dy + radius) (2 radius + 1) + (dx + radius).
 * Score: num = n Sab - Sa Sb, da = n Saa - Sa^2, db = n Sbb - Sb^2 are evaluated exactly in integers (128 bit), each converted ONCE to
 *   the nearest double (ties to even), and zncc = num / sqrt(da db) in f64.  A shift is usable iff n >= min_cells, da > 0 and db > 0;
 *   zncc = -2 otherwise.
 * Peak: the usable shift with the largest zncc; ties go to the smallest dx^2 + dy^2, then the smallest dy, then the smallest dx.  No
 *   usable shift: dx = dy = 0, zncc = -2, n = n0, offsets 0, on_border = 0.
 * Sub-cell offset: per axis a parabola through the peak and its two neighbours on that axis, p = 0.5 (z- - z+) / (z- - 2 z0 + z+)
 *   (evaluated left to right in f64); p = 0 on both axes when the peak is on the border of the search square, and on an axis where a
 *   neighbour is not usable or the denominator is not below 0.  off = ((dx + px) cell, (dy + py) cell) in metres.                    */
typedef struct { int32_t radius, min_cells; } dsss_reg_params;            /* radius 0..16 cells; default 8, 256 */
typedef struct { int32_t dx, dy; double off_x, off_y;                     /* peak in cells, offset in metres (sub-cell) */
                 double zncc, zncc0; int64_t n, n0;                       /* at the peak / at zero shift */
                 int32_t on_border, pad_; } dsss_reg_result;              /* 1: peak at |dx| or |dy| == radius, the true offset may lie beyond */
void dsss_reg_params_default(dsss_reg_params*);
/* ids, rpy6, ping_off, the grid and the state rules are those of dsss_mosaic_consistency; pair_a[k], pair_b[k] are frame ids that both
 * occur in ids; the parameters may be NULL (the defaults).  sums_host: npairs x (2 radius + 1)^2 x 6, may be NULL.
 * DSSS_E_ARG: a pair member not in ids, a == b, radius outside 0..16, min_cells < 1, npairs < 0, out_host NULL with npairs > 0
 * (npairs == 0 is valid).  DSSS_E_STATE: frames not extracted, or a communicator of more than one rank.  DSSS_E_CAPACITY: a cell
 * received more than 2^24 samples of one frame.  The results are those of dsss_mosaic_register_peak on the pair's table.            */
int  dsss_mosaic_register(dsss_ctx*, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params*,
                          const int* pair_a, const int* pair_b, int npairs, const dsss_reg_params*,
                          dsss_reg_result* out_host /* npairs */, uint64_t* sums_host /* npairs x (2r+1)^2 x 6, may be NULL */);
/* pure host arithmetic, no context (as dsss_mosaic_grid): the score, peak, tie and sub-cell rules on a table of (2 radius + 1)^2 x 6
 * sums.  DSSS_E_ARG: a NULL pointer, radius outside 0..16, min_cells < 1, cell <= 0 or not finite                                   */
int  dsss_mosaic_register_peak(const uint64_t* sums, int radius, int min_cells, double cell, dsss_reg_result* out);

/* ---- dense loop closures: the registration by SEGMENTS of frame b, and a segment's offset as a pose-graph edge.  One offset per pair
 * of frames is too coarse for a drift that changes along the track; a segment of some tens of pings gives one offset per stretch of it.
 * Segments: for pair k, frame b = pair_b[k] with N_b pings is cut into ceil(N_b / seg_pings) segments [s seg_pings, min((s + 1) seg_pings, N_b)).
 * Segment layer: cnt, sum, m = (sum + cnt / 2) / cnt and validity as defined above, from the samples of that segment's pings only.
 * Table: the six shift sums of (whole frame a, segment of b), as defined above.  Record: r is what dsss_mosaic_register_peak returns
 *   on that table.  Order: rows by pair, then by segment; *nseg_host is their number.
 * Centroid sums: V = the grid cells (ix, iy) where a is valid and the segment is valid at (ix + dx, iy + dy), for the peak (dx, dy);
 *   sx = sum of ix, sy = sum of iy over V, so |V| = r.n.  Both are 0 when no shift is usable.
 * Everything is an integer up to the score: results do not depend on the order of pairs, segments, tiles or atomics and are identical
 * from call to call.  The segment layers of a frame are rendered once per call, however many pairs name it as b.
 * DSSS_E_ARG: seg_pings < 1, nseg_host NULL, cap < 0.  DSSS_E_CAPACITY: cap below the number of rows, decided before anything is
 * launched (*nseg_host holds the number then, too: a call with cap = 0 asks for it).  DSSS_E_NUMERIC: the centroid's cell count differs from r.n (an internal error).  Every other rule (frames, pairs, radius,
 * state, single rank, 2^24 samples) is that of dsss_mosaic_register.                                                                  */
typedef struct { int32_t pair, seg, p0, p1;      /* index into pair_a / pair_b; segment number; pings [p0, p1) of frame pair_b[pair] */
                 dsss_reg_result r;              /* exactly the record dsss_mosaic_register_peak gives for this segment's table */
                 int64_t sx, sy; } dsss_reg_seg; /* sum of ix, sum of iy over V at the peak shift (0, 0 when no shift is usable) */
int  dsss_mosaic_register_segments(dsss_ctx*, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params*,
                                   const int* pair_a, const int* pair_b, int npairs, int seg_pings, const dsss_reg_params*,
                                   dsss_reg_seg* out_host, int cap, int* nseg_host, uint64_t* sums_host /* nseg x (2r+1)^2 x 6, may be NULL */);
/* From a segment result to a pose-graph edge: pure host arithmetic, no context.  rows_a (Na x 6), rows_b (Nb x 6) are the "r p y x y z"
 * rows of the two frames under the trajectory that was registered, base_a / base_b the pose-graph index of each frame's first ping.
 * Accepted iff r.zncc >= min_zncc and r.on_border == 0 (no usable peak has zncc -2).
 * Overlap centre: c = (x0 + (sx / n + 0.5) cell, y0 + (sy / n + 0.5) cell), in f64 in exactly this order, n = r.n.
 * Anchor pings, the pings whose scan line passes nearest the overlap centre: i = argmin over [0, Na) of
 *   |cos(yaw_i) (c_x - x_i) + sin(yaw_i) (c_y - y_i)|, j the same over [p0, p1) of b with the point c + (off_x, off_y), because b's
 *   rendering lies off from where it belongs; ties go to the lowest index.
 * Measurement: X_a = Pose3(Rot3::Rodrigues(r, p, y), (x, y, z)) of rows_a[i], X_b' the same of rows_b[j] with its translation moved
 *   by (-off_x, -off_y, 0).  With ga = base_a + i and gb = base_b + j: ga < gb gives the edge (ga, gb, X_a^-1 X_b'), otherwise
 *   (gb, ga, X_b'^-1 X_a).
 * Variance: (s_rot^2, s_rot^2, s_rot^2, s_xy^2, s_xy^2, s_z^2) with s_xy = sigma_xy_cells cell: rotation and height are measured
 *   weakly at their current values, the registration says nothing about them.
 * Defaults: min_zncc 0.5, sigma_xy_cells 1 (one cell is the quantisation of the search), sigma_z 10 m, sigma_rot 1 rad: the values
 *   of a feasibility check on a synthetic survey, NONE of them tuned on real data.
 * Returns 1 and fills *edge when the segment is accepted, 0 when it is rejected, DSSS_E_ARG for a NULL pointer (the parameters may be
 * NULL: the defaults), Na or Nb < 1, pings outside 0 <= p0 < p1 <= Nb, a cell or a sigma that is not positive and finite, an accepted
 * peak with n <= 0, a pose-graph index outside int32.                                                                               */
typedef struct { double min_zncc, sigma_xy_cells, sigma_z, sigma_rot; } dsss_reg_edge_params;   /* defaults 0.5, 1.0, 10.0 (m), 1.0 (rad) */
void dsss_reg_edge_params_default(dsss_reg_edge_params*);
int  dsss_register_edge(const dsss_reg_seg* s, const dsss_mosaic_params* grid, const double* rows_a, int Na, int base_a,
                        const double* rows_b, int Nb, int base_b, const dsss_reg_edge_params*, dsss_lc_edge* edge);
/* dsss_register_edge on every row of segs, in order; it launches no GPU work.  The rows are the caller's trajectory (rpy6, ping_off as
 * above), the frames' own pose6 when rpy6 == NULL; base is ping_off[i], or, when ping_off == NULL, the running sum of N over ids in
 * order.  segs[k].pair indexes pair_a / pair_b as it did in dsss_mosaic_register_segments.  edge_seg_host[e] (may be NULL) is the row
 * edge e came from.  Frames need their geometry only.  DSSS_E_CAPACITY: more accepted rows than cap.  DSSS_E_STATE: a communicator of
 * more than one rank.  DSSS_E_ARG: what dsss_register_edge refuses, a pair member not in ids, a negative pair index.                 */
int  dsss_mosaic_register_edges(dsss_ctx*, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params*,
                                const int* pair_a, const int* pair_b, const dsss_reg_seg* segs, int nsegs, const dsss_reg_edge_params*,
                                dsss_lc_edge* edges_host, int32_t* edge_seg_host /* may be NULL */, int cap, int* n_edges);

/* ---- dense loop closures with a yaw fan: the segments registered under a fan of small rotations as well, so that an edge measures
 * the heading too.  Dead reckoning accumulates heading error, and a segment rendered under the wrong heading correlates badly at
 * every shift; the closures above slide a segment in x and y only and say nothing about yaw (sigma_rot = 1 rad).
 * Fan: nyaw angles, nyaw odd and in 1..17, theta_k = (k - mid) step with mid = (nyaw - 1) / 2, k = 0 .. nyaw - 1 (the integer k - mid
 *   converted to f64, times step); step > 0 and finite, in radians.  Defaults: nyaw 1 (the registration above), step 0.01 rad -- a
 *   value that has NOT been tuned on any data.
 * Rotated rows: the pings [p0, p1) of rows_b turned by theta about the position of ping pm = (p0 + p1) / 2, (cx, cy) = (rows_b[pm][3],
 *   rows_b[pm][4]).  (s, c) = the library's deterministic sin / cos of theta (Cody-Waite reduction, fdlibm polynomials, plain IEEE
 *   multiplies and adds: the oracle's orc_sincos bit for bit).  Per ping, in f64, in exactly this order and unfused:
 *   dx = x - cx, dy = y - cy, x' = cx + (c dx - s dy), y' = cy + (s dx + c dy), yaw' = yaw + theta; r, p and z are unchanged.
 *   theta == 0 copies the rows unchanged (NOT cx + (x - cx)).
 * Fan registration: for every (pair, segment, k) the segment layer is the one defined above, rendered under the segment's rows rotated
 *   by theta_k; its table and its record are those defined above (dsss_mosaic_register_peak).
 * Angle rule (dsss_register_yaw_peak): a record is usable iff its zncc > -2.  k* = the usable record with the largest zncc; ties go to
 *   the smallest |k - mid|, then to the lowest k.  yaw_on_border = (nyaw > 1 and (k* == 0 or k* == nyaw - 1)).  theta = theta_{k*},
 *   theta_hat = theta + q step with q = 0.5 (z- - z+) / (z- - 2 z0 + z+) (left to right in f64) on the peak znccs of k* - 1, k*, k* + 1;
 *   q = 0 on the border, when a neighbour is not usable or when the denominator is not below 0.  No usable record: k* = mid,
 *   yaw_on_border = 0, theta = theta_hat = 0.
 * Row: s = the (pair, segment) row above with the record and the centroid sums of angle k*, k = k*, zncc_k0 = the peak zncc of the
 *   unrotated angle (k = mid; -2 when it has no usable shift).  With nyaw == 1 every s equals dsss_mosaic_register_segments' row bit
 *   for bit.  Order of rows as above.  sums_host (may be NULL): nseg x nyaw x (2 radius + 1)^2 x 6.
 * Everything is an integer up to the scores.  A frame that is a b is rendered once per call for all its segments and angles.
 * Errors: those of dsss_mosaic_register_segments, and DSSS_E_ARG for a fan outside the rules above (the fan may be NULL: the
 * default) or for frames of more than 2^31 / nyaw pings.  Every argument and capacity error is decided before anything is launched. */
typedef struct { int32_t nyaw; int32_t pad_; double step; } dsss_reg_yaw_params;      /* defaults 1, 0.01 rad (untuned) */
typedef struct { dsss_reg_seg s;                      /* the row of angle k* */
                 int32_t k, yaw_on_border;            /* k*; 1: the best angle is the first or the last of the fan, the true one may lie beyond */
                 double theta, theta_hat, zncc_k0; } dsss_reg_seg_yaw;
void dsss_reg_yaw_params_default(dsss_reg_yaw_params*);
/* pure host arithmetic, no context: out = (p1 - p0) x 6.  DSSS_E_ARG: a NULL pointer, pings outside 0 <= p0 < p1 <= Nb, theta not finite */
int  dsss_register_rotate_rows(const double* rows_b, int Nb, int p0, int p1, double theta, double* out);
/* pure host arithmetic, no context: the angle rule on the nyaw records of one (pair, segment).  DSSS_E_ARG: a NULL pointer, a fan
 * outside the rules above                                                                                                       */
int  dsss_register_yaw_peak(const dsss_reg_result* per_angle, int nyaw, double step, int32_t* k, int32_t* yaw_on_border,
                            double* theta, double* theta_hat);
int  dsss_mosaic_register_segments_yaw(dsss_ctx*, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params*,
                                       const int* pair_a, const int* pair_b, int npairs, int seg_pings, const dsss_reg_params*,
                                       const dsss_reg_yaw_params*, dsss_reg_seg_yaw* out_host, int cap, int* nseg_host,
                                       uint64_t* sums_host /* nseg x nyaw x (2r+1)^2 x 6, may be NULL */);
/* From a fan row to a pose-graph edge that measures the heading: dsss_register_edge with these changes.
 * Accepted iff dsss_register_edge accepts s AND yaw_on_border == 0.  Overlap centre c and anchor ping i of a: as above.
 * Anchor ping j of the segment: the same rule on the rows [p0, p1) of b rotated by theta (theta_{k*}: the rows the chosen layer was
 *   rendered under) and the point c + (off_x, off_y).
 * Measurement: X_b' = the Rodrigues pose of row j of the rows rotated by theta_hat, its translation moved by (-off_x, -off_y, 0); the
 *   direction rule is unchanged.
 * Variance: (s_rot^2, s_rot^2, s_yaw^2, s_xy^2, s_xy^2, s_z^2) with s_yaw = sigma_yaw_steps step (default one step: the quantisation of
 *   the search, as one cell is for x and y).  With fan.nyaw == 1, s_yaw = s_rot and the edge equals dsss_register_edge's bit for bit.
 * fan = the fan the rows were registered with.  DSSS_E_ARG: what dsss_register_edge refuses, a fan outside the rules, sigma_yaw_steps
 * not positive and finite, theta or theta_hat not finite.                                                                       */
typedef struct { dsss_reg_edge_params e; dsss_reg_yaw_params fan; double sigma_yaw_steps; } dsss_reg_edge_yaw_params;   /* defaults: e's, the fan's, 1.0 */
void dsss_reg_edge_yaw_params_default(dsss_reg_edge_yaw_params*);
int  dsss_register_edge_yaw(const dsss_reg_seg_yaw* s, const dsss_mosaic_params* grid, const double* rows_a, int Na, int base_a,
                            const double* rows_b, int Nb, int base_b, const dsss_reg_edge_yaw_params*, dsss_lc_edge* edge);
/* dsss_register_edge_yaw on every row of segs, in order; it launches no GPU work.  Everything else as dsss_mosaic_register_edges. */
int  dsss_mosaic_register_edges_yaw(dsss_ctx*, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params*,
                                    const int* pair_a, const int* pair_b, const dsss_reg_seg_yaw* segs, int nsegs,
                                    const dsss_reg_edge_yaw_params*, dsss_lc_edge* edges_host, int32_t* edge_seg_host /* may be NULL */,
                                    int cap, int* n_edges);

/* ---- dense loop closures over a cell pyramid: the segments registered coarse to fine, so that the capture range is no longer the
 * radius.  A flat search reaches radius <= 16 cells and its table grows with radius^2; a survey under dead reckoning drifts by metres.
 * With L levels the top level, with cells of 2^(L-1) cell, searches the full radius and every level below refines within `refine`
 * cells around twice the shift found above: about 2^(L-1) radius fine cells are reached.
 * Parameters: levels L in 1..4, refine in 1..16 (ignored when L == 1).  Defaults: levels 1 (the registration by segments above),
 *   refine 3 -- a value that has NOT been tuned on any data.
 * Pooled layers: level l has cells of cell_l = cell 2^l (exact), W_l = ceil(W / 2^l), H_l = ceil(H / 2^l).  For a frame or a segment with
 *   the level-0 accumulators cnt, sum defined above: cnt_l(jx, jy) = the sum of cnt over the grid cells with ix >> l == jx and
 *   iy >> l == jy, sum_l the same of sum.  The cell is valid iff cnt_l > 0, and m = (sum_l + cnt_l / 2) / cnt_l in integers.  Level 0 is
 *   the mean layer above bit for bit.  The only capacity rule is level 0's (2^24 samples per fine cell); pooled counts and sums are
 *   kept in 64 bits and cannot wrap.  The definition is the pooling: it differs from a render under the coarse grid only in samples
 *   beyond W, H, which stay dropped.
 * Search, per (pair, segment) row, for l = L-1 down to 0: the centre (cx_l, cy_l) is (0, 0) at the top; the radius r_l is reg.radius
 *   at the top and refine below; min_cells_l = max(1, min_cells >> 2l).  The table T_l holds the six shift sums between whole a and
 *   the segment, both pooled to level l, for the shifts (cx_l + dx, cy_l + dy), |dx|, |dy| <= r_l, stored dy-major by the relative
 *   (dx, dy) as above.  rec_l = dsss_mosaic_register_peak(T_l, r_l, min_cells_l, cell_l).  rec_l.zncc == -2: the search of this row
 *   stops.  Otherwise t_l = (cx_l + rec_l.dx, cy_l + rec_l.dy), bit l of border_mask is set iff rec_l.on_border, and for l > 0 the
 *   next centre is (cx_{l-1}, cy_{l-1}) = 2 t_l.
 * Row: level = the finest level with a usable peak, -1 for none.  lx[l], ly[l] = t_l and lz[l] = the peak zncc of level l; levels not
 *   reached or without a usable peak hold 0, 0, -2.  s.pair, seg, p0, p1 as in dsss_mosaic_register_segments.  s.r = rec_level with
 *   dx, dy replaced by t_level, off_x = rec.off_x + (double)cx cell_level (one multiply and one add, unfused; the same in y; a centre
 *   of 0 leaves rec's offset as it is), zncc0 and n0 those of the table's centre shift, and on_border = (border_mask != 0 or
 *   level != 0): dsss_register_edge rejects every row that did not finish at level 0 or that touched a border on the way.  With
 *   level == -1, s.r is the top level's no-usable-shift record unchanged.  s.sx, s.sy = the centroid sums at the total shift t_0 when
 *   level == 0, and 0 otherwise.  With levels == 1 every s equals dsss_mosaic_register_segments' row of the same call bit for bit,
 *   and border_mask == s.r.on_border.
 * sums_host (may be NULL): per row (2 radius + 1)^2 x 6 sums of the top level, then (2 refine + 1)^2 x 6 for each of the levels
 *   L-2 .. 0; the tables of levels not reached are zero.
 * Everything is an integer up to the scores.  A frame is rendered once per call, its layers of all levels built in one pass.
 * Errors: those of dsss_mosaic_register_segments, and DSSS_E_ARG for levels or refine outside the rules (the parameters may be NULL:
 * the default).  Every argument and capacity error is decided before anything is launched.  The whole frame as one segment is
 * seg_pings >= N_b.                                                                                                              */
typedef struct { int32_t levels, refine; } dsss_reg_pyr_params;                        /* defaults 1, 3 (untuned) */
typedef struct { dsss_reg_seg s;                      /* the row of the finest level with a usable peak */
                 int32_t level, border_mask;          /* that level (-1: none); bit l: the peak of level l lay on the border of its square */
                 int32_t lx[4], ly[4]; double lz[4]; } dsss_reg_seg_pyr;   /* t_l and the peak zncc of level l (0, 0, -2: not reached, or no usable peak) */
void dsss_reg_pyr_params_default(dsss_reg_pyr_params*);
/* pure host arithmetic, no context: the level rule on ONE table, T_level around the centre (cx, cy).  min_cells and cell are the
 * level-0 values.  *usable = 1: out = rec with the centre added as defined above (out->on_border is rec's), and for level > 0
 * (*ncx, *ncy) = the next level's centre 2 t.  *usable = 0: out = the no-usable-shift record unchanged, *ncx, *ncy are not written.
 * DSSS_E_ARG: a NULL pointer, radius outside 0..16, min_cells < 1, cell <= 0 or not finite, level outside 0..3, |cx| or |cy| > 2^28 */
int  dsss_register_pyr_step(const uint64_t* sums, int radius, int min_cells, double cell, int level, int cx, int cy,
                            dsss_reg_result* out, int32_t* usable, int32_t* ncx, int32_t* ncy);
int  dsss_mosaic_register_segments_pyr(dsss_ctx*, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params*,
                                       const int* pair_a, const int* pair_b, int npairs, int seg_pings, const dsss_reg_params*,
                                       const dsss_reg_pyr_params*, dsss_reg_seg_pyr* out_host, int cap, int* nseg_host,
                                       uint64_t* sums_host /* nseg x ((2r+1)^2 + (levels-1) (2 refine+1)^2) x 6, may be NULL */);

/* ---- peaks on the device.  The peak rule is a pure function of a table's integer sums, so it is evaluated where the table lies:
 * mosaic_peak_kernel turns every table into its 64-byte record on the device, and the four registration entries above download records
 * instead of tables whenever the caller did not ask for the sums (sums_host == NULL).  The records are bit for bit those of
 * dsss_mosaic_register_peak: one body of the score, order and parabola rules is compiled for host and device, and everything in it is
 * an IEEE-754 basic operation.  With sums_host the table comes down anyway and the host decides, as before.  The environment switch
 * DSSS_REG_PEAKS=host, read once per call, forces that path without sums_host (an A/B switch; any other value: the rule above).   */
/* dsss_mosaic_register_peak's rules on ntables tables at once, on the device.
 * sums: ntables x (2 radius + 1)^2 x 6, host or device memory.
 * out_host[k] is bit for bit the record dsss_mosaic_register_peak gives for table k (pad_ = 0).
 * ntables == 0 is valid and launches nothing. Any rank may call it (no frames involved).
 * DSSS_E_ARG, decided before anything is launched: NULL sums or out_host with ntables > 0,
 * ntables < 0, radius outside 0..16, min_cells < 1, cell <= 0 or not finite.            */
int  dsss_mosaic_register_peaks(dsss_ctx*, const uint64_t* sums, int64_t ntables, int radius,
                                int min_cells, double cell, dsss_reg_result* out_host);
typedef struct { int64_t tables_device, tables_host, bytes_down, syncs; } dsss_reg_call_info;
/* the last dsss_mosaic_register* / dsss_mosaic_register_peaks call of this context that returned DSSS_OK:
 * tables scored by mosaic_peak_kernel / by the host; bytes the call copied device -> host;
 * stream synchronisations it made. Zeros before any such call.  Counted from the sizes of the copies the call enqueues and from
 * the synchronisations written in the entry, not measured (a synchronisation that a growing buffer makes is not among them).
 * DSSS_E_ARG: a NULL pointer.                                                                                                 */
int  dsss_mosaic_register_info(const dsss_ctx*, dsss_reg_call_info* out);

/* ------------------------------------------------------------------ instrumentation
 * accumulated GPU time (ms, HIP events on the context stream) and launch count per kernel family        */
#define DSSS_K_ROW_REDUCE   0   /* row_reduce_kernel: one f64 read of the waterfall */
#define DSSS_K_PRE_MISC     1   /* final_reduce + mask_init */
#define DSSS_K_NORMALIZE    2   /* normalize_kernel: f64 read, u8 write, hot-pixel scatter */
#define DSSS_K_PYRAMID      3   /* resize_kernel x (nlevels-1) */
#define DSSS_K_FAST         4   /* fast_cells_kernel */
#define DSSS_K_FAST_COMPACT 5   /* scan + gather of candidates */
#define DSSS_K_DESC         6   /* orient_desc_kernel */
#define DSSS_K_FILTER       7   /* mask_filter_kernel */
#define DSSS_K_MATCH        8   /* mt_grid_build_kernel + match_grid_kernel (or match_nn_kernel, all pairs) */
#define DSSS_K_SCC          9   /* scc_kernel */
#define DSSS_K_ROWS        10   /* pair_rows count/scan/write */
#define DSSS_K_LC          11   /* lc_kernel */
#define DSSS_K_PG          12   /* pose-graph LM loop (all its kernels) */
#define DSSS_K_QUADTREE    13   /* quadtree_kernel + collect (K4 on the device) */
#define DSSS_K_PG_ACC      14   /* pg_front_syrk_kernel (trailing update of the fronts: the bulk of the factorisation flops) */
#define DSSS_K_PG_DIAG     15   /* pg_front_diag_kernel */
#define DSSS_K_PG_TRSM     16   /* pg_front_trsm_kernel */
#define DSSS_K_PG_BWD      17   /* pg_front_bwd_kernel */
#define DSSS_K_PG_SUBTREE  18   /* pg_factor_subtree_kernel + pg_bwd_subtree_kernel */
#define DSSS_K_PG_ASM      19   /* pg_front_asm_kernel (extend-add) */
#define DSSS_K_PG_COMM     20   /* the reduced-Hessian all-reduce of a trial (work = bytes) */
#define DSSS_K_PG_RSU      21   /* pg_front_rsu_kernel: row solve + trailing update fused per tile (the levels with few tiles) */
#define DSSS_K_MATCH_DONE 22   /* no kernel of its own: work = the gate evaluations the matcher actually performed (its geo grid skips the cells out of reach; DSSS_K_MATCH's work is the reference's Na x Nb) */
#define DSSS_K_SIFT       23   /* sift_desc_kernel (DSSS_DESC_SIFT128): work = bytes of the 71 x 71 raw windows read + the 128-byte rows written */
#define DSSS_K_COUNT       24
int dsss_profile_enable(dsss_ctx*, int on);
int dsss_profile_get(dsss_ctx*, double* ms_host /*DSSS_K_COUNT*/, int64_t* launches_host /*DSSS_K_COUNT*/);
int dsss_profile_reset(dsss_ctx*);
/* algorithmic work accumulated next to the time of each slot while profiling is on: bytes for the streaming kernels
 * (slots 0..13), f64 flops for the pose-graph factorisation kernels (slots 14..18); definitions in DESIGN.md section 4 */
int dsss_profile_get_work(dsss_ctx*, double* work_host /*DSSS_K_COUNT*/);

#ifdef __cplusplus
}
#endif
#endif /* DSSS_H */

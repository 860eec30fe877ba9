/* include/dsss_profile.h -- per-ping disagreement profile: every ping of a frame held against the mosaic of all OTHER frames.
 *
 * dsss_mosaic_consistency says where on the seabed overlapping frames disagree, per cell.  The profile says when along the track:
 * which frames, which pings and which side (port or starboard) do not fit the rest of the map.  It is the one mosaic entry that reads
 * the map back at a frame's samples (a gather); every other one is a forward scatter.
 *
 * DEFINITION.  Take the frames `ids` under a trajectory on a grid, point samples, with the range-gain table in force: everything as
 * dsss_mosaic_render takes and bins them.
 *   A[cell] = (S, C): sum and count over all listed frames -- exactly the render's accumulators.
 *   A_f[cell] = (S_f, C_f): the contribution of frame f alone.
 *   A sample of f is BINNED iff the render bins it: the mask rule holds, the point is finite, and it lies on the grid.
 *   A binned sample with corrected value v' in cell g is COMPARED iff C[g] - C_f[g] >= min_count.
 *   For a compared sample m = ((S - S_f) + (C - C_f) / 2) / (C - C_f) with floor division -- the mean mosaic of the other frames in
 *   that cell, rounded as the render rounds -- and d = v' - m, in -255 .. 255.
 *   Per ping and per side (side 0, port: col < M / 2; side 1, starboard: the rest) the record dsss_ping_stat holds
 *     binned = the binned samples, n = the compared samples, sad = sum |d|, ssd = sum d^2, sd = sum d (signed).
 *   sad and ssd are u32 and sd is i32: a side has at most 32768 samples (a profiled frame has at most 65536 columns, DSSS_E_ARG
 *   otherwise) and 255^2 * 32768 < 2^32.
 *   The optional residual waterfall of a profiled frame is int16, N x M: d where the sample is compared, DSSS_PROFILE_NONE elsewhere.
 *   min_count is at least 1 and at most 2^24; the default is 1.
 *
 * Why this is exact.  The accumulators are integers, count << 32 | sum per cell.  The frame's sum and count are each at most the
 * map's, so A - A_f is ONE 64-bit subtraction that cannot borrow across the words, and "the mosaic of all other frames" is exact
 * whatever the order of the frames.  Everything here is integer work and the same from call to call, byte for byte.
 *
 * Outputs.  stats_host holds the pings of the profiled frames one frame after the other, in the order of `prof` (of `ids` for the
 * canvas); diff_host holds their N_i x M_i layers in the same order; info sums the call's records.  Each of the three may be NULL.
 *
 * dsss_profile_mosaic.  Argument rules and their precedence are those of dsss_mosaic_render.  Behind them, DSSS_E_ARG before
 *   anything is launched: nprof < 1 with a list given, a prof index outside [0, n), a prof index listed twice, min_count outside
 *   1 .. 2^24, a profiled frame of more than 65536 columns.  prof == NULL profiles all listed frames in the order of ids (nprof is
 *   not read).  DSSS_E_CAPACITY follows the render's rule: a cell over 2^24 samples.  A single listed frame is legal: it has nothing
 *   to compare against, every n is 0 and every diff is DSSS_PROFILE_NONE.
 * dsss_profile_canvas.  Runs on a point canvas (include/dsss_canvas.h); a footprint canvas is DSSS_E_ARG -- profiling under footprints
 *   is out of scope: a frame's own sub-samples would have to be taken out of the map per sub-sample.  ids must be distinct and all on
 *   the canvas (DSSS_E_ARG); the staleness rules of dsss_canvas_remove apply (DSSS_E_STATE); a broken canvas answers DSSS_E_STATE.
 *   It uses the canvas's device copy of each frame's stored rows and the canvas's accumulators as A: no frame outside ids is
 *   scattered.  It changes neither the canvas, nor its set of frames, nor the dirty window.
 *   INVARIANT: its outputs are byte for byte those of dsss_profile_mosaic over the frames on the canvas (ascending) under their
 *   stored rows on the canvas's grid with prof = ids.
 * Single rank, one thread per context, as for every mosaic entry.  Both entries return with the stream synchronised.               */
#ifndef DSSS_PROFILE_H
#define DSSS_PROFILE_H
#include "dsss.h"
#include "dsss_canvas.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DSSS_PROFILE_NONE (-32768)          /* a sample of the residual waterfall that is not compared */
#define DSSS_PROFILE_MAX_MIN_COUNT (1 << 24)
#define DSSS_PROFILE_MAX_M 65536

typedef struct { uint32_t binned[2], n[2], sad[2], ssd[2]; int32_t sd[2]; } dsss_ping_stat;     /* 40 bytes; [0] port, [1] starboard */
typedef struct { int32_t min_count, pad_; } dsss_profile_params;                                  /* default 1 */
typedef struct { int64_t pings, binned, n, sad, ssd, sd; double rms; } dsss_profile_info;         /* over the call; rms = n ? sqrt((double)ssd / (double)n) : 0 */

void dsss_profile_params_default(dsss_profile_params*);
int  dsss_profile_summary(const dsss_ping_stat* stats, int64_t npings, dsss_profile_info* info);   /* pure host arithmetic, no context; npings = 0 is legal */
int  dsss_profile_mosaic(dsss_ctx*, const int* ids, int n, const double* rpy6, const int* ping_off, const dsss_mosaic_params*,
                         const int* prof /* indices into ids, distinct; NULL: all, in order */, int nprof, const dsss_profile_params* /* NULL: defaults */,
                         dsss_ping_stat* stats_host, int16_t* diff_host, dsss_profile_info* info);
int  dsss_profile_canvas(dsss_canvas*, const int* ids, int n, const dsss_profile_params* /* NULL: defaults */,
                         dsss_ping_stat* stats_host, int16_t* diff_host, dsss_profile_info* info);

#ifdef __cplusplus
}
#endif
#endif

/* include/dsss_canvas.h -- mosaic canvas: a mean mosaic that stays on the device and takes frames in, moves them and takes them out.
 *
 * dsss_mosaic_render / dsss_mosaic_render_footprint build a mosaic from nothing: every frame is scattered again, whatever changed.
 * The online solver (dsss_posegraph_update_window) moves the last W frames of a survey per arriving frame and hands the rest back bit
 * for bit, so the mosaic under the new trajectory differs from the old one by those W frames alone.  A canvas keeps the accumulators of
 * ONE grid on the device between calls, and the set S of frames on it, each with the pose rows it was put with.
 *
 * Why this is exact.  Every accumulator of the mean mosaic is an integer, count << 32 | sum per cell, filled by 64-bit atomic adds.
 * Adding the two's complement of what a frame added restores the cell bit for bit, so a frame can be taken out again under the rows it
 * was put with.  (The composite mosaic is a minimum per cell and has no inverse: there is no canvas for it.)
 *
 * INVARIANT.  After every call that returns DSSS_OK, and after every refused call, dsss_canvas_read gives bit for bit (sum, cnt, img)
 * what a fresh dsss_mosaic_render (point canvas) or dsss_mosaic_render_footprint (footprint canvas) gives for the frames of S under
 * their stored rows on the same grid with the gain table in force, whatever the history and the order of calls and ids.
 *
 * put.  Rows as dsss_mosaic_render takes them: rpy6 is a host pointer, frame ids[i] from row ping_off[i]; NULL: the poses the frame was
 *   set with.  A frame not in S is ADDED.  A frame in S whose new rows are bytewise equal to the stored ones (memcmp over N x 6 doubles:
 *   NaN payloads and signed zeros count) is SKIPPED, nothing is launched for it -- so put(all frames, the whole trajectory) after a
 *   windowed update costs the window.  Any other frame of S is MOVED: out under the stored rows, in under the new ones, within the same
 *   launches.  The canvas keeps a host copy and a device copy of every frame's rows; a remove uses the device copy and never reads the
 *   caller's memory again.
 * move.  DSSS_CANVAS_MOVE_SPLIT: a moved frame is a remove job and an add job of the scatter kernel.  DSSS_CANVAS_MOVE_AUTO: on a point
 *   canvas the fused kernel, which bins every sample under both rows and issues nothing for a sample that stays in its cell; on a
 *   footprint canvas the split form.
 * All or nothing.  Arguments and state are checked for the whole call before anything is launched, in this order: the rules of
 *   dsss_mosaic_render on the frames, the footprint rule (a footprint canvas: even M of at least 4), the gain table's M, staleness.
 *   remove of a frame not in S is DSSS_E_ARG.
 * Sample limit.  Launches are cut at 2^31 (sub-)samples; the limit of 2^24 samples per cell is checked over the call's window between
 *   the launches and at the end.  On DSSS_E_CAPACITY the launches issued so far are undone by the same jobs with the signs flipped: the
 *   canvas and S are as before the call.
 * Staleness.  A put or remove that touches a frame that was set or extracted again since it was put is DSSS_E_STATE (its images are no
 *   longer those that were added); so is a put or remove on a non-empty canvas after the gain table changed.  dsss_canvas_clear is
 *   the way out.
 * Windows (win4 = ox, oy, bw, bh in cells; bw = 0: none).  dsss_canvas_frame_window is the window of the cells a frame's geo extremes
 *   can reach under the given rows; for a footprint canvas the metric extent is grown by 2 max_gap on every side first (a step longer
 *   than max_gap has one sub-sample, so a sub-sample lies within (7/8) 2 max_gap per axis of its parent).  put_info.win and the dirty
 *   window are unions of these windows over the old and the new rows.  A read window that leaves the grid is DSSS_E_ARG.
 * A HIP error inside a call leaves the canvas broken: every later call but clear and destroy answers DSSS_E_STATE.
 * Single rank, one thread per context, as for every mosaic entry.  Every call returns with the stream synchronised.               */
#ifndef DSSS_CANVAS_H
#define DSSS_CANVAS_H
#include "dsss.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct dsss_canvas dsss_canvas;
#define DSSS_CANVAS_MOVE_AUTO  0   /* point canvas: fused move; footprint canvas: split */
#define DSSS_CANVAS_MOVE_SPLIT 1   /* a moved frame is a remove job and an add job */
typedef struct { int32_t footprint /* 0: point samples */, move; dsss_footprint_params fp; } dsss_canvas_params;
typedef struct { int32_t added, moved, skipped, pad_; int64_t pings /* workgroups launched */; int32_t win[4] /* ox, oy, bw, bh touched by this call; bw = 0: none */; } dsss_canvas_put_info;

void dsss_canvas_params_default(dsss_canvas_params*);                 /* point samples, AUTO, footprint defaults */
int  dsss_canvas_create(dsss_ctx*, const dsss_mosaic_params* grid, const dsss_canvas_params* /* NULL: defaults */, dsss_canvas** out);
int  dsss_canvas_destroy(dsss_canvas*);                              /* dsss_destroy frees what is left */
int  dsss_canvas_put(dsss_canvas*, const int* ids, int n, const double* rpy6, const int* ping_off, dsss_canvas_put_info* /* may be NULL */);
int  dsss_canvas_remove(dsss_canvas*, const int* ids, int n);
int  dsss_canvas_clear(dsss_canvas*);                                 /* S empty, accumulators zero, dirty = whole grid */
int  dsss_canvas_read(dsss_canvas*, const int32_t* win4 /* NULL: the grid */, uint32_t* sum, uint32_t* cnt, uint8_t* img);  /* bw x bh row-major, each may be NULL */
int  dsss_canvas_dirty(dsss_canvas*, int32_t* win4, int reset);      /* bounding window of everything touched since the last reset; bw = 0: nothing */
int  dsss_canvas_frames(const dsss_canvas*, int* ids_host, int cap, int* n);   /* ascending */
int  dsss_canvas_rows(dsss_canvas*, int id, double* rows_host /* N x 6 */);      /* downloaded from the canvas's device copy */
int  dsss_canvas_frame_window(dsss_canvas*, int id, const double* rows /* N x 6 host; NULL: the stored rows */, int32_t* win4);  /* host arithmetic */

#ifdef __cplusplus
}
#endif
#endif

// diasss_amd/csrc/dsss_mosaic_profile.h -- what the two entries of the per-ping profile (include/dsss_profile.h) share: the plan of a
// call.  dsss_profile_mosaic (dsss_mosaic_profile.hip) renders the accumulators A itself; dsss_profile_canvas (dsss_mosaic_canvas.hip,
// beside struct dsss_canvas) hands in the canvas's.  Behind that both are the same launches, so the canvas's invariant holds by
// construction.
#pragma once
#include "dsss_mosaic_int.h"
#include "../../include/dsss_profile.h"

// one profiled frame: its job as mosaic_fill_jobs fills it with the rows it is profiled under (device), and its window of the grid
// (on_grid false: no cell of it lies on the grid; every record of it is zero)
struct profile_frame { mosaic_job job; mosaic_win w; bool on_grid; };

// one job of mosaic_profile_kernel: a mosaic_job, the frame's window of the grid (bw = 0: none), where its own accumulators start in
// the arena of windows (cells), and where its records and its residual layer start in the outputs (pings, samples)
struct prof_job : mosaic_job { int ox = 0, oy = 0, bw = 0, bh = 0; unsigned long long woff = 0, ping0 = 0, diff0 = 0; };

// The plan of a call: frames in the order of the outputs.  take() takes its pieces of mosaic_buf from the caller's arena (before the
// reserve; the windows may follow later), run() cuts the frames into batches whose windows fit the arena, issues the launches behind
// whatever the caller queued on the stream and returns with the stream synchronised.
struct profile_plan {
    std::vector<profile_frame> frames;
    int min_count = 1;
    bool want_stats = false, want_diff = false;                                    // what comes down (info needs the records too)
    size_t pings = 0, samples = 0, arena_cells = 0;
    std::vector<int> batch_end;                                                    // frames [batch_end[b - 1], batch_end[b]) share the arena
    mosaic_piece<unsigned long long> o_win; mosaic_piece<mosaic_job> o_sjobs; mosaic_piece<prof_job> o_pjobs;
    mosaic_piece<dsss_ping_stat> o_stats; mosaic_piece<int16_t> o_diff;
    void take(mosaic_arena& A, size_t grid_cells);                                 // reads N and M of the frames' jobs, nothing else of them
    // acc = the accumulators of all frames on the grid p (device, W x H)
    int run(dsss_ctx* c, const mosaic_arena& A, const dsss_mosaic_params* p, const unsigned long long* acc,
            dsss_ping_stat* stats_host, int16_t* diff_host, dsss_profile_info* info);
};

// the rules the profile adds to a frame and to the parameters; *min_count = the caller's or the default
int profile_check_params(dsss_ctx* c, const dsss_profile_params* pp, int* min_count);
int profile_check_frame(dsss_ctx* c, int id);

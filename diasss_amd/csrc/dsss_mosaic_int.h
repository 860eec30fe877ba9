// diasss_amd/csrc/dsss_mosaic_int.h -- what dsss_mosaic.hip (mosaic, consistency map) and dsss_mosaic_reg.hip (overlap registration)
// share: the job and window records of mosaic_scatter_kernel, the argument checks, a frame's window of the grid, the upload of a
// caller's trajectory and the scatter launch.  The definitions are in dsss_mosaic.hip.
#pragma once
#include "dsss_internal.h"

#define MOSAIC_MAX_CELLS (1ll << 28)
#define MOSAIC_MAX_SAMPLES (1u << 24)      // per cell: 255 * 2^24 < 2^32, the u32 sum cannot wrap below it

// one frame of a launch: its pose rows (the frame's own or the caller's trajectory), geometry and images; blk0 = its first workgroup
struct mosaic_job { const double* pose; const double* gr; const uint8_t* img; const uint8_t* mask; int N, M, blk0, pad; };
// the grid (x0, y0, cell, W, H: where a point falls and whether it is kept) and the window of it the accumulators cover
// (ox, oy, bw, bh: the whole grid for the mosaic, one frame's cell bounding box for the consistency map and the registration)
struct mosaic_win { double x0, y0, cell; int W, H, ox, oy, bw, bh, use_mask; };
// one segment of a frame in the segmented scatter: its window of the grid (bw = 0: no cell of it lies on the grid) and where its
// accumulators start, in cells, behind the frame's first
struct mosaic_seg { int ox, oy, bw, bh; unsigned long long off; };

// The samples of one ping, by the 256 threads of its workgroup (mosaic_scatter_kernel's comment in dsss_mosaic.hip): P = the ping's
// pose row, sc = sin and cos of the bearing of the port and of the starboard side (dsss_geo_side on P, in LDS), row = the ping's row
// in the frame's images, G = grid and window, acc = the window's accumulators.  The one place a sample is binned on the device.
__device__ __forceinline__ void mosaic_scatter_samples(const double* P, const double* sc, const mosaic_job& J, int row, const mosaic_win& G,
                                                       unsigned long long* __restrict__ acc)
{
    const int M = J.M, half = M / 2;
    const uint8_t* __restrict__ img = J.img + (size_t)row * M;
    const uint8_t* __restrict__ mask = J.mask + (size_t)row * M;
    const int lane = threadIdx.x & 63;
    for (int c0 = 0; c0 < M; c0 += 256) {
        const int col = c0 + (int)threadIdx.x;
        int key = -1; unsigned v = 0;                                              // v: count << 16 | sum within the wavefront
        if (col < M && (!G.use_mask || mask[col] != 0)) {
            const int side = col >= half;
            double x, y;
            dsss_geo_bin(P, J.gr, M, col, sc[2 * side], sc[2 * side + 1], &x, &y);
            const double fx = floor((x - G.x0) / G.cell), fy = floor((y - G.y0) / G.cell);
            if (fx >= 0.0 && fx < (double)G.W && fy >= 0.0 && fy < (double)G.H) {  // on the f64 values: NaN, infinite and huge points drop out here
                const int ix = (int)fx - G.ox, iy = (int)fy - G.oy;
                if (ix >= 0 && ix < G.bw && iy >= 0 && iy < G.bh) { key = iy * G.bw + ix; v = (1u << 16) | img[col]; }
            }
        }
        const int prev = __shfl_up(key, 1);
        const bool head = lane == 0 || prev != key;
        const unsigned long long hb = __ballot(head);
        const int start = 63 - __clzll((long long)(hb & (~0ull >> (63 - lane))));   // first lane of this lane's run
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const unsigned t = __shfl_up(v, d); if (lane - d >= start) v += t; }
        const bool tail = lane == 63 || ((hb >> (lane + 1)) & 1ull);
        if (tail && key >= 0) atomicAdd(&acc[key], ((unsigned long long)(v >> 16) << 32) | (v & 0xffffu));
    }
}

// carves mosaic_buf into 256-byte aligned pieces
struct carve { size_t off = 0; size_t take(size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; } };

int mosaic_check_frames(dsss_ctx* c, const int* ids, int n, const double* rpy6, const int* ping_off, bool need_img, size_t* rows);
int mosaic_check_params(dsss_ctx* c, const dsss_mosaic_params* p);
void frame_extent(const dsss_frame& f, const double* rows, double* bb);
void frame_extent_rows(const dsss_frame& f, const double* rows, int r0, int r1, double* bb);      // pings [r0, r1) only
bool cell_range(double lo, double hi, double origin, double cell, int n, int* a, int* b);
int upload_rows(dsss_ctx* c, const int* ids, int n, const double* rpy6, const int* ping_off, double* d_rows, std::vector<const double*>& dev_rows);
void launch_scatter(dsss_ctx* c, const mosaic_job* d_jobs, int njobs, int blocks, const mosaic_win& G, unsigned long long* acc);
// the segmented form for ONE frame (d_job: its record, blk0 = 0; blocks = its pings): ping p goes into d_segs[p / seg_pings]
void launch_scatter_seg(dsss_ctx* c, const mosaic_job* d_job, int blocks, const mosaic_win& G, unsigned long long* acc, const mosaic_seg* d_segs, int seg_pings);

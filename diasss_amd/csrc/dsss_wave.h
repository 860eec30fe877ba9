// diasss_amd/csrc/dsss_wave.h -- the wave scan, the workgroup scan and the wave sum of the kernels (device only, wave64).
// Every caller sits on an order-sensitive path (candidate order, kept keypoints, kp7 offsets, edge order, the normal
// stream, the bit-reproducible mean), so there is one copy of each.  Sums only: the min / max butterflies, the segmented
// scan of the mosaic (mosaic_run_reduce, + or min), the two-step sums of the fronts and the matcher's fold are different code and stay where they are.
#pragma once
#include <hip/hip_runtime.h>

// inclusive scan over the 64 lanes of a wavefront
template <typename T>
__device__ __forceinline__ T dsss_wave_scan_incl(T v)
{
    const int lane = threadIdx.x & 63;
    T inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const T t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
    return inc;
}

// Exclusive scan over a one-dimensional workgroup of WAVES wavefronts; *total receives the sum of all threads, s_w is
// WAVES values of LDS.  Every thread of the workgroup calls it.  The leading barrier protects s_w against the readers of
// the previous call (a scan carried over chunks calls this back to back), so callers need none between two calls.
template <int WAVES, typename T>
__device__ __forceinline__ T dsss_block_scan_excl(T v, T* total, T* s_w)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const T inc = dsss_wave_scan_incl(v);
    __syncthreads();
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    T base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < WAVES; ++k) { const T t = s_w[k]; if (k < w) base += t; tot += t; }
    *total = tot;
    return base + inc - v;
}

// sum over the 64 lanes, every lane receives it.  The butterfly runs from 32 down to 1 with `v += partner`: the f64 sums
// feed bit-exact outputs, so neither the order of the steps nor that of the operands may change.
template <typename T>
__device__ __forceinline__ T dsss_wave_sum(T v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

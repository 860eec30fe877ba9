// diasss_amd/csrc/dsss_match.hip -- batched FEAmatcher on the device (gfx950).
// Restates /root/reference/src/core/FEAmatcher.cpp: GeoNearNeighSearch first stage (:79-183) as an all-pairs
// gate + 256-bit Hamming kernel with LDS-staged descriptor tiles, SCC_x (:186-248) with one hypothesis per lane,
// ConsistentCheck (:323-405) + RobustMatching rows (:35-45) + Optimizer::GetKpsPairs (optimizer.cpp:575-639)
// as ordered block compactions.  Integer results are bit-exact against oracle/orc_match.c.
#include "dsss_internal.h"
#include "dsss_wave.h"
#include <type_traits>

#define MT_TILE 256          // threads per block = keypoints of A per block = B entries per LDS tile

// ------------------------------------------------------------------ K9: gate + nearest / second nearest
// grid: (tiles of A, 2 * active pairs).  Thread = one keypoint a of the query frame; the reference frame's
// descriptors (32 B) and geo points (16 B) are staged through LDS in tiles of 256 and read as wave-wide
// broadcasts (all lanes same address: conflict-free).  Order of b is index order, so "first index wins" ties
// (FEAmatcher.cpp:152-161) come out exactly as in the scalar loop.
// MODE 0: Hamming on the 32 ORB bytes; 1: L2 on the same 32 bytes (what the shipped reference feeds its L2 branch); 2: L2 on the 128-element
// rows of DSSS_DESC_SIFT128 (`desc` is then the 128-byte store).  The elements are integers 0..255, so the squared distance is an exact
// integer: |a|^2 + |b|^2 - 2 a.b with the dot products on v_dot4_u32_u8 (NW uint4 of four words each; 32 per product of 128-byte rows).
template <int NW>
__device__ inline unsigned mt_dot(const uint4 (&q)[NW], const uint4* __restrict__ b)
{
    unsigned acc = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const uint4 v = b[w];
        acc = __builtin_amdgcn_udot4(q[w].x, v.x, acc, false); acc = __builtin_amdgcn_udot4(q[w].y, v.y, acc, false);
        acc = __builtin_amdgcn_udot4(q[w].z, v.z, acc, false); acc = __builtin_amdgcn_udot4(q[w].w, v.w, acc, false);
    }
    return acc;
}
// ---- the rules of the first stage, each said once (match_nn_kernel, match_grid_kernel, mt_grid_count_kernel; scc_kernel takes the first)
// directed pair pd = 2 p + dir: the query frame fa is the pair's source in direction 0, its target in direction 1
struct mt_dir { int p, dir, fa, fb; };
__device__ __forceinline__ mt_dir mt_dir_of(const int* __restrict__ act_s, const int* __restrict__ act_t, int pd)
{
    const int p = pd >> 1, dir = pd & 1;
    return { p, dir, dir ? act_t[p] : act_s[p], dir ? act_s[p] : act_t[p] };
}
// the geo box of the reference frame; a query outside it has no match (FEAmatcher.cpp:84): ordered comparisons, a NaN is NOT outside
struct mt_box { double x0, x1, y0, y1; };
__device__ __forceinline__ mt_box mt_box_of(const double* __restrict__ bbox, int fb) { return { bbox[fb * 4 + 0], bbox[fb * 4 + 1], bbox[fb * 4 + 2], bbox[fb * 4 + 3] }; }
__device__ __forceinline__ bool mt_outside(double x, double y, const mt_box& B) { return x < B.x0 || y < B.y0 || x > B.x1 || y > B.y1; }
__device__ __forceinline__ int mt_hamming256(const unsigned* a, const unsigned* b)
{
    int d = 0;
#pragma unroll
    for (int w = 0; w < 8; ++w) d += __popc(a[w] ^ b[w]);
    return d;
}
// the query's descriptor and its distance to a candidate's; where the candidate's words (and, MODE 2, its squared norm) come from --
// an LDS tile, the sorted copy, the store -- is the caller's business
template <int MODE>
struct mt_query {
    uint4 w[MODE == 2 ? 8 : 2]; unsigned n2;                   // the 32 bytes as (lo, hi), or the 128-byte row and |q|^2
    __device__ __forceinline__ void load(const uint4* __restrict__ d)
    {
#pragma unroll
        for (int i = 0; i < (MODE == 2 ? 8 : 2); ++i) w[i] = d[i];
        if constexpr (MODE != 0) n2 = mt_dot(w, d);
    }
    __device__ __forceinline__ int dist(const uint4& lo, const uint4& hi) const        // MODE 0, 1: the candidate's 32 bytes
    {
        if constexpr (MODE == 0) {
            const unsigned wa[8] = { w[0].x, w[0].y, w[0].z, w[0].w, w[1].x, w[1].y, w[1].z, w[1].w };
            const unsigned wb[8] = { lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w };
            return mt_hamming256(wa, wb);
        } else {
            const uint4 b[2] = { lo, hi };
            return dist(b, mt_dot(b, b));
        }
    }
    __device__ __forceinline__ int dist(const uint4* __restrict__ b, unsigned bn2) const { return (int)(n2 + bn2 - 2u * mt_dot(w, b)); }      // MODE 1, 2
};
// (best, second, lowest index at the minimum, number of candidates) of a query, FEAmatcher.cpp:86-161.  The scalar loop's "first
// index wins" (:152-161) is take_in_order() when the candidates come in index order; take() and fold() say the same without the
// order: the two smallest distances (a tie at the minimum makes the second equal to it) and the lowest index at the minimum.
struct mt_best2 {
    int best, second, id, nc;
    template <bool L2> __device__ __forceinline__ static mt_best2 none() { return { L2 ? 1000000 : 1000, L2 ? 1000000 : 1000, -1, 0 }; }
    __device__ __forceinline__ void take_in_order(int d, int i)
    {
        ++nc;
        if (d < best) { second = best; best = d; id = i; } else if (d < second) second = d;
    }
    __device__ __forceinline__ void take(int d, int i)
    {
        ++nc;
        if (d < best) { second = best; best = d; id = i; } else if (d == best) { second = d; if (i < id) id = i; } else if (d < second) second = d;
    }
    // another part of the same query's candidates: the two smallest of the union, the lowest index among the minima, the counts added
    __device__ __forceinline__ void fold(const mt_best2& o)
    {
        if (o.best < best) { second = min(best, o.second); best = o.best; id = o.id; }
        else if (o.best == best) { second = best; id = min(id, o.id); }      // (both -1 when nothing beat the initial value)
        else second = min(second, o.best);
        nc += o.nc;
    }
    // the accepted candidate or -1 (FEAmatcher.cpp:99-131)
    template <bool L2> __device__ __forceinline__ int accept(int fa, int fb, int bound_same, int bound_diff, double l2_bound, double ratio_max) const
    {
        if (nc == 0) return -1;
        if (!L2) {
            const int bound = ((fa % 2) != (fb % 2)) ? bound_diff : bound_same;
            const double r = (double)best / (double)second;
            if (id != -1 && best <= bound && r <= ratio_max && second != 1000) return id;
            return nc == 1 && best <= bound ? id : -1;
        }
        const double bd = sqrt((double)best), sd = sqrt((double)second);   // cv::norm(NORM_L2), FEAmatcher.cpp:113
        const double r = bd / sd;
        if (id != -1 && bd < l2_bound && r <= ratio_max) return id;
        return nc == 1 && bd < l2_bound ? id : -1;
    }
};
template <int MODE>
__global__ __launch_bounds__(MT_TILE) void match_nn_kernel(
    const int* __restrict__ act_s, const int* __restrict__ act_t, const int* __restrict__ nkp,
    const uint8_t* __restrict__ desc, const double* __restrict__ geo, const double* __restrict__ bbox,
    int kcap, double gate_T, int bound_same, int bound_diff, double l2_bound, double ratio_max,
    int32_t* __restrict__ corres_nn)
{
    constexpr bool L2 = MODE != 0;
    constexpr int DW = MODE == 2 ? 8 : 1;          // uint4 per half-descriptor slot
    constexpr int DB = MODE == 2 ? 128 : 32;       // bytes per descriptor
    __shared__ uint4 s_lo[MT_TILE * DW], s_hi[MODE == 2 ? 1 : MT_TILE];
    __shared__ unsigned s_n2[MODE == 2 ? MT_TILE : 1];
    __shared__ double2 s_geo[MT_TILE];
    const int pd = blockIdx.y;
    const mt_dir D = mt_dir_of(act_s, act_t, pd);
    const int fa = D.fa, fb = D.fb, na = nkp[fa], nb = nkp[fb];
    const int a = blockIdx.x * MT_TILE + threadIdx.x;
    if (blockIdx.x * MT_TILE >= na) return;                       // whole block beyond the query frame
    int32_t* out = corres_nn + (size_t)pd * kcap;
    const mt_box B = mt_box_of(bbox, fb);
    double ax = 0, ay = 0;
    mt_query<MODE> Q = {};
    bool live = a < na;
    if (live) {
        const double2 g = reinterpret_cast<const double2*>(geo)[(size_t)fa * kcap + a];
        ax = g.x; ay = g.y;
        live = !mt_outside(ax, ay, B);
        Q.load(reinterpret_cast<const uint4*>(desc + ((size_t)fa * kcap + a) * DB));
    }
    if (!__syncthreads_or(live)) { if (a < na) out[a] = -1; return; }
    mt_best2 R = mt_best2::none<L2>();
    const uint4* bdesc = reinterpret_cast<const uint4*>(desc + (size_t)fb * kcap * DB);
    const double2* bgeo = reinterpret_cast<const double2*>(geo) + (size_t)fb * kcap;
    for (int b0 = 0; b0 < nb; b0 += MT_TILE) {
        const int bj = b0 + threadIdx.x;
        if (bj < nb) {
            if (MODE == 2) {
                uint4 t[8];
#pragma unroll
                for (int w = 0; w < 8; ++w) { t[w] = bdesc[8 * bj + w]; s_lo[threadIdx.x * 8 + w] = t[w]; }
                s_n2[threadIdx.x] = mt_dot(t, bdesc + 8 * bj);
            } else { s_lo[threadIdx.x] = bdesc[2 * bj]; s_hi[threadIdx.x] = bdesc[2 * bj + 1]; }
            s_geo[threadIdx.x] = bgeo[bj];
        }
        __syncthreads();
        const int cnt = min(MT_TILE, nb - b0);
        if (live) {
            for (int j = 0; j < cnt; ++j) {
                const double2 g = s_geo[j];
                const double dx = ax - g.x, dy = ay - g.y;
                const double d2 = dx * dx + dy * dy;
                if (d2 < gate_T) {                               // sqrt(d2) < radius, FEAmatcher.cpp:92-93
                    int d;
                    if constexpr (MODE == 2) d = Q.dist(s_lo + 8 * j, s_n2[j]);
                    else d = Q.dist(s_lo[j], s_hi[j]);
                    R.take_in_order(d, b0 + j);                  // b in index order
                }
            }
        }
        __syncthreads();
    }
    if (a < na) out[a] = R.template accept<L2>(fa, fb, bound_same, bound_diff, l2_bound, ratio_max);      // (a query outside the box has met no candidate)
}

// ------------------------------------------------------------------ K9 on a geo grid
// (best, second, lowest index at the minimum, number of candidates) of FEAmatcher.cpp:86-161 do not depend on the order in which the
// candidates inside the search circle are met, so only the keypoints that CAN be inside it are looked at: every frame of an active pair
// gets its keypoints counting-sorted by the cell of a grid over its geo box whose cells are a hair wider than the radius (so that two
// points closer than the radius lie in the same or in adjacent cells whatever the rounding of the cell arithmetic), and a query walks the
// three rows of three cells around its own cell -- three contiguous ranges of the sorted arrays.  The gate itself is the SAME double
// comparison as in the all-pairs kernel, on the same coordinates: the set that passes it is the same set.  At C3 a query meets ~25
// candidates instead of 2 000.
struct mt_grid { int W, H, off, pad; };            // cells per row, rows, first entry of the frame's (W H + 1) cell offsets

__device__ inline int mt_cell(double v, double o, double inv_cs, int n)
{
    const int c = (int)((v - o) * inv_cs);           // monotone in v (saturating conversion; NaN -> 0), and so is the clamp
    return min(max(c, 0), n - 1);
}

// one workgroup per frame: count per cell (global atomics), exclusive scan over the cells, scatter.  The order inside a cell is
// whatever the atomics give; nothing downstream depends on it.
#define MTG_THREADS 1024
__global__ __launch_bounds__(MTG_THREADS) void mt_grid_build_kernel(
    const int* __restrict__ frames, const mt_grid* __restrict__ tab, const int* __restrict__ nkp,
    const uint8_t* __restrict__ desc, const double* __restrict__ geo, const double* __restrict__ bbox, int kcap, double inv_cs,
    int* __restrict__ start_all, int* __restrict__ cur_all, double2* __restrict__ s_geo, uint4* __restrict__ s_desc, int* __restrict__ s_idx)
{
    __shared__ int s_w[MTG_THREADS / 64];
    const int f = frames[blockIdx.x];
    const mt_grid T = tab[f];
    const int n = nkp[f], cells = T.W * T.H;
    int* __restrict__ start = start_all + T.off; int* __restrict__ cur = cur_all + T.off;
    const double ox = bbox[f * 4 + 0], oy = bbox[f * 4 + 2];
    const double2* __restrict__ g = reinterpret_cast<const double2*>(geo) + (size_t)f * kcap;
    for (int i = threadIdx.x; i <= cells; i += MTG_THREADS) cur[i] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += MTG_THREADS) {
        const double2 p = g[i];
        atomicAdd(&cur[mt_cell(p.y, oy, inv_cs, T.H) * T.W + mt_cell(p.x, ox, inv_cs, T.W)], 1);
    }
    __syncthreads();
    int run = 0;
    for (int c0 = 0; c0 < cells; c0 += MTG_THREADS) {
        const int i = c0 + threadIdx.x;
        const int v = i < cells ? __hip_atomic_load(&cur[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;      // (counted by atomics at L2: not through this CU's vector cache)
        int tot;
        const int pos = run + dsss_block_scan_excl<MTG_THREADS / 64, int>(v, &tot, s_w);
        if (i < cells) { start[i] = pos; cur[i] = pos; }
        run += tot;
    }
    __syncthreads();                                 // (every cur[] is in place before another thread's atomic moves it)
    if (threadIdx.x == 0) start[cells] = n;
    const uint4* __restrict__ d = reinterpret_cast<const uint4*>(desc + (size_t)f * kcap * 32);
    const size_t ob = (size_t)f * kcap;
    for (int i = threadIdx.x; i < n; i += MTG_THREADS) {
        const double2 p = g[i];
        const int pos = atomicAdd(&cur[mt_cell(p.y, oy, inv_cs, T.H) * T.W + mt_cell(p.x, ox, inv_cs, T.W)], 1);
        s_geo[ob + pos] = p; s_desc[2 * (ob + pos)] = d[2 * i]; s_desc[2 * (ob + pos) + 1] = d[2 * i + 1]; s_idx[ob + pos] = i;
    }
}

// grid: (tiles of MT_TILE / MT_LPQ queries, 2 * active pairs).  MT_LPQ = 8 ADJACENT LANES PER QUERY: lane s of the eight takes the
// candidates s, s + 8, ... of each of the three row ranges (eight neighbouring geo points are one 128-byte read), and the eight partial
// results are folded by three butterfly steps -- the fold of two (best, second, lowest index, count) is as order-free as the update.  The
// kernel's time is its longest chain of dependent cache round trips: keypoints come in clumps (one landmark at several pyramid levels),
// and with one lane per query a clump of 200 in a cell is 600 round trips for its lanes while the rest of the chip has long finished
// (323 us at C3 against 926 us for the all-pairs kernel; with eight lanes per query and cells of half the radius 162 us + 27 us for the sort).  Queries in THEIR OWN sorted order:
// neighbouring groups are neighbours on the sea floor and walk the same cells.  No LDS, no barrier.
#ifndef MT_LPQ
#define MT_LPQ 8
#endif
#ifndef MT_SUB
#define MT_SUB 2                 // cells per radius: a query walks (2 MT_SUB + 1)^2 cells, 25 cells of 4 m = 400 m^2 against 9 of 8 m = 576 m^2 (the circle: 201 m^2)
#endif
// the rows a query at (x, y) walks in the grid of frame fb: the clamped columns c0 .. c1 of the 2 MT_SUB + 1 rows around its cell
struct mt_rows {
    const int* start; int W, H, cy, c0, c1;
    // row r of the 2 MT_SUB + 1: the range [jb, je) of the sorted arrays, empty for a row outside the grid
    __device__ __forceinline__ void range(int r, int& jb, int& je) const
    {
        const int row = cy - MT_SUB + r;
        const bool ok = row >= 0 && row < H;
        jb = ok ? start[row * W + c0] : 0; je = ok ? start[row * W + c1 + 1] : 0;
    }
};
__device__ __forceinline__ mt_rows mt_rows_of(const mt_grid* __restrict__ tab, const int* __restrict__ start_all, int fb, const mt_box& B, double x, double y, double inv_cs)
{
    const mt_grid T = tab[fb];
    const int cx = mt_cell(x, B.x0, inv_cs, T.W), cy = mt_cell(y, B.y0, inv_cs, T.H);
    return { start_all + T.off, T.W, T.H, cy, max(cx - MT_SUB, 0), min(cx + MT_SUB, T.W - 1) };
}
template <int MODE>          // as match_nn_kernel; MODE 2 reads the 128-byte rows of the feature store through the sorted index (s_desc = the store)
__global__ __launch_bounds__(MT_TILE) void match_grid_kernel(
    const int* __restrict__ act_s, const int* __restrict__ act_t, const int* __restrict__ nkp, const double* __restrict__ bbox,
    const mt_grid* __restrict__ tab, const int* __restrict__ start_all, const double2* __restrict__ s_geo, const uint4* __restrict__ s_desc,
    const int* __restrict__ s_idx, int kcap, double inv_cs, double gate_T, int bound_same, int bound_diff, double l2_bound, double ratio_max,
    int32_t* __restrict__ corres_nn)
{
    constexpr bool L2 = MODE != 0;
    const int pd = blockIdx.y;
    const mt_dir D = mt_dir_of(act_s, act_t, pd);
    const int fa = D.fa, fb = D.fb, na = nkp[fa];
    const int t = blockIdx.x * (MT_TILE / MT_LPQ) + (threadIdx.x / MT_LPQ), sub = threadIdx.x & (MT_LPQ - 1);
    if (t >= na) return;                                         // (whole groups of eight lanes leave together: the shuffles below stay inside a group)
    const size_t sa = (size_t)fa * kcap + t;
    const double2 ga = s_geo[sa];
    const int a = s_idx[sa];
    int32_t* out = corres_nn + (size_t)pd * kcap;
    const mt_box B = mt_box_of(bbox, fb);
    const double ax = ga.x, ay = ga.y;
    if (mt_outside(ax, ay, B)) { if (sub == 0) out[a] = -1; return; }
    mt_query<MODE> Q;
    Q.load(MODE == 2 ? s_desc + ((size_t)fa * kcap + a) * 8 : s_desc + 2 * sa);
    const mt_rows rows = mt_rows_of(tab, start_all, fb, B, ax, ay, inv_cs);
    int jb[2 * MT_SUB + 1], je[2 * MT_SUB + 1];                  // the rows' ranges, fetched together
#pragma unroll
    for (int r = 0; r < 2 * MT_SUB + 1; ++r) rows.range(r, jb[r], je[r]);
    const size_t sb = (size_t)fb * kcap;
    mt_best2 R = mt_best2::none<L2>();
#pragma unroll
    for (int r = 0; r < 2 * MT_SUB + 1; ++r)
        for (int j = jb[r] + sub; j < je[r]; j += MT_LPQ) {
            const double2 g = s_geo[sb + j];
            const double dx = ax - g.x, dy = ay - g.y;
            const double d2 = dx * dx + dy * dy;
            if (d2 < gate_T) {                                   // sqrt(d2) < radius, FEAmatcher.cpp:92-93
                const int id = s_idx[sb + j];
                int d;
                if constexpr (MODE == 2) {
                    const uint4* bd = s_desc + (sb + id) * 8;
                    uint4 t[8];
#pragma unroll
                    for (int w = 0; w < 8; ++w) t[w] = bd[w];
                    d = Q.dist(bd, mt_dot(t, bd));
                } else d = Q.dist(s_desc[2 * (sb + j)], s_desc[2 * (sb + j) + 1]);
                R.take(d, id);                                   // cells in any order
            }
        }
#pragma unroll
    for (int o = 1; o < MT_LPQ; o <<= 1)                         // the eight lanes of the query
        R.fold(mt_best2{ __shfl_xor(R.best, o, 64), __shfl_xor(R.second, o, 64), __shfl_xor(R.id, o, 64), __shfl_xor(R.nc, o, 64) });
    if (sub == 0) out[a] = R.template accept<L2>(fa, fb, bound_same, bound_diff, l2_bound, ratio_max);
}

// per-kernel profile only (outside the matcher's timed scope): the gate evaluations match_grid_kernel performs = the sizes of the row
// ranges its live queries walk; bench.py prices the kernel by them
__global__ __launch_bounds__(MT_TILE) void mt_grid_count_kernel(
    const int* __restrict__ act_s, const int* __restrict__ act_t, const int* __restrict__ nkp, const double* __restrict__ bbox,
    const mt_grid* __restrict__ tab, const int* __restrict__ start_all, const double2* __restrict__ s_geo, int kcap, double inv_cs,
    unsigned long long* __restrict__ n_evals)
{
    __shared__ unsigned long long s_tot;
    if (threadIdx.x == 0) s_tot = 0;
    __syncthreads();
    const mt_dir D = mt_dir_of(act_s, act_t, blockIdx.y);
    const int t = blockIdx.x * MT_TILE + threadIdx.x;
    if (t < nkp[D.fa]) {
        const double2 ga = s_geo[(size_t)D.fa * kcap + t];
        const mt_box B = mt_box_of(bbox, D.fb);
        if (!mt_outside(ga.x, ga.y, B)) {
            const mt_rows rows = mt_rows_of(tab, start_all, D.fb, B, ga.x, ga.y, inv_cs);
            int tot = 0;
            for (int r = 0; r < 2 * MT_SUB + 1; ++r) { int jb, je; rows.range(r, jb, je); tot += je - jb; }
            atomicAdd(&s_tot, (unsigned long long)tot);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_tot) atomicAdd(n_evals, s_tot);
}

// ------------------------------------------------------------------ K10: SCC_x (FEAmatcher.cpp:186-248)
// the model of hypothesis `it`: the mean of the two matches its RNG words draw (:201), summed in the reference's order
__device__ __forceinline__ double scc_model_of(const float* xv, const uint32_t* __restrict__ rng_raw, int it, int nloc)
{
    const int s0 = (int)(rng_raw[2 * it] % (uint32_t)nloc), s1 = (int)(rng_raw[2 * it + 1] % (uint32_t)nloc);
    double model = 0.0;
    model = model + xv[s0];
    model = model + xv[s1];
    model = model / 2;
    return model;
}
// one block per directed active pair; hypotheses are independent given the fixed cv::RNG stream (the reference
// default-constructs the generator on every call, :59), so each lane evaluates whole hypotheses and the
// "first strictly larger inlier set wins" rule (:237) becomes max count, then lowest iteration index.
__global__ __launch_bounds__(256) void scc_kernel(
    const int* __restrict__ act_s, const int* __restrict__ act_t, const int* __restrict__ nkp,
    const int* __restrict__ frows, const dsss_kp* __restrict__ kps, int kcap,
    const uint32_t* __restrict__ rng_raw, int iters, double pix_err,
    const int32_t* __restrict__ corres_nn, int32_t* __restrict__ corres,
    int* __restrict__ scc_hist, int* __restrict__ scc_count, double* __restrict__ scc_model)
{
    extern __shared__ __align__(16) unsigned char smem[];
    int* id_loc = reinterpret_cast<int*>(smem);                       // [kcap]
    float* xv = reinterpret_cast<float*>(smem + (size_t)kcap * 4);    // [kcap] X_tmp per accepted match, ID_loc order
    int* cnts = reinterpret_cast<int*>(smem + (size_t)kcap * 8);      // [iters]
    __shared__ int s_w[4];
    __shared__ int s_best_it, s_hist, s_nloc;
    __shared__ double s_model;
    const int pd = blockIdx.x;
    const mt_dir D = mt_dir_of(act_s, act_t, pd);
    const int fa = D.fa, fb = D.fb, na = nkp[fa];
    const bool flip = (fa % 2) != (fb % 2);
    const float rows_ref = (float)frows[fb];
    const dsss_kp* ka = kps + (size_t)fa * kcap;
    const dsss_kp* kb = kps + (size_t)fb * kcap;
    const int32_t* nn = corres_nn + (size_t)pd * kcap;
    int32_t* out = corres + (size_t)pd * kcap;
    // ID_loc in index order (:132,169)
    int base = 0;
    for (int c0 = 0; c0 < na; c0 += 256) {
        const int i = c0 + threadIdx.x;
        const int m = (i < na) ? nn[i] : -1;
        int tot;
        const int pos = dsss_block_scan_excl<4, int>(m != -1, &tot, s_w);
        if (m != -1) {
            const float ya = ka[i].y, yb = kb[m].y;
            id_loc[base + pos] = i;
            xv[base + pos] = flip ? fabsf(ya - ((rows_ref - yb) + 1.0f)) : fabsf(ya - yb);   // :209-212,222-227
        }
        base += tot;
    }
    if (threadIdx.x == 0) s_nloc = base;
    __syncthreads();
    const int nloc = s_nloc;
    if (nloc == 0) {
        for (int i = threadIdx.x; i < na; i += 256) out[i] = -1;
        if (threadIdx.x == 0) { scc_hist[pd] = 0; scc_count[pd] = 0; scc_model[pd] = 0.0; }
        return;
    }
    for (int it = threadIdx.x; it < iters; it += 256) {
        const double model = scc_model_of(xv, rng_raw, it, nloc);
        int cnt = 0;
        for (int k = 0; k < nloc; ++k) cnt += fabs(model - (double)xv[k]) <= pix_err;
        cnts[it] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int fin = 0, best_it = -1, hist = 0;
        for (int it = 0; it < iters; ++it) if (fin < cnts[it]) { fin = cnts[it]; best_it = it; ++hist; }   // :237-242
        s_best_it = best_it; s_hist = hist;
        const double model = best_it >= 0 ? scc_model_of(xv, rng_raw, best_it, nloc) : 0.0;
        s_model = model;
        scc_hist[pd] = hist; scc_count[pd] = fin; scc_model[pd] = model;
    }
    __syncthreads();
    const double model = s_model; const bool any = s_best_it >= 0;
    for (int i = threadIdx.x; i < na; i += 256) out[i] = -1;
    __syncthreads();
    for (int k = threadIdx.x; k < nloc; k += 256) {
        const int i = id_loc[k];
        if (any && fabs(model - (double)xv[k]) <= pix_err) out[i] = nn[i];
    }
}

// ------------------------------------------------------------------ ConsistentCheck + rows + GetKpsPairs
// block per active pair.  WRITE = false counts, WRITE = true fills rows6/kp7 at the scanned offsets, so the
// placement is deterministic (pair order, then the reference's in-pair order).
template <bool WRITE>
__global__ __launch_bounds__(256) void pair_rows_kernel(
    const int* __restrict__ act_s, const int* __restrict__ act_t, const int* __restrict__ nkp,
    const int* __restrict__ frows, const int* __restrict__ fcols, const dsss_kp* __restrict__ kps, int kcap,
    const int32_t* __restrict__ corres, const int* __restrict__ scc_hist, const double* __restrict__ scc_model,
    double merge_thr, const double* const* __restrict__ alt_ptr, const double* const* __restrict__ gr_ptr,
    const double* const* __restrict__ pose_ptr,
    int* __restrict__ row_cnt, int* __restrict__ kp7_cnt, const int* __restrict__ row_off, const int* __restrict__ kp7_off,
    double* __restrict__ rows6, double* __restrict__ kp7, int* __restrict__ kp7_pair, uint8_t* __restrict__ kp7_flip)
{
    __shared__ int s_w[4];
    __shared__ int s_red[2];
    const int p = blockIdx.x;
    const int fs = act_s[p], ft = act_t[p];
    const int n1 = nkp[fs], n2 = nkp[ft];
    const int32_t* c1 = corres + (size_t)(2 * p) * kcap;
    const int32_t* c2 = corres + (size_t)(2 * p + 1) * kcap;
    const dsss_kp* ks = kps + (size_t)fs * kcap;
    const dsss_kp* kt = kps + (size_t)ft * kcap;
    // merge decision (:341-345); an empty scc history falls to the "larger direction" branch
    double img_diff = 0;
    if ((fs % 2) != (ft % 2)) img_diff = (double)abs(frows[fs] - frows[ft]);
    bool merge = false;
    if (scc_hist[2 * p] > 0 && scc_hist[2 * p + 1] > 0)
        merge = fabs(fabs(scc_model[2 * p] - scc_model[2 * p + 1]) - img_diff) <= merge_thr;
    bool use1 = true, use2 = true;
    if (!merge) {
        if (threadIdx.x < 2) s_red[threadIdx.x] = 0;
        __syncthreads();
        int l1 = 0, l2 = 0;
        for (int i = threadIdx.x; i < n1; i += 256) l1 += c1[i] != -1;
        for (int i = threadIdx.x; i < n2; i += 256) l2 += c2[i] != -1;
        atomicAdd(&s_red[0], l1); atomicAdd(&s_red[1], l2);
        __syncthreads();
        use1 = s_red[0] > s_red[1]; use2 = !use1;                  // :378,391 ties -> direction 2
    }
    const int ngr_s = fcols[fs] / 2, ngr_t = fcols[ft] / 2;      // ground_ranges.size()
    const double* alt_s = alt_ptr[fs]; const double* alt_t = alt_ptr[ft];
    const double* gr_s = gr_ptr[fs]; const double* gr_t = gr_ptr[ft];
    const double* pose_s = pose_ptr[fs]; const double* pose_t = pose_ptr[ft];
    const int ro = WRITE ? row_off[p] : 0, ko = WRITE ? kp7_off[p] : 0;
    int rbase = 0, kbase = 0, flip_s_run = 0, flip_t_run = 0;
    for (int phase = 0; phase < 2; ++phase) {
        if (phase == 0 && !use1) continue;
        if (phase == 1 && !use2) continue;
        const int n = phase == 0 ? n1 : n2;
        for (int c0 = 0; c0 < n; c0 += 256) {
            const int i = c0 + threadIdx.x;
            int src = -1, tgt = -1;
            if (i < n) {
                if (phase == 0) { const int m = c1[i]; if (m != -1 && !(merge && c2[m] == i)) { src = i; tgt = m; } }   // :348-360
                else { const int m = c2[i]; if (m != -1) { src = m; tgt = i; } }                                    // :362-371
            }
            const bool valid = src >= 0;
            int tot;
            const int pos = dsss_block_scan_excl<4, int>(valid, &tot, s_w);
            double ys = 0, xs = 0, yt = 0, xt = 0;
            if (valid) {
                ys = (double)ks[src].y; xs = (double)ks[src].x; yt = (double)kt[tgt].y; xt = (double)kt[tgt].x;
                if (WRITE) {
                    double* r = rows6 + (size_t)(ro + rbase + pos) * 6;                                              // :37-40
                    r[0] = fs; r[1] = ft; r[2] = ys; r[3] = xs; r[4] = yt; r[5] = xt;
                }
            }
            rbase += tot;
            // GetKpsPairs (optimizer.cpp:596-631): int truncation, nadir rejection
            bool v7 = false; int ps = 0, bs = 0, pt = 0, bt = 0;
            if (valid) {
                ps = (int)ys; bs = (int)xs; pt = (int)yt; bt = (int)xt;
                v7 = !(abs(bs - ngr_s) < 20 || abs(bt - ngr_t) < 20);
            }
            int tot7;
            const int pos7 = dsss_block_scan_excl<4, int>(v7, &tot7, s_w);
            // sticky yaw compensation flags of LoopClosingTFs (optimizer.cpp:650,698-703): prefix OR in list order
            const int fs_here = v7 && dsss_yaw_flips(pose_s[(size_t)ps * 6 + 2]);
            const int ft_here = v7 && dsss_yaw_flips(pose_t[(size_t)pt * 6 + 2]);
            int tfs, tft;
            const int pre_s = dsss_block_scan_excl<4, int>(fs_here, &tfs, s_w) + fs_here;
            const int pre_t = dsss_block_scan_excl<4, int>(ft_here, &tft, s_w) + ft_here;
            if (WRITE && v7) {
                const size_t o = (size_t)(ko + kbase + pos7);
                int gis = abs(bs - ngr_s), git = abs(bt - ngr_t);
                gis = gis < ngr_s ? gis : ngr_s - 1; git = git < ngr_t ? git : ngr_t - 1;
                const double as = alt_s[ps], gs = gr_s[gis], at = alt_t[pt], gt = gr_t[git];
                double* q = kp7 + o * 7;
                q[0] = ps; q[1] = bs; q[2] = sqrt(as * as + gs * gs);                                               // :616-619
                q[3] = pt; q[4] = bt; q[5] = sqrt(at * at + gt * gt); q[6] = 0;
                kp7_pair[o] = p;
                kp7_flip[o] = (uint8_t)(((flip_s_run + pre_s) > 0 ? 1 : 0) | ((flip_t_run + pre_t) > 0 ? 2 : 0));
            }
            kbase += tot7; flip_s_run += tfs; flip_t_run += tft;
        }
    }
    if (!WRITE && threadIdx.x == 0) { row_cnt[p] = rbase; kp7_cnt[p] = kbase; }
}

// exclusive scan of two small int arrays (one block)
__global__ void scan2_kernel(const int* __restrict__ a, const int* __restrict__ b, int n, int* __restrict__ oa, int* __restrict__ ob)
{
    __shared__ int s_w[4];
    int ba = 0, bb = 0;
    for (int c0 = 0; c0 < n; c0 += 256) {
        const int i = c0 + threadIdx.x;
        const int va = i < n ? a[i] : 0, vb = i < n ? b[i] : 0;
        int ta, tb;
        const int pa = dsss_block_scan_excl<4, int>(va, &ta, s_w);
        const int pb = dsss_block_scan_excl<4, int>(vb, &tb, s_w);
        if (i < n) { oa[i] = ba + pa; ob[i] = bb + pb; }
        ba += ta; bb += tb;
    }
    if (threadIdx.x == 0) { oa[n] = ba; ob[n] = bb; }
}

__global__ void hamming_one_kernel(const uint8_t* a, const uint8_t* b, int* out)
{
    *out = mt_hamming256(reinterpret_cast<const unsigned*>(a), reinterpret_cast<const unsigned*>(b));
}

// threshold T with sqrt(d) < radius  <=>  d < T for correctly rounded sqrt
static double gate_threshold(double radius)
{
    double t = radius * radius;
    if (std::sqrt(t) >= radius) { while (std::sqrt(t) >= radius && t > 0) t = std::nextafter(t, 0.0); t = std::nextafter(t, INFINITY); }
    else { while (std::sqrt(t) < radius) t = std::nextafter(t, INFINITY); }
    return t;
}

// ------------------------------------------------------------------ the device buffers of a pair result set (dsss_internal.h)
// Allocated and freed HERE only, one family per capacity field, by the family rule of dsss_internal.h (dsss_family_alloc): synchronise, free + null, allocate, and
// publish the capacity only after every allocation of the family succeeded.  Each family is listed ONCE, with the sizes for `n` of its capacity's unit.
static std::array<dsss_fam_slot, 3> pair_index_family(dsss_ctx* c, size_t np = 0) { return {{ dsss_slot(c->act_s, np * sizeof(int)), dsss_slot(c->act_t, np * sizeof(int)), dsss_slot(c->kp7_off, (np + 1) * sizeof(int)) }}; }
static std::array<dsss_fam_slot, 8> pair_match_family(dsss_ctx* c, size_t np = 0)
{
    return {{ dsss_slot(c->corres_nn, 2 * np * c->kcap * sizeof(int32_t)), dsss_slot(c->corres, 2 * np * c->kcap * sizeof(int32_t)), dsss_slot(c->scc_hist, 2 * np * sizeof(int)), dsss_slot(c->scc_count, 2 * np * sizeof(int)),
              dsss_slot(c->scc_model, 2 * np * sizeof(double)), dsss_slot(c->row_cnt, np * sizeof(int)), dsss_slot(c->kp7_cnt, np * sizeof(int)), dsss_slot(c->row_off, (np + 1) * sizeof(int)) }};
}
static std::array<dsss_fam_slot, 4> rows_family(dsss_ctx* c, size_t want = 0) { return {{ dsss_slot(c->rows6, want * 6 * sizeof(double)), dsss_slot(c->kp7, want * 7 * sizeof(double)), dsss_slot(c->kp7_pair, want * sizeof(int)), dsss_slot(c->kp7_flip, want) }}; }
static std::array<dsss_fam_slot, 3> grid_sorted_family(dsss_ctx* c, size_t FK = 0) { return {{ dsss_slot(c->mt_gs_geo, FK * 2 * sizeof(double)), dsss_slot(c->mt_gs_desc, FK * 32), dsss_slot(c->mt_gs_idx, FK * sizeof(int)) }}; }
int dsss_mt_reserve_pair_index(dsss_ctx* c, size_t np) { return np <= c->pair_idx_cap ? DSSS_OK : dsss_family_alloc(c, "pair index", c->pair_idx_cap, np, pair_index_family(c, np)); }
int dsss_mt_reserve_pair_match(dsss_ctx* c, size_t np) { return np <= c->match_cap_pairs ? DSSS_OK : dsss_family_alloc(c, "pair match buffers", c->match_cap_pairs, np, pair_match_family(c, np)); }
int dsss_mt_reserve_rows(dsss_ctx* c, size_t n) { return n <= c->rows_cap ? DSSS_OK : dsss_family_alloc(c, "match rows", c->rows_cap, n + 1024, rows_family(c, n + 1024)); }
// mt_aux = the [3][max_frames] device pointers alt, gr, pose6 (d_ptrs; small, rebuilt per call), then the 2 * scc_iters words of the cv::RNG stream
static uint32_t* aux_rng_words(dsss_ctx* c) { return (uint32_t*)(c->mt_aux.as<char>() + 3 * (size_t)c->max_frames * sizeof(double*)); }
int dsss_mt_upload_ptr_tables(dsss_ctx* c)
{
    const int F = c->max_frames;
    std::vector<const double*> hp(3 * (size_t)F, nullptr);
    for (int f = 0; f < F; ++f) { hp[f] = c->frames[f].alt; hp[F + f] = c->frames[f].gr; hp[2 * F + f] = c->frames[f].pose6; }
    const size_t need = hp.size() * sizeof(double*) + 2 * (size_t)c->mt.scc_iters * sizeof(uint32_t);
    c->d_ptrs = nullptr;                 // a view into mt_aux: none while that may fail
    if (const int rc = c->mt_aux.reserve(c, need)) return rc;
    c->d_ptrs = c->mt_aux.as<const double*>();
    HIPCHK(c, hipMemcpyAsync((void*)c->d_ptrs, hp.data(), hp.size() * sizeof(double*), hipMemcpyHostToDevice, c->stream));
    return DSSS_OK;
}

// the geo grid's own buffers (matcher only): the sorted copies of [F][kcap] keypoints, and tables + cell offsets with a quarter of headroom
static int reserve_grid(dsss_ctx* c, size_t FK, size_t cells_bytes)
{
    if (c->mt_gs_cap != FK) { if (const int rc = dsss_family_alloc(c, "geo grid sorted copies", c->mt_gs_cap, FK, grid_sorted_family(c, FK))) return rc; }
    return c->mt_cells.reserve(c, cells_bytes, cells_bytes + cells_bytes / 4);
}
void dsss_mt_clear_results(dsss_ctx* c)
{
    c->npairs = c->nactive = 0; c->total_rows = c->total_kp7 = 0; c->has_lc = false; c->corres_valid = false;
    c->pair_s.clear(); c->pair_t.clear(); c->pair_active.clear(); c->h_row_off.assign(1, 0); c->h_kp7_off.assign(1, 0);
}
void dsss_mt_free(dsss_ctx* c)
{
    dsss_mt_clear_results(c);            // the bookkeeping describes these buffers
    dsss_family_release(c->pair_idx_cap, pair_index_family(c)); dsss_family_release(c->match_cap_pairs, pair_match_family(c)); dsss_family_release(c->rows_cap, rows_family(c));
    dsss_family_release(c->mt_gs_cap, grid_sorted_family(c)); c->d_ptrs = nullptr; c->mt_aux.release(); c->mt_cells.release();
}

// dsss_match_params::use_l2 -> the kernels' MODE, chosen in ONE place: fn gets it as a compile-time constant
template <class Fn> static void with_mode(int use_l2, Fn&& fn)
{
    if (use_l2 == 2) fn(std::integral_constant<int, 2>()); else if (use_l2) fn(std::integral_constant<int, 1>()); else fn(std::integral_constant<int, 0>());
}

// ------------------------------------------------------------------ host flow of dsss_match_pairs
// In the manner of ex_run (dsss_extract.hip): the call's state and one method per stage, in the order of run().  Everything is built in the run's own
// members; the context's result set is written by publish() alone, after the last launch.
struct mt_run {
    dsss_ctx* const c; const int* const src; const int* const tgt; const int npairs; const dsss_switches sw;      // ---- the call
    const int F; const size_t K; const int iters;
    // ---- the plan: active pairs, launch sizes, the gate, the matcher's algorithmic work, the grid's host half
    std::vector<int> as, at, active; int na = 0, max_nkp = 0; double T = 0, evals = 0;
    bool use_grid = false; double inv_cs = 0; std::vector<mt_grid> gtab; std::vector<int> gframes; size_t gcells = 0;
    // ---- views into mt_cells (grid only; d_evals: profile only) and the downloaded offsets
    mt_grid* d_tab = nullptr; int *d_frames = nullptr, *d_start = nullptr, *d_cur = nullptr; unsigned long long* d_evals = nullptr;
    std::vector<int> h_row_off, h_kp7_off;
    mt_run(dsss_ctx* c_, const int* s_, const int* t_, int n_) : c(c_), src(s_), tgt(t_), npairs(n_), sw(dsss_switches_read()), F(c_->max_frames), K(c_->kcap), iters(c_->mt.scc_iters) {}
    int run() {
        int rc = plan(); if (rc) return rc;
        if (na > 0) {
            use_grid = plan_grid();
            if ((rc = reserve()) || (rc = upload_tables()) || (rc = enqueue_nn()) || (rc = enqueue_scc()) || (rc = enqueue_row_counts()) || (rc = finish())) return rc;
        }
        publish(); return DSSS_OK;
    }

    int plan() {
        int rc = dsss_sync_bboxes(c); if (rc) return rc;
        active.assign(npairs, -1);
        for (int p = 0; p < npairs; ++p) {
            const int s = src[p], t = tgt[p];
            if (s < 0 || s >= F || t < 0 || t >= F || s == t) DSSS_FAIL(c, DSSS_E_ARG, "pair %d: bad frame ids (%d,%d)", p, s, t);
            const dsss_frame &a = c->frames[s], &b = c->frames[t];
            if (!a.has_feat || !b.has_feat) DSSS_FAIL(c, DSSS_E_STATE, "pair %d: frames %d/%d have no features", p, s, t);
            if (c->mt.use_l2 == 2 && (!a.has_sift || !b.has_sift)) DSSS_FAIL(c, DSSS_E_STATE, "pair %d: use_l2 = 2 needs the 128-element rows of frames %d/%d (dsss_orb_params.descriptor = DSSS_DESC_SIFT128)", p, s, t);
            // a keypoint outside the other frame's geo box is skipped (FEAmatcher.cpp:84), so disjoint boxes match nothing
            const bool disjoint = a.bbox[1] < b.bbox[0] || b.bbox[1] < a.bbox[0] || a.bbox[3] < b.bbox[2] || b.bbox[3] < a.bbox[2];
            if (disjoint || a.nkp == 0 || b.nkp == 0) continue;
            active[p] = (int)as.size(); as.push_back(s); at.push_back(t);
            evals += 2.0 * a.nkp * b.nkp;      // algorithmic work of the matcher: gate + Hamming evaluations = sum over the directed active pairs of Na x Nb
        }
        na = (int)as.size();
        h_row_off.assign(na + 1, 0); h_kp7_off.assign(na + 1, 0);
        for (int f = 0; f < F; ++f) if (c->frames[f].has_feat) max_nkp = std::max(max_nkp, c->frames[f].nkp);
        T = gate_threshold(c->mt.radius);
        if (na > 0 && scc_lds() > 150 * 1024) DSSS_FAIL(c, DSSS_E_CAPACITY, "SCC kernel needs %zu B of LDS", scc_lds());
        return DSSS_OK;
    }
    size_t scc_lds() const { return K * 8 + (size_t)iters * 4; }

    // geo grid over the frames of the active pairs (match_grid_kernel); the all-pairs kernel stays for a degenerate geometry (a
    // non-finite box or radius, or a box of more than 2^22 cells) and as the A/B switch DSSS_MT_GRID=0
    bool plan_grid() {
        if (!(sw.mt_grid && std::isfinite(c->mt.radius) && c->mt.radius > 0)) return false;
        const double cs = c->mt.radius / MT_SUB * (1.0 + 1.0 / 1048576.0); inv_cs = 1.0 / cs;      // the hair: 1e-6 of a cell against 1e-13 of rounding
        gtab.assign(F, mt_grid{ 0, 0, 0, 0 });
        std::vector<char> seen(F, 0);
        for (int a2 = 0; a2 < na; ++a2)
            for (int f : { as[a2], at[a2] }) {
                if (seen[f]) continue; else seen[f] = 1;
                const double* b = c->frames[f].bbox;
                const double w = (b[1] - b[0]) * inv_cs, h = (b[3] - b[2]) * inv_cs;
                if (!(std::isfinite(b[0]) && std::isfinite(b[2]) && w >= 0 && h >= 0 && (w + 1) * (h + 1) < 4194304.0)) return false;
                mt_grid& g = gtab[f];
                g.W = (int)w + 1; g.H = (int)h + 1; g.off = (int)gcells; gcells += (size_t)g.W * g.H + 1;
                gframes.push_back(f);
            }
        return gcells < (size_t)1 << 30;
    }

    int reserve() {
        int rc;
        if ((rc = dsss_mt_reserve_pair_index(c, na)) || (rc = dsss_mt_reserve_pair_match(c, na)) || !use_grid) return rc;
        if ((rc = reserve_grid(c, (size_t)F * K, 2 * gcells * sizeof(int) + (size_t)F * sizeof(mt_grid) + (size_t)F * sizeof(int) + 16))) return rc;
        char* base = c->mt_cells.as<char>();
        d_tab = (mt_grid*)base;                                                   // [F] (16-byte entries first: alignment)
        d_frames = (int*)(base + (size_t)F * sizeof(mt_grid));                    // [frames of the active pairs]
        d_start = d_frames + F; d_cur = d_start + gcells;
        if (c->prof.on) d_evals = (unsigned long long*)(((uintptr_t)(d_cur + gcells) + 7) & ~(uintptr_t)7);
        return DSSS_OK;
    }

    int upload_tables() {
        HIPCHK(c, hipMemcpyAsync(c->act_s, as.data(), na * sizeof(int), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->act_t, at.data(), na * sizeof(int), hipMemcpyHostToDevice, c->stream));
        int rc = dsss_mt_upload_ptr_tables(c); if (rc) return rc;
        std::vector<uint32_t> raw(2 * (size_t)iters);
        { uint64_t st = 0xffffffffu; for (auto& r : raw) { st = (uint64_t)(uint32_t)st * 4164903690U + (uint32_t)(st >> 32); r = (uint32_t)st; } }
        HIPCHK(c, hipMemcpyAsync(aux_rng_words(c), raw.data(), raw.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        if (!use_grid) return DSSS_OK;
        if (d_evals) HIPCHK(c, hipMemsetAsync(d_evals, 0, sizeof(unsigned long long), c->stream));
        HIPCHK(c, hipMemcpyAsync(d_tab, gtab.data(), (size_t)F * sizeof(mt_grid), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_frames, gframes.data(), gframes.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
        return DSSS_OK;
    }

    int enqueue_nn() {
        const dsss_match_params& m = c->mt;
        const dim3 grid((max_nkp + MT_TILE - 1) / MT_TILE, 2 * na);
        if (use_grid) {
            dsss_scope sc(c, DSSS_K_MATCH, evals, 2);
            const dim3 ggrid((max_nkp + MT_TILE / MT_LPQ - 1) / (MT_TILE / MT_LPQ), 2 * na);
            hipLaunchKernelGGL(mt_grid_build_kernel, dim3((unsigned)gframes.size()), dim3(MTG_THREADS), 0, c->stream, d_frames, d_tab, c->nkp_dev, c->desc, c->geo,
                               c->bbox_dev, (int)K, inv_cs, d_start, d_cur, (double2*)c->mt_gs_geo, (uint4*)c->mt_gs_desc, c->mt_gs_idx);
            const uint4* sdesc = (const uint4*)(m.use_l2 == 2 ? c->desc128.as<uint8_t>() : c->mt_gs_desc);      // MODE 2 reads the store's 128-byte rows
            with_mode(m.use_l2, [&](auto mode) {
                hipLaunchKernelGGL(match_grid_kernel<decltype(mode)::value>, ggrid, dim3(MT_TILE), 0, c->stream, c->act_s, c->act_t, c->nkp_dev, c->bbox_dev, d_tab,
                                   d_start, (const double2*)c->mt_gs_geo, sdesc, c->mt_gs_idx, (int)K, inv_cs, T, m.bound_same, m.bound_diff, m.l2_bound, m.ratio, c->corres_nn); });
            HIPCHK(c, hipGetLastError());
        } else {
            dsss_scope sc(c, DSSS_K_MATCH, evals);
            if (c->prof.on) c->prof.work[DSSS_K_MATCH_DONE] += evals;      // the all-pairs kernel performs every evaluation it is credited with
            with_mode(m.use_l2, [&](auto mode) {
                hipLaunchKernelGGL(match_nn_kernel<decltype(mode)::value>, grid, dim3(MT_TILE), 0, c->stream, c->act_s, c->act_t, c->nkp_dev,
                                   m.use_l2 == 2 ? c->desc128.as<uint8_t>() : c->desc, c->geo, c->bbox_dev, (int)K, T, m.bound_same, m.bound_diff, m.l2_bound, m.ratio, c->corres_nn); });
            HIPCHK(c, hipGetLastError());
        }
        if (!d_evals) return DSSS_OK;
        // (profile on) the grid's evaluations, counted behind the matcher's closed scope; finish() adds them to the work done
        hipLaunchKernelGGL(mt_grid_count_kernel, grid, dim3(MT_TILE), 0, c->stream, c->act_s, c->act_t, c->nkp_dev, c->bbox_dev, d_tab, d_start, (const double2*)c->mt_gs_geo, (int)K, inv_cs, d_evals);
        HIPCHK(c, hipMemcpyAsync(&c->mt_evals_host, d_evals, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        return DSSS_OK;
    }

    int enqueue_scc() {
        dsss_scope sc(c, DSSS_K_SCC);
        hipLaunchKernelGGL(scc_kernel, dim3(2 * na), dim3(256), scc_lds(), c->stream, c->act_s, c->act_t, c->nkp_dev, c->rows_dev, c->kps, (int)K,
                           aux_rng_words(c), iters, c->mt.pix_err, c->corres_nn, c->corres, c->scc_hist, c->scc_count, c->scc_model);
        HIPCHK(c, hipGetLastError());
        return DSSS_OK;
    }

    template <bool WRITE> hipError_t launch_rows() {      // the count pass (nothing but row_cnt / kp7_cnt written) and the write pass
        const double* const* P = c->d_ptrs;
        hipLaunchKernelGGL(pair_rows_kernel<WRITE>, dim3(na), dim3(256), 0, c->stream, c->act_s, c->act_t, c->nkp_dev, c->rows_dev, c->cols_dev,
                           c->kps, (int)K, c->corres, c->scc_hist, c->scc_model, c->mt.merge_thr, P, P + F, P + 2 * F, c->row_cnt, c->kp7_cnt,
                           WRITE ? c->row_off : nullptr, WRITE ? c->kp7_off : nullptr, WRITE ? c->rows6 : nullptr, WRITE ? c->kp7 : nullptr,
                           WRITE ? c->kp7_pair : nullptr, WRITE ? c->kp7_flip : nullptr);
        return hipGetLastError();
    }
    int enqueue_row_counts() {
        dsss_scope sc(c, DSSS_K_ROWS);
        HIPCHK(c, launch_rows<false>());
        hipLaunchKernelGGL(scan2_kernel, dim3(1), dim3(256), 0, c->stream, c->row_cnt, c->kp7_cnt, na, c->row_off, c->kp7_off);
        HIPCHK(c, hipGetLastError());
        return DSSS_OK;
    }

    // the one synchronisation of the call: the totals size the row buffers of the write pass
    int finish() {
        HIPCHK(c, hipMemcpyAsync(h_row_off.data(), c->row_off, (na + 1) * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(h_kp7_off.data(), c->kp7_off, (na + 1) * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (d_evals) c->prof.work[DSSS_K_MATCH_DONE] += (double)c->mt_evals_host;
        int rc = dsss_mt_reserve_rows(c, h_row_off[na]); if (rc) return rc;
        if (h_row_off[na] > 0) {
            dsss_scope sc(c, DSSS_K_ROWS);
            HIPCHK(c, launch_rows<true>());
        }
        return DSSS_OK;
    }

    void publish() {
        c->npairs = npairs; c->nactive = na;
        c->pair_s.assign(src, src + npairs); c->pair_t.assign(tgt, tgt + npairs); c->pair_active.swap(active);
        c->total_rows = h_row_off[na]; c->total_kp7 = h_kp7_off[na];
        c->h_row_off.swap(h_row_off); c->h_kp7_off.swap(h_kp7_off);
        c->corres_valid = true;           // (has_lc stays false: dsss_lc_solve_all has not seen these rows)
    }
};

extern "C" {

int dsss_match_pairs(dsss_ctx* c, const int* src_ids, const int* tgt_ids, int npairs)
{
    if (!c || npairs < 0 || (npairs > 0 && (!src_ids || !tgt_ids))) return DSSS_E_ARG;
    dsss_mt_clear_results(c);            // whatever fails from here on leaves an EMPTY result set (include/dsss.h)
    HIPCHK(c, hipSetDevice(c->device));
    return mt_run(c, src_ids, tgt_ids, npairs).run();
}

int dsss_match_get_dir(dsss_ctx* c, int pair, int dir, int32_t* corres_nn, int32_t* corres, int cap, int* hist, int* count, double* model)
{
    if (!c) return DSSS_E_ARG;
    if (pair < 0 || pair >= c->npairs || dir < 0 || dir > 1) DSSS_FAIL(c, DSSS_E_ARG, "pair %d / dir %d out of range", pair, dir);
    const int fa = dir ? c->pair_t[pair] : c->pair_s[pair];
    const int n = c->frames[fa].nkp;
    if (cap < n) DSSS_FAIL(c, DSSS_E_CAPACITY, "caller capacity %d < %d", cap, n);
    const int a = c->pair_active[pair];
    if (a >= 0 && !c->corres_valid) DSSS_FAIL(c, DSSS_E_STATE, "pair %d: the result set is dsss_lc_solve_pairs', which has no correspondences", pair);
    if (a < 0) {
        for (int i = 0; i < n; ++i) { if (corres_nn) corres_nn[i] = -1; if (corres) corres[i] = -1; }
        if (hist) *hist = 0; if (count) *count = 0; if (model) *model = 0;
        return DSSS_OK;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t o = (size_t)(2 * a + dir) * c->kcap;
    if (corres_nn && n) HIPCHK(c, hipMemcpy(corres_nn, c->corres_nn + o, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (corres && n) HIPCHK(c, hipMemcpy(corres, c->corres + o, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (hist) HIPCHK(c, hipMemcpy(hist, c->scc_hist + 2 * a + dir, sizeof(int), hipMemcpyDeviceToHost));
    if (count) HIPCHK(c, hipMemcpy(count, c->scc_count + 2 * a + dir, sizeof(int), hipMemcpyDeviceToHost));
    if (model) HIPCHK(c, hipMemcpy(model, c->scc_model + 2 * a + dir, sizeof(double), hipMemcpyDeviceToHost));
    return DSSS_OK;
}

// one pair's rows of rows6 / kp7 (width doubles each) to the host; off: the host copy of the active pairs' offsets into the buffer
static int get_pair_rows(dsss_ctx* c, int pair, std::vector<int> dsss_ctx::*off_, double* dsss_ctx::*dev, int width, double* out, int cap, int* nout)
{
    if (!c) return DSSS_E_ARG;
    if (pair < 0 || pair >= c->npairs) DSSS_FAIL(c, DSSS_E_ARG, "pair %d out of range", pair);
    const std::vector<int>& off = c->*off_;
    const int a = c->pair_active[pair];
    const int n = a < 0 ? 0 : off[a + 1] - off[a];
    if (nout) *nout = n;
    if (n == 0 || !out) return DSSS_OK;
    if (cap < n) DSSS_FAIL(c, DSSS_E_CAPACITY, "caller capacity %d < %d rows", cap, n);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->*dev + (size_t)off[a] * width, (size_t)n * width * sizeof(double), hipMemcpyDeviceToHost));
    return DSSS_OK;
}
int dsss_match_get_rows(dsss_ctx* c, int pair, double* rows6, int cap, int* nrows) { return get_pair_rows(c, pair, &dsss_ctx::h_row_off, &dsss_ctx::rows6, 6, rows6, cap, nrows); }
int dsss_match_get_kp7(dsss_ctx* c, int pair, double* kp7, int cap, int* nout) { return get_pair_rows(c, pair, &dsss_ctx::h_kp7_off, &dsss_ctx::kp7, 7, kp7, cap, nout); }

int dsss_match_pair_active(dsss_ctx* c, int pair, int* active)
{
    if (!c || !active) return DSSS_E_ARG;
    if (pair < 0 || pair >= c->npairs) DSSS_FAIL(c, DSSS_E_ARG, "pair %d out of range", pair);
    *active = c->pair_active[pair] >= 0;
    return DSSS_OK;
}

int dsss_match_total(dsss_ctx* c, int* total_rows, int* total_kp7)
{
    if (!c) return DSSS_E_ARG;
    if (total_rows) *total_rows = c->total_rows;
    if (total_kp7) *total_kp7 = c->total_kp7;
    return DSSS_OK;
}

int dsss_descriptor_distance(dsss_ctx* c, int id_a, int ia, int id_b, int ib, int* dist)
{
    if (!c || !dist) return DSSS_E_ARG;
    if (id_a < 0 || id_a >= c->max_frames || id_b < 0 || id_b >= c->max_frames) DSSS_FAIL(c, DSSS_E_ARG, "frame id out of range");
    if (!c->frames[id_a].has_feat || !c->frames[id_b].has_feat || ia < 0 || ib < 0 || ia >= c->frames[id_a].nkp || ib >= c->frames[id_b].nkp)
        DSSS_FAIL(c, DSSS_E_ARG, "descriptor index out of range");
    if (const int rc = c->tmp_dev.reserve(c, 64 * sizeof(int))) return rc;      // once per context, not per call
    int* d_out = c->tmp_dev.as<int>();
    hipLaunchKernelGGL(hamming_one_kernel, dim3(1), dim3(1), 0, c->stream, c->desc + ((size_t)id_a * c->kcap + ia) * 32,
                       c->desc + ((size_t)id_b * c->kcap + ib) * 32, d_out);
    hipError_t e = hipMemcpyAsync(dist, d_out, sizeof(int), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    HIPCHK(c, e);
    return DSSS_OK;
}

} // extern "C"

// diasss_amd/csrc/dsss_pg_bins.hip -- the BOTTOM of the elimination tree of the reduced pose-graph system (dsss_pg_sym.h): whole subtrees
// binned into one workgroup each.  First the kernels that build the bins' index tables on the device (update lists, update map, root
// boundary indices), then the numeric kernels (left-looking block columns, backward substitution).
// These kernels are compared with the oracle at 1e-6 on the poses, not bit for bit, so they may fuse multiply-adds; everything else in
// the library stays at -ffp-contract=off.
#include "dsss_pg_kernels.h"
#include "dsss_pg_dev.h"
#pragma clang fp contract(fast)
// ---- sparse block Cholesky of the binned columns, left-looking.
// Column j holds blocks L(i, j), i in rowidx[colptr[j] .. colptr[j+1]) ascending, first the diagonal.
// rowlist(j) = binned columns k < j with L(j, k) != 0 and the position of that block.
// upd_map (built once per solve by pg_build_map_kernel): for update t of column j and target block q the position of
// L(i_q, k_t) or -1; layout [mapptr[j] + t * m_j + q], so the factor kernel has no dependent index search.
__global__ __launch_bounds__(256) void pg_build_map_kernel(int nupd, const int* __restrict__ rlrow, const int* __restrict__ rlptr,
                                                           const int* __restrict__ rlcol, const int* __restrict__ rlpos,
                                                           const int* __restrict__ colptr, const int* __restrict__ rowidx,
                                                           const long long* __restrict__ mapptr, int* __restrict__ upd_map, const int* __restrict__ nupd_dev)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= (nupd_dev ? *nupd_dev : nupd)) return;             // (lists built on the device: their total stays there, the grid covers the bound)
    const int j = rlrow[e], k = rlcol[e];
    const int c0 = colptr[j], m = colptr[j + 1] - c0;
    int* mp = upd_map + mapptr[j] + (long long)(e - rlptr[j]) * m;
    int q = 0;
    for (int p = rlpos[e]; p < colptr[k + 1]; ++p) {           // rows of column k from row j downwards: a subset of column j's rows
        const int i = rowidx[p];
        while (q < m && rowidx[c0 + q] < i) ++q;
        if (q < m && rowidx[c0 + q] == i) mp[q] = p;
    }
}

// ---- The bins' index tables built ON THE DEVICE (round 3): the update lists (per target column j the binned source columns k < j
// with L(j, k) != 0, ascending, and the position of that block), the offsets of the update map, and for the rows of a binned column
// beyond its subtree root their index in the root's boundary list.  On the host they were the last 0.9 ms of the analysis before the
// first trial could touch the bins (35 ms at the 4 M-pose graph of config 5); they are independent of everything the analysis does
// afterwards.  Same content, same order (a list is sorted by source column), so the factor is bit-identical to the host-built one
// (DSSS_PG_LISTS=host keeps the host path; the host twin of the CPU tests always uses it).
__global__ __launch_bounds__(256) void pg_rl_count_kernel(int ns, const int* __restrict__ colptr, const int* __restrict__ rowidx, const char* __restrict__ binned,
                                                          int* __restrict__ cnt)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= ns || !binned[k]) return;
    for (int q = colptr[k] + 1; q < colptr[k + 1]; ++q) { const int j = rowidx[q]; if (binned[j]) atomicAdd(&cnt[j], 1); }
}
// exclusive scan in three launches (1024 values per workgroup, up to 1024 x 1024 values): VAL 0 = the counts themselves (int),
// VAL 1 = count x blocks of the column (long long: the update map holds one entry per (update, target block))
template <typename T, int VAL>
__global__ __launch_bounds__(1024) void pg_scan_block_kernel(int n, const int* __restrict__ cnt, const int* __restrict__ colptr, T* __restrict__ out, T* __restrict__ block_sum)
{
    __shared__ T s_w[16];
    const int i = blockIdx.x * 1024 + threadIdx.x;
    T v = 0, tot;
    if (i < n) v = VAL == 0 ? (T)cnt[i] : (T)cnt[i] * (T)(colptr[i + 1] - colptr[i]);
    const T pos = dsss_block_scan_excl<16, T>(v, &tot, s_w);
    if (i < n) out[i] = pos;
    if (threadIdx.x == 0) block_sum[blockIdx.x] = tot;
}
template <typename T>
__global__ __launch_bounds__(1024) void pg_scan_tops_kernel(int nblocks, T* __restrict__ block_sum, T* __restrict__ total)
{
    __shared__ T s_w[16];
    T carry = 0;
    for (int b0 = 0; b0 < nblocks; b0 += 1024) {
        const int i = b0 + threadIdx.x;
        const T v = i < nblocks ? block_sum[i] : (T)0;
        T tot;
        const T pos = dsss_block_scan_excl<16, T>(v, &tot, s_w);
        if (i < nblocks) block_sum[i] = carry + pos;
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}
template <typename T>
__global__ __launch_bounds__(1024) void pg_scan_add_kernel(int n, T* __restrict__ out, const T* __restrict__ block_sum, const T* __restrict__ total)
{
    const int i = blockIdx.x * 1024 + threadIdx.x;
    if (i < n) out[i] += block_sum[blockIdx.x];
    if (i == 0) out[n] = *total;
}
__global__ __launch_bounds__(256) void pg_rl_fill_kernel(int ns, const int* __restrict__ colptr, const int* __restrict__ rowidx, const char* __restrict__ binned,
                                                         const int* __restrict__ rlptr, int* __restrict__ cur, int* __restrict__ rlcol, int* __restrict__ rlpos)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= ns || !binned[k]) return;
    for (int q = colptr[k] + 1; q < colptr[k + 1]; ++q) {
        const int j = rowidx[q];
        if (!binned[j]) continue;
        const int at = rlptr[j] + atomicAdd(&cur[j], 1);          // any order: pg_rl_sort_kernel sorts the list by source column
        rlcol[at] = k; rlpos[at] = q;
    }
}
// one wavefront per target column: its list sorted by source column (the keys are distinct: rank = number of smaller keys)
#define PG_RL_SORT_CAP 1024
__global__ __launch_bounds__(256) void pg_rl_sort_kernel(int ns, const int* __restrict__ rlptr, int* __restrict__ rlcol, int* __restrict__ rlpos, int* __restrict__ rlrow,
                                                         int* __restrict__ fail)
{
    __shared__ int s_k[4][PG_RL_SORT_CAP], s_q[4][PG_RL_SORT_CAP];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + wv;
    if (j >= ns) return;
    const int b = rlptr[j], len = rlptr[j + 1] - b;
    if (len <= 0) return;
    if (len > PG_RL_SORT_CAP) { if (lane == 0) *fail = 2; return; }      // (a bin's lists sum to a few hundred entries: cannot happen; never silent)
    for (int e = lane; e < len; e += 64) { s_k[wv][e] = rlcol[b + e]; s_q[wv][e] = rlpos[b + e]; }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_wave_barrier();
    for (int e = lane; e < len; e += 64) {
        const int key = s_k[wv][e];
        int rank = 0;
        for (int f = 0; f < len; ++f) rank += s_k[wv][f] < key;
        rlcol[b + rank] = key; rlpos[b + rank] = s_q[wv][e]; rlrow[b + rank] = j;
    }
}
__global__ __launch_bounds__(256) void pg_fill_map_kernel(int* __restrict__ upd_map, const long long* __restrict__ total)
{
    const long long n = *total;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) upd_map[i] = -1;
}
__global__ __launch_bounds__(256) void pg_anc_rel_kernel(int ns, const int* __restrict__ colptr, const int* __restrict__ rowidx, const char* __restrict__ binned,
                                                         const int* __restrict__ root_of, int* __restrict__ anc_first, int* __restrict__ anc_rel)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= ns || !binned[k]) return;
    const int r = root_of[k], c0 = colptr[k], m = colptr[k + 1] - c0;
    int q = 0;
    while (q < m && rowidx[c0 + q] <= r) ++q;
    anc_first[k] = q;
    const int* __restrict__ rb = rowidx + colptr[r] + 1; const int nb = colptr[r + 1] - colptr[r] - 1;
    int w = 0;
    for (; q < m; ++q) { const int row = rowidx[c0 + q]; while (w < nb && rb[w] < row) ++w; anc_rel[c0 + q] = (w < nb && rb[w] == row) ? w : -1; }
}

#define PG_TCH 128
// ---- bottom of the elimination tree: whole subtrees per workgroup (no grid-wide level barriers).
// A bin is a list of columns in ascending order whose sources all lie in the same bin, so the workgroup can run them back to
// back with workgroup barriers only (left-looking, block-sparse, update map).  Only columns with at most 42 blocks
// (6m <= 256 rows: one pass) are binned.  Every finished column also adds its outer product over the rows BEYOND its subtree
// root to the root's update matrix U_root (and L y to its right-hand side part): what the first front above the bin
// extend-adds, exactly like the F22 of a child front.  One workgroup owns a bin, columns in fixed order: deterministic.
// acc[s] += sum_t L(i,k_t)[r][:] . L(j,k_t)[s][:] for the tn updates staged in LDS.  Updates that do not touch this
// row (map entry -1) are masked instead of skipped, and four updates are in flight at once, so the index load and the
// six operand loads of different updates overlap instead of forming one dependent chain per update.
__device__ inline void pg_acc_rows(const int* __restrict__ mp, int m, int tn, const double* __restrict__ Lvals, int r,
                                   const double* __restrict__ s_Ljk, double* acc)
{
    int t = 0;
    for (; t + 4 <= tn; t += 4) {
        int pos[4]; double a[4][6];
#pragma unroll
        for (int u = 0; u < 4; ++u) pos[u] = mp[(size_t)(t + u) * m];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double* Lik = Lvals + (size_t)(pos[u] < 0 ? 0 : pos[u]) * 36 + r * 6;
#pragma unroll
            for (int c = 0; c < 6; ++c) a[u][c] = Lik[c];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (pos[u] < 0) continue;
            const double* B = s_Ljk + (t + u) * 36;
#pragma unroll
            for (int s = 0; s < 6; ++s)
                acc[s] += a[u][0] * B[s * 6] + a[u][1] * B[s * 6 + 1] + a[u][2] * B[s * 6 + 2] + a[u][3] * B[s * 6 + 3] + a[u][4] * B[s * 6 + 4] + a[u][5] * B[s * 6 + 5];
        }
    }
    for (; t < tn; ++t) {
        const int pos = mp[(size_t)t * m];
        if (pos < 0) continue;
        const double* Lik = Lvals + (size_t)pos * 36 + r * 6;
        const double* B = s_Ljk + t * 36;
        const double a0 = Lik[0], a1 = Lik[1], a2 = Lik[2], a3 = Lik[3], a4 = Lik[4], a5 = Lik[5];
#pragma unroll
        for (int s = 0; s < 6; ++s)
            acc[s] += a0 * B[s * 6] + a1 * B[s * 6 + 1] + a2 * B[s * 6 + 2] + a3 * B[s * 6 + 3] + a4 * B[s * 6 + 4] + a5 * B[s * 6 + 5];
    }
}
// THE SERIAL FORM (DSSS_PG_BINS=serial): a column's phases follow each other, every operand is fetched where it is used.  What the pipelined
// kernel below is held to, bit for bit (tests/test_gpu_pg_bins.py).
__global__ __launch_bounds__(256) void pg_factor_subtree_serial_kernel(const int* __restrict__ bin_perm, const int* __restrict__ binptr, const int* __restrict__ bincols,
                                                                const int* __restrict__ colptr, const int* __restrict__ rlptr,
                                                                const int* __restrict__ rlcol, const int* __restrict__ rlpos,
                                                                const long long* __restrict__ mapptr, const int* __restrict__ upd_map,
                                                                double* __restrict__ Lvals, double* __restrict__ x, int* __restrict__ fail,
                                                                const int* __restrict__ binroot_ptr, const int* __restrict__ binroot_idx,
                                                                const int* __restrict__ broot_b, const long long* __restrict__ broot_uoff,
                                                                const int* __restrict__ broot_of_col, const int* __restrict__ anc_first,
                                                                const int* __restrict__ anc_rel, double* __restrict__ ubin, double* __restrict__ rdiag)
{
    __shared__ double s_Ljk[PG_TCH * 36];          // update staging; reused for the column's ancestor blocks (42 x 36)
    __shared__ double s_yk[PG_TCH * 6];
    __shared__ double s_diag[36];
    __shared__ int s_arel[48];                     // boundary indices of the column's ancestor rows (at most 42)
    __shared__ double s_ri[6];                     // 1 / L(j, j)[a][a]: the solves below multiply (a dependent f64 division is ~15 instructions)
    __shared__ double s_y[6];
    __shared__ double s_xj[6];
    __shared__ int s_ok;
    const int bin = bin_perm[blockIdx.x];          // bins in descending order of work
    for (int q = binroot_ptr[bin]; q < binroot_ptr[bin + 1]; ++q) {        // zero the update matrices of this bin's roots
        const int ri = binroot_idx[q]; const long long b6 = 6LL * broot_b[ri]; double* U = ubin + broot_uoff[ri];
        for (long long e = threadIdx.x; e < b6 * b6 + b6; e += 256) U[e] = 0.0;
    }
    // (round 5) what a column needs to know about itself -- column -> pointers -> root descriptor, three dependent look-ups of a microsecond
    // together -- is fetched one column AHEAD; and a thread keeps its row of the column in registers from the update to the triangular solve
    // (it was stored after the update and read back after the pivot: a round trip through the caches on every column's chain)
    struct colinfo { int j, c0, m, t0, T, af, ri, b6; long long mapoff, uoff; };
    auto col_of = [&](int ci2) {
        colinfo k;
        k.j = bincols[ci2];
        k.c0 = colptr[k.j]; k.m = colptr[k.j + 1] - k.c0;
        k.t0 = rlptr[k.j]; k.T = rlptr[k.j + 1] - k.t0;
        k.mapoff = mapptr[k.j]; k.af = anc_first[k.j]; k.ri = broot_of_col[k.j];
        k.b6 = k.ri >= 0 ? 6 * broot_b[k.ri] : 0; k.uoff = k.ri >= 0 ? broot_uoff[k.ri] : 0;
        return k;
    };
    const int ci_end = binptr[bin + 1];
    colinfo cur = {}, nxt = {};
    if (binptr[bin] < ci_end) cur = col_of(binptr[bin]);
    for (int ci = binptr[bin]; ci < ci_end; ++ci, cur = nxt) {
        if (ci + 1 < ci_end) nxt = col_of(ci + 1);
        const int j = cur.j;
        const int c0 = cur.c0, m = cur.m;
        const int t0 = cur.t0, T = cur.T;
        const int* mp = upd_map + cur.mapoff;
        const int idx = threadIdx.x;
        const bool act = idx < 6 * m;
        const int q = act ? idx / 6 : 0, r = idx - q * 6;
        const bool rhs = threadIdx.x >= 250;
        const int rs_ = threadIdx.x - 250;
        double acc[6] = { 0, 0, 0, 0, 0, 0 }, accy = 0;
        double rowv[6] = { 0, 0, 0, 0, 0, 0 };                             // row r of block q of the column, as assembled: requested before the updates
        if (act) {
#pragma unroll
            for (int s2 = 0; s2 < 6; ++s2) rowv[s2] = Lvals[(size_t)(c0 + q) * 36 + r * 6 + s2];
        }
        for (int tc = 0; tc < T; tc += PG_TCH) {
            const int tn = min(PG_TCH, T - tc);
            __syncthreads();
            for (int x0 = threadIdx.x; x0 < tn * 36; x0 += 4 * 256) {      // four dependent (position -> block) loads in flight per thread
                int pos[4]; double val[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) { const int xx = x0 + u * 256; pos[u] = xx < tn * 36 ? rlpos[t0 + tc + xx / 36] : 0; }
#pragma unroll
                for (int u = 0; u < 4; ++u) { const int xx = x0 + u * 256; val[u] = xx < tn * 36 ? Lvals[(size_t)pos[u] * 36 + (xx % 36)] : 0.0; }
#pragma unroll
                for (int u = 0; u < 4; ++u) { const int xx = x0 + u * 256; if (xx < tn * 36) s_Ljk[xx] = val[u]; }
            }
            for (int xx = threadIdx.x; xx < tn * 6; xx += 256) s_yk[xx] = x[(size_t)rlcol[t0 + tc + xx / 6] * 6 + (xx % 6)];
            __syncthreads();
            if (rhs)
                for (int t = 0; t < tn; ++t) {
                    const double* yk = s_yk + t * 6; const double* B = s_Ljk + t * 36 + rs_ * 6;
                    accy += B[0] * yk[0] + B[1] * yk[1] + B[2] * yk[2] + B[3] * yk[3] + B[4] * yk[4] + B[5] * yk[5];
                }
            if (act)
                pg_acc_rows(mp + (size_t)tc * m + q, m, tn, Lvals, r, s_Ljk, acc);
        }
        // (round 5) the updated pivot block and right-hand side reach the one-thread section below through LDS: stored to global memory
        // and read back by another thread they were a round trip through the cache hierarchy on every column's chain.  The pivot thread
        // writes both back (the factor and the solved right-hand side), as before.
        if (rhs) s_xj[rs_] = x[(size_t)j * 6 + rs_] - accy;               // (accy = 0 without updates)
        if (act) {
#pragma unroll
            for (int s = 0; s < 6; ++s) rowv[s] -= acc[s];                  // (no updates: acc = 0, x - 0 = x)
            if (idx < 6) { for (int s = 0; s < 6; ++s) s_diag[r * 6 + s] = rowv[s]; }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            // (round 4: in-kernel stamps put this one-thread section at 4 200 cycles per column, 28 % of the kernel -- a square root and
            // 21 dependent divisions; one reciprocal square root per pivot and multiplications by it from here on)
            double A[36], xj[6], ri[6];
#pragma unroll
            for (int a = 0; a < 36; ++a) A[a] = s_diag[a];
#pragma unroll
            for (int a = 0; a < 6; ++a) xj[a] = s_xj[a];
            const int bad = chol6_recip(A, ri);
            if (bad) *fail = 1;
            s_ok = !bad;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int b = 0; b < 6; ++b) { const double v = b <= a ? A[a * 6 + b] : 0.0; s_diag[a * 6 + b] = v; Lvals[(size_t)c0 * 36 + a * 6 + b] = v; }
#pragma unroll
            for (int a = 0; a < 6; ++a) { s_ri[a] = ri[a]; rdiag[(size_t)j * 6 + a] = ri[a]; }
            if (!bad) {
                double v[6];
#pragma unroll
                for (int a = 0; a < 6; ++a) {
                    double t = xj[a];
#pragma unroll
                    for (int b = 0; b < 6; ++b) if (b < a) t -= A[a * 6 + b] * v[b];
                    v[a] = t * ri[a];
                }
#pragma unroll
                for (int a = 0; a < 6; ++a) { x[(size_t)j * 6 + a] = v[a]; s_y[a] = v[a]; }
            }
        }
        __syncthreads();
        if (!s_ok) return;
        const int af = cur.af, ta = m - af;                             // block rows beyond the subtree root (a suffix of the column)
        if (act && idx >= 6) {
            double* row = Lvals + (size_t)(c0 + q) * 36 + r * 6;
            double xr[6];
#pragma unroll
            for (int s = 0; s < 6; ++s) { double v = rowv[s];
#pragma unroll
                                          for (int c = 0; c < 6; ++c) if (c < s) v -= xr[c] * s_diag[s * 6 + c];
                                          xr[s] = v * s_ri[s]; }
            for (int s = 0; s < 6; ++s) row[s] = xr[s];
            if (q >= af) for (int s = 0; s < 6; ++s) s_Ljk[(q - af) * 36 + r * 6 + s] = xr[s];       // keep the ancestor rows for the update matrix
        }
        __syncthreads();
        const int ri = cur.ri;
        if (ri >= 0 && ta > 0) {
            const int b6 = cur.b6;
            double* __restrict__ U = ubin + cur.uoff;
            double* __restrict__ g = U + (size_t)b6 * b6;
            // (round 4) the boundary indices of the column's ancestor rows go to LDS once, and the block pairs ib <= ia are ONE flat loop:
            // per ancestor row the pass was a dependent index load, a load and a store of U in global memory, and the rows followed each
            // other (in-kernel stamps: 3 200 cycles per column, a quarter of the kernel).  Every entry of U still receives one term per column.
            if ((int)threadIdx.x < ta) s_arel[threadIdx.x] = anc_rel[c0 + af + threadIdx.x];
            __syncthreads();
            if ((int)threadIdx.x < 6 * ta) {                            // right-hand side: g[ia] -= L_a y_j
                const int pa = threadIdx.x / 6, a = threadIdx.x - pa * 6;
                const double* La = s_Ljk + pa * 36 + a * 6;
                g[s_arel[pa] * 6 + a] -= La[0] * s_y[0] + La[1] * s_y[1] + La[2] * s_y[2] + La[3] * s_y[3] + La[4] * s_y[4] + La[5] * s_y[5];
            }
            const int npair = ta * (ta + 1) / 2;                        // U[ia][ib] -= L_a L_b^T for the block pairs ib <= ia
            for (int e = threadIdx.x; e < 36 * npair; e += 256) {
                const int pr = e / 36, ab = e - 36 * pr;
                int pa = (int)((sqrtf(8.0f * (float)pr + 1.0f) - 1.0f) * 0.5f);      // pr = pa (pa + 1) / 2 + pb, pb <= pa
                while (pa * (pa + 1) / 2 > pr) --pa;
                while ((pa + 1) * (pa + 2) / 2 <= pr) ++pa;
                const int pb = pr - pa * (pa + 1) / 2, a = ab / 6, b = ab - 6 * a;
                const double* La = s_Ljk + pa * 36 + a * 6; const double* Lb = s_Ljk + pb * 36 + b * 6;
                U[(size_t)(s_arel[pa] * 6 + a) * b6 + s_arel[pb] * 6 + b] -= La[0] * Lb[0] + La[1] * Lb[1] + La[2] * Lb[2] + La[3] * Lb[3] + La[4] * Lb[4] + La[5] * Lb[5];
            }
        }
        __syncthreads();
        __threadfence_block();
    }
}
// ---- THE PIPELINED FORM (the default).  Same sums in the same order as the serial form -- the bits are its bits --, but no dependent global round
// trip is left on a column's chain except the operand rows of the updates, and those run under the previous column's pivot.
//
// What the serial chain was, per column: index -> block -> LDS (staging), then per group of four updates map entry -> operand row, the one-thread
// pivot, the row solve with its stores, boundary indices -> LDS, load / multiply-add / store of U, and only then the next column's staging, which
// fetched back the blocks just stored.  Everything but the values is structure, known columns ahead; every source block of column n + 1 other than
// column n's own is final before column n's pivot begins; and column n's own blocks exist in the workgroup's LDS the moment they are computed.
//
// The phases of column n (B1, B2, B3 are the three workgroup barriers of a column; "top" is what precedes B1, "shadow" lies between B1 and B2):
//   top(n)     T1  issue, for column n + 1: its map entries (PG_NIDX per thread), its boundary indices, and the VALUES of its staged blocks
//                  L(n+1, k) and x_k for the first PG_PCH sources k other than column n (six threads per block, one row each; the positions were
//                  fetched at top(n-1)); issue, for column n + 2, the positions of its staged blocks.
//              T2  (rare) what column n has beyond PG_PCH such sources: staged and accumulated in place, as in the serial form.
//              T3  the update of column n by column n - 1, if that is one of its sources (then it is the LAST of the ascending list): block, operand rows
//                  and x from s_col / s_y, where the row solve and the pivot of column n - 1 left them.  Never through memory.
//              T4  row and right-hand side minus the sums; the pivot rows to s_diag; the boundary indices of column n to s_arel[n & 1].
//              T5  the values of T1 to the staging half (n+1) & 1.
//   shadow(n)      thread 250 (idle in all but 42-block columns, and in the wavefront that has least to do) factorises the pivot block and solves the
//                  right-hand side, as thread 0 does in the serial form; meanwhile every thread adds column n - 1's terms to the update matrix U of its
//                  root, and accumulates the staged updates of column n + 1 (operand rows from global memory, the first PG_NIDX addresses already in
//                  registers).  The assembled row of column n + 1 is requested.  (The pivot on SIX lanes, a row each and the right-hand side as a seventh
//                  column, was built and measured: 176 us a launch at C3 against 153 us with the one thread -- 54 cross-lane moves on the chain cost more
//                  than the 80 operations they save, now that the other 255 threads no longer wait for the pivot but work beside it.)
//   B2 .. B3       the row solve of column n: rows to Lvals and x (for the fronts, the backward sweep and later columns; not awaited) and to s_col.
// Why each early read sees final data -- a value is final for a thread once it was stored before a barrier that thread has passed:
//   * staged blocks L(n+1, k), x_k and the operand rows L(i, k) of column n + 1, k <= n - 1 (T1 and shadow(n)): rows stored between B2(k) and B3(k), x_k
//     in shadow(k) before B2(k); the reader has passed B3(n-1).  Column n itself is excluded (T3 of the next column takes it from LDS).
//   * the assembled row and right-hand side of column n + 1 (shadow(n)): written before the launch; inside it only column n + 1's own pivot and row solve write them.
//   * positions, map entries, boundary indices, descriptors: written before the launch, never inside it.
//   * s_col (written B2(n) .. B3(n)) and s_y[n & 1] (written in shadow(n)) are read at T3 of top(n+1) and by U in shadow(n+1); s_col is overwritten after
//     B2(n+1), s_y[n & 1] in shadow(n+2).
//   * staging half h = (n+1) & 1: written at T5 of top(n), read in shadow(n) and at T2 of top(n+1); written again at T5 of top(n+2), after B3(n+1).
//   * s_arel[n & 1]: written at top(n), read in shadow(n+1), written again at top(n+2).  s_diag, s_xj: pivot rows and right-hand side in at T4, factor out in shadow(n), read B2 .. B3.
//   * U: column n - 1's read-modify-writes lie in shadow(n), column n's in shadow(n+1) (the last column's after its B3): B2(n), B3(n) and B1(n+1), which every
//     thread passes, lie between two columns' accesses to the same entries, and the stores of shadow(n) are a column old by then.
//   * the descriptor ring (PG_DW columns, refilled by halves at top(n), n = 32, 64, ...): the half refilled holds columns n - 32 .. n - 1, which nobody reads
//     any more (descriptors are read at the top, before B1), and is first read 30 columns later.
#define PG_PCH 42               // updates staged ahead per column: 6 threads x 42 = 252; two halves are 28 KB (the serial form's one buffer: 43 KB)
#define PG_NIDX 4               // map entries a thread holds in registers for the next column
#define PG_DW 64                // columns in the descriptor ring
struct pg_coldesc { int j, c0, m, t0, T, af, ri, b6, fpos, c0p; long long mapoff, uoff; };
__device__ inline void pg_upd_term(double (&acc)[6], const double (&a)[6], const double* __restrict__ B)
{
#pragma unroll
    for (int s = 0; s < 6; ++s)
        acc[s] += a[0] * B[s * 6] + a[1] * B[s * 6 + 1] + a[2] * B[s * 6 + 2] + a[3] * B[s * 6 + 3] + a[4] * B[s * 6 + 4] + a[5] * B[s * 6 + 5];
}
__device__ inline void pg_upd_group(const int (&pos)[4], int t, const double* __restrict__ Lvals, int r, const double* __restrict__ s_B, double (&acc)[6])
{
    double a[4][6];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const double* Lik = Lvals + (size_t)(pos[u] < 0 ? 0 : pos[u]) * 36 + r * 6;
#pragma unroll
        for (int c = 0; c < 6; ++c) a[u][c] = Lik[c];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if (pos[u] < 0) continue;
        pg_upd_term(acc, a[u], s_B + (t + u) * 36);
    }
}
// pg_acc_rows with the first PG_NIDX map entries in registers (mpi[u], u < min(tn, PG_NIDX), whatever beyond): the same terms in the same order.  The
// last, partial group runs as a group with its missing updates masked, and no load hangs on a condition (a load behind a branch is waited for
// on the spot, one round trip per update: the serial form's tail).
__device__ inline void pg_acc_rows_ahead(const int (&mpi)[PG_NIDX], const int* __restrict__ mp, int m, int tn, const double* __restrict__ Lvals, int r,
                                         const double* __restrict__ s_B, double (&acc)[6])
{
    const int ng = (tn + 3) >> 2;
#pragma unroll
    for (int g = 0; g < PG_NIDX / 4; ++g)
        if (g < ng) {
            int pos[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) pos[u] = 4 * g + u < tn ? mpi[4 * g + u] : -1;
            pg_upd_group(pos, 4 * g, Lvals, r, s_B, acc);
        }
    for (int g = PG_NIDX / 4; g < ng; ++g) {
        int pos[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) pos[u] = mp[(size_t)min(4 * g + u, tn - 1) * m];
#pragma unroll
        for (int u = 0; u < 4; ++u) if (4 * g + u >= tn) pos[u] = -1;
        pg_upd_group(pos, 4 * g, Lvals, r, s_B, acc);
    }
}
__global__ __launch_bounds__(256, 3) void pg_factor_subtree_kernel(const int* __restrict__ bin_perm, const int* __restrict__ binptr, const int* __restrict__ bincols,
                                                                const int* __restrict__ colptr, const int* __restrict__ rlptr,
                                                                const int* __restrict__ rlcol, const int* __restrict__ rlpos,
                                                                const long long* __restrict__ mapptr, const int* __restrict__ upd_map,
                                                                double* __restrict__ Lvals, double* __restrict__ x, int* __restrict__ fail,
                                                                const int* __restrict__ binroot_ptr, const int* __restrict__ binroot_idx,
                                                                const int* __restrict__ broot_b, const long long* __restrict__ broot_uoff,
                                                                const int* __restrict__ broot_of_col, const int* __restrict__ anc_first,
                                                                const int* __restrict__ anc_rel, double* __restrict__ ubin, double* __restrict__ rdiag)
{
    __shared__ double s_st[2][PG_PCH * 36];        // staged blocks L(n, k) of a column's updates, two halves by the column's parity
    __shared__ double s_sy[2][PG_PCH * 6];         // and the x_k that go with them
    __shared__ double s_col[42 * 36];              // the solved rows of the last column (block 0, the pivot block, is s_diag)
    __shared__ double s_diag[36];
    __shared__ double s_ri[6];                     // 1 / L(j, j)[a][a]
    __shared__ double s_y[2][6];                   // the solved right-hand side of a column, by parity
    __shared__ int s_arel[2][48];                  // boundary indices of a column's ancestor rows (at most 42), by parity
    __shared__ int s_di[PG_DW][10];                // descriptor ring: pg_coldesc's ints
    __shared__ long long s_dl[PG_DW][2];           // and its offsets
    __shared__ double s_xj[6];                     // the updated right-hand side on its way to the pivot thread
    __shared__ int s_ok;
    const int tid = threadIdx.x;
    const int bin = bin_perm[blockIdx.x];          // bins in descending order of work
    for (int q = binroot_ptr[bin]; q < binroot_ptr[bin + 1]; ++q) {        // zero the update matrices of this bin's roots
        const int ri = binroot_idx[q]; const long long b6 = 6LL * broot_b[ri]; double* U = ubin + broot_uoff[ri];
        for (long long e = threadIdx.x; e < b6 * b6 + b6; e += 256) U[e] = 0.0;
    }
    const int ci0 = binptr[bin], ci_end = binptr[bin + 1];
    if (ci0 >= ci_end) return;
    // descriptors of cnt columns from column index base on: one thread per column, so the three dependent look-ups are paid once per 32 columns and not per column
    auto fill = [&](int base, int cnt) {
        if (tid < cnt) {
            const int ci = base + tid, j = bincols[ci];
            const int c0 = colptr[j], m = colptr[j + 1] - c0, t0 = rlptr[j], T = rlptr[j + 1] - t0, ri = broot_of_col[j];
            int fpos = -1, c0p = 0;
            if (ci > ci0 && T > 0) {                            // is the column before it in the bin its last source?
                const int jp = bincols[ci - 1];
                if (rlcol[t0 + T - 1] == jp) { c0p = colptr[jp]; fpos = rlpos[t0 + T - 1] - c0p; }
            }
            int* d = s_di[(ci - ci0) & (PG_DW - 1)];
            d[0] = j; d[1] = c0; d[2] = m; d[3] = t0; d[4] = T; d[5] = anc_first[j]; d[6] = ri; d[7] = ri >= 0 ? 6 * broot_b[ri] : 0; d[8] = fpos; d[9] = c0p;
            long long* dl = s_dl[(ci - ci0) & (PG_DW - 1)];
            dl[0] = mapptr[j]; dl[1] = ri >= 0 ? broot_uoff[ri] : 0;
        }
    };
    auto desc = [&](int ci) {                                   // (the same on every thread: kept in scalar registers)
        const int* d = s_di[(ci - ci0) & (PG_DW - 1)]; const long long* dl = s_dl[(ci - ci0) & (PG_DW - 1)];
        pg_coldesc k;
        k.j = __builtin_amdgcn_readfirstlane(d[0]); k.c0 = __builtin_amdgcn_readfirstlane(d[1]); k.m = __builtin_amdgcn_readfirstlane(d[2]);
        k.t0 = __builtin_amdgcn_readfirstlane(d[3]); k.T = __builtin_amdgcn_readfirstlane(d[4]); k.af = __builtin_amdgcn_readfirstlane(d[5]);
        k.ri = __builtin_amdgcn_readfirstlane(d[6]); k.b6 = __builtin_amdgcn_readfirstlane(d[7]); k.fpos = __builtin_amdgcn_readfirstlane(d[8]);
        k.c0p = __builtin_amdgcn_readfirstlane(d[9]);
        const long long mo = dl[0], uo = dl[1];
        k.mapoff = ((long long)__builtin_amdgcn_readfirstlane((int)(mo >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)mo);
        k.uoff = ((long long)__builtin_amdgcn_readfirstlane((int)(uo >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)uo);
        return k;
    };
    // column k's terms of its root's update matrix and right-hand side, from s_col, sy = s_y[parity of k], sa = s_arel[parity of k]: one term per entry and column
    auto u_update = [&](const pg_coldesc& k, const double* sy, const int* sa) {
        const int ta = k.m - k.af;                              // block rows beyond the subtree root (a suffix of the column)
        if (k.ri < 0 || ta <= 0) return;
        const int b6 = k.b6;
        double* __restrict__ U = ubin + k.uoff;
        double* __restrict__ g = U + (size_t)b6 * b6;
        const double* sL = s_col + k.af * 36;
        if (tid < 6 * ta) {                                     // right-hand side: g[ia] -= L_a y_j
            const int pa = tid / 6, a = tid - pa * 6;
            const double* La = sL + pa * 36 + a * 6;
            g[sa[pa] * 6 + a] -= La[0] * sy[0] + La[1] * sy[1] + La[2] * sy[2] + La[3] * sy[3] + La[4] * sy[4] + La[5] * sy[5];
        }
        const int npair = ta * (ta + 1) / 2;                    // U[ia][ib] -= L_a L_b^T for the block pairs ib <= ia
        // a thread takes row a of a block pair, six adjacent entries: the index arithmetic and the row of L_a once per six terms, six loads of U in flight
        // (entry by entry this pass was the serial form's largest section in the longest C3 bin, 6 700 of a column's 20 800 cycles, and none of it waiting)
        for (int it = tid; it < 6 * npair; it += 256) {
            const int pr = it / 6, a = it - 6 * pr;
            int pa = (int)((sqrtf(8.0f * (float)pr + 1.0f) - 1.0f) * 0.5f);      // pr = pa (pa + 1) / 2 + pb, pb <= pa
            while (pa * (pa + 1) / 2 > pr) --pa;
            while ((pa + 1) * (pa + 2) / 2 <= pr) ++pa;
            const int pb = pr - pa * (pa + 1) / 2;
            const double* La = sL + pa * 36 + a * 6;
            double* Ur = U + (size_t)(sa[pa] * 6 + a) * b6 + sa[pb] * 6;
            double old[6];
#pragma unroll
            for (int b = 0; b < 6; ++b) old[b] = Ur[b];
            const double la[6] = { La[0], La[1], La[2], La[3], La[4], La[5] };
#pragma unroll
            for (int b = 0; b < 6; ++b) {
                const double* Lb = sL + pb * 36 + b * 6;
                Ur[b] = old[b] - (la[0] * Lb[0] + la[1] * Lb[1] + la[2] * Lb[2] + la[3] * Lb[3] + la[4] * Lb[4] + la[5] * Lb[5]);
            }
        }
    };
    fill(ci0, min(PG_DW, ci_end - ci0));
    __syncthreads();
    const int q = tid / 6, r = tid - q * 6;                     // the thread's block row and row of it, in every column; also its staged block and row
    const bool rhs = tid >= 250;                                // the right-hand side's six lanes; the first of them is the pivot thread
    const int rs_ = rhs ? tid - 250 : 0;
    pg_coldesc cur = desc(ci0), prv = cur;
    // the first column's own loads, and the staged positions of the second (a first column has no sources: nothing of it was accumulated ahead)
    double acc[6] = { 0, 0, 0, 0, 0, 0 }, accy = 0, rowv[6] = { 0, 0, 0, 0, 0, 0 }, xa = 0;
    // None of the loads ahead hangs on a condition: a thread with nothing to fetch reads `idle` (a load behind a branch makes the compiler count the
    // loads in flight from the last one it can be sure of, and the first use of ANY earlier result then drains them all -- a round trip on the chain).
    // What such a thread read is never used: every use below is under the condition the load would have been under.
    const int* idle = bin_perm + blockIdx.x;
    int mpf = -1, arel, ip, ic;
#pragma unroll
    for (int s = 0; s < 6; ++s) rowv[s] = Lvals[(size_t)(cur.c0 + (tid < 6 * cur.m ? q : 0)) * 36 + r * 6 + s];
    xa = x[(size_t)cur.j * 6 + rs_];
    arel = *(tid < cur.m - cur.af ? anc_rel + cur.c0 + cur.af + tid : idle);
    {
        const pg_coldesc d1 = ci0 + 1 < ci_end ? desc(ci0 + 1) : cur;
        const bool st1 = ci0 + 1 < ci_end && tid < 6 * min(PG_PCH, d1.T - (d1.fpos >= 0));
        ip = *(st1 ? rlpos + d1.t0 + q : idle); ic = *(st1 ? rlcol + d1.t0 + q : idle);
    }
    for (int ci = ci0; ci < ci_end; ++ci) {
        const int par = ci & 1, rel = ci - ci0;
        const bool have1 = ci + 1 < ci_end, have2 = ci + 2 < ci_end;
        if (rel >= 32 && (rel & 31) == 0 && ci + 32 < ci_end) fill(ci + 32, min(32, ci_end - (ci + 32)));
        const pg_coldesc d1 = have1 ? desc(ci + 1) : cur;
        const int m = cur.m, c0 = cur.c0, j = cur.j;
        const bool act = tid < 6 * m;
        const int Tnf = cur.T - (cur.fpos >= 0);                // sources other than the column before
        const int* mp = upd_map + cur.mapoff;
        // ---- T1: what column ci + 1 needs, issued a column ahead
        const int Tnf1 = have1 ? d1.T - (d1.fpos >= 0) : 0, tn1 = min(PG_PCH, Tnf1);
        const bool act1 = have1 && tid < 6 * d1.m;
        const int* mp1 = upd_map + d1.mapoff;
        int mpi[PG_NIDX], mpf1, arel1, ip2, ic2;
#pragma unroll
        for (int u = 0; u < PG_NIDX; ++u) mpi[u] = *(act1 && u < tn1 ? mp1 + (size_t)u * d1.m + q : idle);
        mpf1 = *(act1 && d1.fpos >= 0 ? mp1 + (size_t)(d1.T - 1) * d1.m + q : idle);
        arel1 = *(have1 && tid < d1.m - d1.af ? anc_rel + d1.c0 + d1.af + tid : idle);
        double sv[6], syv;
        {
            const bool st1 = tid < 6 * tn1;                     // (block 0 and x_0 for the others: read, not used)
            const size_t ipc = st1 ? ip : 0, icc = st1 ? ic : 0;
#pragma unroll
            for (int s = 0; s < 6; ++s) sv[s] = Lvals[ipc * 36 + r * 6 + s];
            syv = x[icc * 6 + r];
        }
        {
            const pg_coldesc d2 = have2 ? desc(ci + 2) : cur;
            const bool st2 = have2 && tid < 6 * min(PG_PCH, d2.T - (d2.fpos >= 0));
            ip2 = *(st2 ? rlpos + d2.t0 + q : idle); ic2 = *(st2 ? rlcol + d2.t0 + q : idle);
        }
        // ---- T2: sources beyond those accumulated ahead (the first column of a bin: all of them), staged and accumulated in place
        for (int tc = ci == ci0 ? 0 : min(PG_PCH, Tnf); tc < Tnf; tc += PG_PCH) {
            const int tn = min(PG_PCH, Tnf - tc);
            __syncthreads();
            if (tid < 6 * tn) {
                const int pos = rlpos[cur.t0 + tc + q], col = rlcol[cur.t0 + tc + q];
#pragma unroll
                for (int s = 0; s < 6; ++s) s_st[par][tid * 6 + s] = Lvals[(size_t)pos * 36 + r * 6 + s];
                s_sy[par][tid] = x[(size_t)col * 6 + r];
            }
            __syncthreads();
            if (rhs)
                for (int t = 0; t < tn; ++t) {
                    const double* yk = s_sy[par] + t * 6; const double* B = s_st[par] + t * 36 + rs_ * 6;
                    accy += B[0] * yk[0] + B[1] * yk[1] + B[2] * yk[2] + B[3] * yk[3] + B[4] * yk[4] + B[5] * yk[5];
                }
            if (act) pg_acc_rows(mp + (size_t)tc * m + q, m, tn, Lvals, r, s_st[par], acc);
        }
        // ---- T3: the column before as a source, from LDS
        if (cur.fpos >= 0) {
            const double* Bf = s_col + cur.fpos * 36;
            if (rhs) {
                const double* yk = s_y[par ^ 1]; const double* B = Bf + rs_ * 6;
                accy += B[0] * yk[0] + B[1] * yk[1] + B[2] * yk[2] + B[3] * yk[3] + B[4] * yk[4] + B[5] * yk[5];
            }
            if (act && mpf >= 0) {
                const double* Lik = s_col + (mpf - cur.c0p) * 36 + r * 6;
                const double a[6] = { Lik[0], Lik[1], Lik[2], Lik[3], Lik[4], Lik[5] };
                pg_upd_term(acc, a, Bf);
            }
        }
        // ---- T4: the updated row and right-hand side; pivot rows and boundary indices to LDS
        if (rhs) s_xj[rs_] = xa - accy;                         // (accy = 0 without updates)
        if (act) {
#pragma unroll
            for (int s = 0; s < 6; ++s) rowv[s] -= acc[s];      // (no updates: acc = 0, x - 0 = x)
            if (tid < 6) { for (int s = 0; s < 6; ++s) s_diag[r * 6 + s] = rowv[s]; }
        }
        if (tid < m - cur.af) s_arel[par][tid] = arel;
        // ---- T5: the staged values of column ci + 1
        if (tid < 6 * tn1) {
#pragma unroll
            for (int s = 0; s < 6; ++s) s_st[par ^ 1][tid * 6 + s] = sv[s];
            s_sy[par ^ 1][tid] = syv;
        }
        __syncthreads();                                        // B1
        // ---- shadow: the pivot on thread 250, everything below beside it
        double acc1[6] = { 0, 0, 0, 0, 0, 0 }, accy1 = 0, rowv1[6] = { 0, 0, 0, 0, 0, 0 }, xa1 = 0;
        if (tid == 250) {                                       // the serial form's one-thread section, word for word
            double A[36], xj[6], ri[6];
#pragma unroll
            for (int a = 0; a < 36; ++a) A[a] = s_diag[a];
#pragma unroll
            for (int a = 0; a < 6; ++a) xj[a] = s_xj[a];
            const int bad = chol6_recip(A, ri);
            if (bad) *fail = 1;
            s_ok = !bad;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int b = 0; b < 6; ++b) { const double v = b <= a ? A[a * 6 + b] : 0.0; s_diag[a * 6 + b] = v; Lvals[(size_t)c0 * 36 + a * 6 + b] = v; }
#pragma unroll
            for (int a = 0; a < 6; ++a) { s_ri[a] = ri[a]; rdiag[(size_t)j * 6 + a] = ri[a]; }
            if (!bad) {
                double v[6];
#pragma unroll
                for (int a = 0; a < 6; ++a) {
                    double t = xj[a];
#pragma unroll
                    for (int b = 0; b < 6; ++b) if (b < a) t -= A[a * 6 + b] * v[b];
                    v[a] = t * ri[a];
                }
#pragma unroll
                for (int a = 0; a < 6; ++a) { x[(size_t)j * 6 + a] = v[a]; s_y[par][a] = v[a]; }
            }
        }
        if (ci > ci0) u_update(prv, s_y[par ^ 1], s_arel[par ^ 1]);
        if (tn1 > 0) {
            if (rhs)
                for (int t = 0; t < tn1; ++t) {
                    const double* yk = s_sy[par ^ 1] + t * 6; const double* B = s_st[par ^ 1] + t * 36 + rs_ * 6;
                    accy1 += B[0] * yk[0] + B[1] * yk[1] + B[2] * yk[2] + B[3] * yk[3] + B[4] * yk[4] + B[5] * yk[5];
                }
            if (act1) pg_acc_rows_ahead(mpi, mp1 + q, d1.m, tn1, Lvals, r, s_st[par ^ 1], acc1);
        }
#pragma unroll
        for (int s = 0; s < 6; ++s) rowv1[s] = Lvals[(size_t)(d1.c0 + (act1 ? q : 0)) * 36 + r * 6 + s];      // the assembled row of column ci + 1: requested here, used at its T4
        xa1 = x[(size_t)d1.j * 6 + rs_];
        __syncthreads();                                        // B2
        if (!s_ok) return;
        if (act && tid >= 6) {
            double* row = Lvals + (size_t)(c0 + q) * 36 + r * 6;
            double xr[6];
#pragma unroll
            for (int s = 0; s < 6; ++s) { double v = rowv[s];
#pragma unroll
                                          for (int c = 0; c < 6; ++c) if (c < s) v -= xr[c] * s_diag[s * 6 + c];
                                          xr[s] = v * s_ri[s]; }
            for (int s = 0; s < 6; ++s) { row[s] = xr[s]; s_col[tid * 6 + s] = xr[s]; }
        }
        __syncthreads();                                        // B3
        prv = cur; cur = d1;
#pragma unroll
        for (int s = 0; s < 6; ++s) { acc[s] = acc1[s]; rowv[s] = rowv1[s]; }
        accy = accy1; xa = xa1; mpf = mpf1; arel = arel1; ip = ip2; ic = ic2;
    }
    u_update(prv, s_y[(ci_end - 1) & 1], s_arel[(ci_end - 1) & 1]);        // the last column's terms (a failed pivot has returned above, as the serial form does before them)
}
// backward substitution through a bin, columns in descending order, one wave per bin
__global__ __launch_bounds__(64) void pg_bwd_subtree_kernel(const int* __restrict__ bin_perm, const int* __restrict__ binptr, const int* __restrict__ bincols,
                                                            const int* __restrict__ colptr, const int* __restrict__ rowidx,
                                                            const double* __restrict__ Lvals, double* __restrict__ x, const double* __restrict__ rdiag)
{
    const int lane = threadIdx.x;
    const int bin = bin_perm[blockIdx.x];
    // (round 5) column -> its pointers, and the pivot block with its reciprocals -- nothing of which depends on the solution so far -- are
    // fetched one column ahead of the chain (x of the ancestors -> sums -> the 6 x 6 back-substitution -> x of the column)
    const int ci_lo = binptr[bin];
    int jn = 0, cn0 = 0, cn1 = 0;
    double ldn[36], rin[6];
    auto ahead = [&](int ci2) {
        jn = bincols[ci2]; cn0 = colptr[jn]; cn1 = colptr[jn + 1];
        if (lane == 0) {
            const double* Ld = Lvals + (size_t)cn0 * 36;
#pragma unroll
            for (int a = 0; a < 36; ++a) ldn[a] = Ld[a];
#pragma unroll
            for (int a = 0; a < 6; ++a) rin[a] = rdiag[(size_t)jn * 6 + a];
        }
    };
    if (binptr[bin + 1] - 1 >= ci_lo) ahead(binptr[bin + 1] - 1);
    for (int ci = binptr[bin + 1] - 1; ci >= ci_lo; --ci) {
        const int j = jn, c0 = cn0, c1 = cn1;
        double ld[36], ri[6];
#pragma unroll
        for (int a = 0; a < 36; ++a) ld[a] = ldn[a];
#pragma unroll
        for (int a = 0; a < 6; ++a) ri[a] = rin[a];
        if (ci - 1 >= ci_lo) ahead(ci - 1);
        double acc[6] = { 0, 0, 0, 0, 0, 0 };
        for (int p = c0 + 1 + lane; p < c1; p += 64) {
            const double* B = Lvals + (size_t)p * 36; const double* xi = x + (size_t)rowidx[p] * 6;
            for (int a = 0; a < 6; ++a) { double s = 0; for (int b = 0; b < 6; ++b) s += B[b * 6 + a] * xi[b]; acc[a] += s; }
        }
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[a] = dsss_wave_sum(acc[a]);
        if (lane == 0) {
            double v[6], xj[6];
#pragma unroll
            for (int a = 0; a < 6; ++a) xj[a] = x[(size_t)j * 6 + a];
#pragma unroll
            for (int a = 5; a >= 0; --a) { double s = xj[a] - acc[a];
#pragma unroll
                                           for (int b = 0; b < 6; ++b) if (b > a) s -= ld[b * 6 + a] * v[b];
                                           v[a] = s * ri[a]; }
#pragma unroll
            for (int a = 0; a < 6; ++a) x[(size_t)j * 6 + a] = v[a];
        }
        __threadfence_block();
        __builtin_amdgcn_s_barrier();
    }
}

// the instances the driver launches (the templates are declared in dsss_pg_kernels.h)
template __global__ void pg_scan_block_kernel<int, 0>(int, const int* __restrict__, const int* __restrict__, int* __restrict__, int* __restrict__);
template __global__ void pg_scan_block_kernel<long long, 1>(int, const int* __restrict__, const int* __restrict__, long long* __restrict__, long long* __restrict__);
template __global__ void pg_scan_tops_kernel<int>(int, int* __restrict__, int* __restrict__);
template __global__ void pg_scan_tops_kernel<long long>(int, long long* __restrict__, long long* __restrict__);
template __global__ void pg_scan_add_kernel<int>(int, int* __restrict__, const int* __restrict__, const int* __restrict__);
template __global__ void pg_scan_add_kernel<long long>(int, long long* __restrict__, const long long* __restrict__, const long long* __restrict__);

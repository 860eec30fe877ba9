// diasss_amd/csrc/dsss_quadtree.hip -- K4: ORBextractor::DistributeOctTree on the device, one workgroup per
// (frame, pyramid level).  Restates /root/reference/thirdparty/ORBextractor.cpp:481-763 without the std::list:
//
//   * a node's keypoints are a contiguous segment of a key array; DivideNode is a STABLE 4-way partition of that
//     segment (one wave per node, ballot ranks), children living in the other of two ping-pong key buffers;
//   * the list is an array in list order.  "push_front the non-empty children, erase the parent" over a whole pass
//     (:606-665) gives  new list = reverse(children in creation order) ++ old leaves;  the size-ordered refinement
//     (:676-737) processes the expandable children of the previous round by descending (size, creation order),
//     stops at the first point where the node count reaches the quota (the reference's `break`), and gives
//     new list = reverse(children created this round) ++ (old list minus the divided parents);
//   * ties in the size sort use creation order (the reference compares heap addresses; same rule as the oracle and
//     the host routine in quadtree.cpp);
//   * nIni = max(1, round(w/h)) (the reference divides by zero for tall levels), as the oracle and quadtree.cpp have it: qt_n_roots.
// Output: the kept candidate of every node (first maximum response in key order), in list order.
// The rules of the tree that the host twin shares (roots, midpoint, quadrant, child boxes, the work area) are in dsss_quadtree.h.
#include "dsss_internal.h"
#include "dsss_quadtree.h"
#include "dsss_wave.h"

// The workgroup of one (frame, level) instance: sixteen wavefronts.  The passes stream the level's whole key segment several times
// and the first passes have a handful of nodes, so the time of the kernel is the time of ONE workgroup on the largest level: four
// wavefronts took 3 ms per launch.
#define QT_THREADS 1024
#define QT_WAVES (QT_THREADS / 64)
#define QT_RANK_CAP 4096                           // expandable nodes whose (size, id) pairs fit the LDS staging of the rank pass
// qnode::leaf: bit 0 = the node holds one key; for the nodes of a PRE-SORTED level (qt_presort) bits 4..6 = depth and
// bits 8.. = the path code (two bits per level), which is also where the node's keys start in the sorted array
#define QT_SORT_DEPTH 6                            // deepest pre-sort: the bucket tables hold one entry per path code of that depth
#define QT_BUCKET_CAP (1 << (2 * QT_SORT_DEPTH))
static_assert(QT_SORT_DEPTH <= 7, "qnode::leaf keeps three bits of depth");
static_assert(QT_BUCKET_CAP <= 4 * QT_THREADS, "the scan of the bucket sizes takes four buckets per thread");
__device__ inline int qt_leaf_depth(int leaf) { return (leaf >> 4) & 7; }
__device__ inline int qt_leaf_path(int leaf) { return leaf >> 8; }
__device__ inline int qt_leaf_of(int kcnt, int depth, int path) { return (kcnt == 1) | (depth << 4) | (path << 8); }

// A key carries the candidate's coordinates (integers: FAST cell offset + position in the cell) next to its index, so
// DivideNode streams the key segment and never gathers xs / ys.
typedef unsigned long long qkey;
#define QT_NOKEY (~0ull)
// The response rides along (FAST scores are integers below 256, the index keeps 24 bits): the point kept per node is then found
// from the keys alone.   key = y << 48 | x << 32 | response << 24 | index
__device__ inline qkey qt_make_key(int idx, float x, float y, float resp) { return ((qkey)(unsigned)(int)y << 48) | ((qkey)((unsigned)(int)x & 0xffffu) << 32) | ((qkey)((unsigned)(int)resp & 0xffu) << 24) | (qkey)((unsigned)idx & 0xffffffu); }
__device__ inline float qt_key_x(qkey k) { return (float)(int)((k >> 32) & 0xffffull); }
__device__ inline float qt_key_y(qkey k) { return (float)(int)(k >> 48); }
// what the kept point of a node maximises: larger = higher response, then smaller index
__device__ inline unsigned qt_rank(unsigned resp, unsigned idx) { return (resp & 0xffu) << 24 | (0xffffffu - (idx & 0xffffffu)); }
__device__ inline unsigned qt_key_rank(qkey k) { return qt_rank((unsigned)(k >> 24), (unsigned)k); }
__device__ inline int qt_rank_idx(unsigned rank) { return (int)(0xffffffu - (rank & 0xffffffu)); }
// path code of a point after D levels of DivideNode starting from the root box (0, 0, W, H): two bits per level, n1..n4 = 0..3
__device__ inline int qt_code(float x, float y, int W, int H, int D)
{
    qt_box b = { 0, 0, W, H };
    int code = 0;
    for (int l = 0; l < D; ++l) {
        const int c = qt_quadrant(x, y, (float)qt_mid(b.x0, b.x1), (float)qt_mid(b.y0, b.y1));
        code = (code << 2) | c;
        b = qt_child_box(b, c);
    }
    return code;
}

struct qt_lds {
    __attribute__((aligned(16))) int rank[2 * QT_RANK_CAP];      // refinement: (size, id) pairs
    int cnt[QT_WAVES][4];                          // qt_divide_block: counts per wave and class
    int w[QT_WAVES];                               // the block scans          (16-byte aligned down to here: read four at a time)
    unsigned best[QT_BUCKET_CAP];                  // per bucket: the best qt_rank of its keys; the cursors of the key scatter once keys are needed
    int off[QT_BUCKET_CAP + 1];                    // bucket offsets of the D-level path codes (kept to the end: every division above depth D reads its children's sizes here)
    int S, pool, nexp, done, phase2, t, have_keys; // nodes in the list, nodes in the pool, expandable children of the last round, ...
};
// one instance: its candidates, keys and work area, the tree's constants and the workgroup's LDS
struct qt_tree {
    const float *xs, *ys, *rs; int base, n;        // the level's candidates
    qkey *keys0, *keys1;                           // frame-wide key arrays, this level's segment
    qnode* pool; int *L, *Ln, *parents, *expv, *order, *pcnt;
    int W, H, N, nIni, D;                          // FAST range, quota, roots, pre-sort depth (0: none)
    int list_cap, pool_cap; int* err;
    qt_lds& s;
};

// f(i, x, y, response) on every candidate of the level, QT_CAND_ILP candidates in flight per thread
#define QT_CAND_ILP 8
template <class F> __device__ __forceinline__ void qt_for_candidates(const qt_tree& T, F f)
{
    const float* __restrict__ xs = T.xs; const float* __restrict__ ys = T.ys; const float* __restrict__ rs = T.rs;
    const int n = T.n;
    for (int i0 = threadIdx.x; i0 < n; i0 += QT_CAND_ILP * QT_THREADS) {
        float x8[QT_CAND_ILP], y8[QT_CAND_ILP], r8[QT_CAND_ILP];
#pragma unroll
        for (int u = 0; u < QT_CAND_ILP; ++u) { const int i = min(i0 + u * QT_THREADS, n - 1); x8[u] = xs[i]; y8[u] = ys[i]; r8[u] = rs[i]; }      // (unconditional: a load under `i < n` waits for the one before it)
#pragma unroll
        for (int u = 0; u < QT_CAND_ILP; ++u) { const int i = i0 + u * QT_THREADS; if (i < n) f(i, x8[u], y8[u], r8[u]); }
    }
}

// ---- ExtractorNode::DivideNode (:481-537): stable 4-way partition of a node's key segment from its buffer into the other
// one; cnt[0..3] = keys of n1..n4 (top-left, top-right, bottom-left, bottom-right).  The key -> coordinate loads are
// streamed with QT_ILP chunks of 64 keys in flight per wave: a pass over the level costs (keys / (1024 x QT_ILP)) round trips.
#define QT_ILP 8
struct qt_division { const qkey* src; qkey* dst; float mx, my; };
__device__ __forceinline__ qt_division qt_division_of(const qt_tree& T, const qnode& P)
{
    const qt_division d = { P.buf ? T.keys1 : T.keys0, P.buf ? T.keys0 : T.keys1, (float)qt_mid(P.box.x0, P.box.x1), (float)qt_mid(P.box.y0, P.box.y1) };
    return d;
}
__device__ inline void qt_classify4(const qt_division& d, int beg, int end, int b, int lane, int* c, qkey* k)
{
#pragma unroll
    for (int u = 0; u < QT_ILP; ++u) { const int i = b + u * 64 + lane; k[u] = i < end ? d.src[beg + i] : QT_NOKEY; }
#pragma unroll
    for (int u = 0; u < QT_ILP; ++u) c[u] = k[u] != QT_NOKEY ? qt_quadrant(qt_key_x(k[u]), qt_key_y(k[u]), d.mx, d.my) : -1;
}
// counts of the four classes over keys [lo, hi) of the node (one wave)
__device__ inline void qt_count_range(const qnode& P, const qt_division& d, int lo, int hi, int* cnt)
{
    const int lane = threadIdx.x & 63;
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    for (int b = lo; b < hi; b += 64 * QT_ILP) {
        int c[QT_ILP]; qkey k[QT_ILP];
        qt_classify4(d, P.kbeg, hi, b, lane, c, k);
#pragma unroll
        for (int u = 0; u < QT_ILP; ++u) {
            c0 += __popcll(__ballot(c[u] == 0)); c1 += __popcll(__ballot(c[u] == 1)); c2 += __popcll(__ballot(c[u] == 2)); c3 += __popcll(__ballot(c[u] == 3));
        }
    }
    cnt[0] = c0; cnt[1] = c1; cnt[2] = c2; cnt[3] = c3;
}
// stable scatter of keys [lo, hi) given the destination offset of each class for this range (one wave)
__device__ inline void qt_scatter_range(const qnode& P, const qt_division& d, int lo, int hi, const int* off)
{
    const int lane = threadIdx.x & 63;
    int r0 = off[0], r1 = off[1], r2 = off[2], r3 = off[3];
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int b = lo; b < hi; b += 64 * QT_ILP) {
        int c[QT_ILP]; qkey k[QT_ILP];
        qt_classify4(d, P.kbeg, hi, b, lane, c, k);
#pragma unroll
        for (int u = 0; u < QT_ILP; ++u) {
            const unsigned long long m0 = __ballot(c[u] == 0), m1 = __ballot(c[u] == 1), m2 = __ballot(c[u] == 2), m3 = __ballot(c[u] == 3);
            if (c[u] == 0) d.dst[P.kbeg + r0 + __popcll(m0 & below)] = k[u];
            else if (c[u] == 1) d.dst[P.kbeg + r1 + __popcll(m1 & below)] = k[u];
            else if (c[u] == 2) d.dst[P.kbeg + r2 + __popcll(m2 & below)] = k[u];
            else if (c[u] == 3) d.dst[P.kbeg + r3 + __popcll(m3 & below)] = k[u];
            r0 += __popcll(m0); r1 += __popcll(m1); r2 += __popcll(m2); r3 += __popcll(m3);
        }
    }
}
// one node, one wave
__device__ inline void qt_divide_wave(const qt_tree& T, const qnode& P, int* cnt)
{
    const qt_division d = qt_division_of(T, P);
    qt_count_range(P, d, 0, P.kcnt, cnt);
    const int off[4] = { 0, cnt[0], cnt[0] + cnt[1], cnt[0] + cnt[1] + cnt[2] };
    qt_scatter_range(P, d, 0, P.kcnt, off);
}
// one node, the whole workgroup (the first passes have fewer nodes than waves, and those nodes hold most of the keys):
// every wave takes a contiguous share of the segment; s.cnt[wave][class] carries the counts between the two passes
__device__ inline void qt_divide_block(const qt_tree& T, const qnode& P, int* cnt)
{
    const qt_division d = qt_division_of(T, P);
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = ((P.kcnt + QT_WAVES - 1) / QT_WAVES + 63) & ~63;
    const int lo = min(wv * q, P.kcnt), hi = min(lo + q, P.kcnt);
    int mine[4];
    qt_count_range(P, d, lo, hi, mine);
    if (lane == 0) { T.s.cnt[wv][0] = mine[0]; T.s.cnt[wv][1] = mine[1]; T.s.cnt[wv][2] = mine[2]; T.s.cnt[wv][3] = mine[3]; }
    __syncthreads();
    int off[4], run = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        int before = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < QT_WAVES; ++w) { const int t = T.s.cnt[w][c]; if (w < wv) before += t; tot += t; }
        off[c] = run + before; cnt[c] = tot; run += tot;
    }
    qt_scatter_range(P, d, lo, hi, off);
    __syncthreads();
}
// child c of P given the sizes of the four; from_buckets: a child of a pre-sorted node above the sort depth, whose keys are a range of the sorted array
__device__ inline qnode qt_child(const qnode& P, int c, const int* cnt, bool from_buckets)
{
    qnode q;
    q.box = qt_child_box(P.box, c);
    int off = 0;
    for (int k = 0; k < c; ++k) off += cnt[k];
    q.kbeg = P.kbeg + off; q.kcnt = cnt[c]; q.buf = from_buckets ? 1 : P.buf ^ 1;
    q.leaf = from_buckets ? qt_leaf_of(cnt[c], qt_leaf_depth(P.leaf) + 1, (qt_leaf_path(P.leaf) << 2) | c) : qt_leaf_of(cnt[c], 0, 0);
    return q;
}

// ---- the steps of a round (a whole-list pass or a round of the refinement).  Workgroup-uniform calls only.
__device__ __forceinline__ void qt_store_counts(const qt_tree& T, int r, const int* cnt)
{
    T.pcnt[4 * r] = cnt[0]; T.pcnt[4 * r + 1] = cnt[1]; T.pcnt[4 * r + 2] = cnt[2]; T.pcnt[4 * r + 3] = cnt[3];
}
// the sorted key array, on demand: counting-sort scatter by the D-level code into keys1 (the second pass of the pre-sort)
__device__ __forceinline__ void qt_ensure_keys(const qt_tree& T)
{
    if (T.s.have_keys) return;
    const int nb = 1 << (2 * T.D);
    int* cur = reinterpret_cast<int*>(T.s.best);      // (the bucket maxima are gone from here on: the kept points come from the keys)
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += QT_THREADS) cur[i] = T.s.off[i];
    __syncthreads();
    qt_for_candidates(T, [&](int i, float x, float y, float r) { T.keys1[atomicAdd(&cur[qt_code((float)(int)x, (float)(int)y, T.W, T.H, T.D)], 1)] = qt_make_key(i, x, y, r); });
    __syncthreads();
    if (threadIdx.x == 0) T.s.have_keys = 1;
    __syncthreads();
}
// sizes of the children of nodes ids[0 .. m) -> pcnt, three ways.  From the bucket offsets: the nodes sit above the sort depth of a
// pre-sorted level, nothing is streamed
__device__ __forceinline__ void qt_sizes_from_buckets(const qt_tree& T, const int* ids, int m)
{
    for (int r = threadIdx.x; r < m; r += QT_THREADS) {
        const int lf = T.pool[ids[r]].leaf, pf = qt_leaf_path(lf), sh = 2 * (T.D - qt_leaf_depth(lf) - 1);
        int cnt[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) { const int cp = (pf << 2) | c; cnt[c] = T.s.off[(cp + 1) << sh] - T.s.off[cp << sh]; }
        qt_store_counts(T, r, cnt);
    }
}
// by dividing them on the keys, the workgroup on one node at a time
__device__ __forceinline__ void qt_divide_by_block(const qt_tree& T, const int* ids, int m)
{
    for (int r = 0; r < m; ++r) {
        int cnt[4];
        qt_divide_block(T, T.pool[ids[r]], cnt);
        if (threadIdx.x == 0) qt_store_counts(T, r, cnt);
    }
}
// or a wave a node
__device__ __forceinline__ void qt_divide_by_wave(const qt_tree& T, const int* ids, int m)
{
    for (int r = threadIdx.x >> 6; r < m; r += QT_WAVES) {
        int cnt[4];
        qt_divide_wave(T, T.pool[ids[r]], cnt);
        if ((threadIdx.x & 63) == 0) qt_store_counts(T, r, cnt);
    }
}
// the pool holds the children of m more parents
__device__ __forceinline__ bool qt_pool_has_room(const qt_tree& T, int m)
{
    if (T.s.pool + 4 * m <= T.pool_cap) return true;
    if (threadIdx.x == 0) *T.err = QT_E_POOL;
    return false;
}
// the children of parents ids[0 .. m), sizes in pcnt, appended to the pool in creation order: parents in the order given, n1..n4,
// empty ones skipped; the parents are erased (:660,728) and the children that can still divide listed in expv.  Cn children, nexp in expv
__device__ __forceinline__ void qt_make_children(const qt_tree& T, const int* ids, int m, bool from_buckets, int& Cn, int& nexp)
{
    const int pool0 = T.s.pool;
    Cn = 0; nexp = 0;
    for (int b = 0; b < m; b += QT_THREADS) {
        const int r = b + threadIdx.x;
        int ne = 0, nx = 0, cnt[4] = { 0, 0, 0, 0 };
        if (r < m) for (int c = 0; c < 4; ++c) { cnt[c] = T.pcnt[4 * r + c]; ne += cnt[c] > 0; nx += cnt[c] > 1; }
        int te, tx;
        const int qe = dsss_block_scan_excl<QT_WAVES, int>(ne, &te, T.s.w), qx = dsss_block_scan_excl<QT_WAVES, int>(nx, &tx, T.s.w);
        if (r < m) {
            const qnode P = T.pool[ids[r]];
            int q = pool0 + Cn + qe, x = nexp + qx;
            for (int c = 0; c < 4; ++c) if (cnt[c] > 0) {
                T.pool[q] = qt_child(P, c, cnt, from_buckets);
                if (cnt[c] > 1) T.expv[x++] = q;
                ++q;
            }
            T.pool[ids[r]].kcnt = -1;
        }
        Cn += te; nexp += tx;
    }
    __syncthreads();
}
// new list = reverse(the Cn children just made) ++ the old list of S nodes without the erased parents, then the round's verdict
// (:667-672,733-735): done at the quota or when nothing divided, the refinement once three more nodes per expandable child could
// pass the quota.  false: the list is full
__device__ __forceinline__ bool qt_finish_round(qt_tree& T, int S, int Cn, int nexp)
{
    const int pool0 = T.s.pool;
    int kept = 0;
    for (int b = 0; b < S; b += QT_THREADS) {
        const int i = b + threadIdx.x;
        const int id = i < S ? T.L[i] : -1;
        const int keep = (id >= 0 && T.pool[id].kcnt >= 0) ? 1 : 0;
        int tk;
        const int rk = dsss_block_scan_excl<QT_WAVES, int>(keep, &tk, T.s.w);
        if (keep) { if (Cn + kept + rk < T.list_cap) T.Ln[Cn + kept + rk] = id; }
        kept += tk;
    }
    const int Snew = Cn + kept;
    if (Snew > T.list_cap) {                           // (the old list holds erased nodes: nothing is emitted)
        if (threadIdx.x == 0) { *T.err = QT_E_LIST; T.s.S = 0; }
        return false;
    }
    for (int i = threadIdx.x; i < Cn; i += QT_THREADS) T.Ln[Cn - 1 - i] = pool0 + i;      // push_front order
    __syncthreads();
    if (threadIdx.x == 0) {
        T.s.pool = pool0 + Cn; T.s.nexp = nexp; T.s.S = Snew;
        if (Snew >= T.N || Snew == S) T.s.done = 1;
        else if (Snew + nexp * 3 > T.N) T.s.phase2 = 1;
    }
    { int* t = T.L; T.L = T.Ln; T.Ln = t; }
    __syncthreads();
    return true;
}

// ---- initial nodes (:543-585)
__device__ __forceinline__ void qt_roots(qt_tree& T)
{
    const int lane = threadIdx.x & 63;
    const float hX = qt_root_width(T.W, T.nIni);      // nIni is never clamped from above: make_layout sizes pool, lists and pcnt for the level's roots
    if (T.nIni == 1) {
        if (T.N <= 1)                                // (with a quota above one the pre-sort writes the keys, and only on demand)
            qt_for_candidates(T, [&](int i, float x, float y, float r) { T.keys0[i] = qt_make_key(i, x, y, r); });
    }
    else if (threadIdx.x < 64) {                     // stable partition of 0..n-1 by root index, one wave
        int off = 0;
        for (int r = 0; r < T.nIni; ++r) {
            int run = 0;
            for (int b = 0; b < T.n; b += 64) {
                const int i = b + lane;
                const bool in = i < T.n && qt_root_of(T.xs[i], hX, T.nIni) == r;
                const unsigned long long m = __ballot(in);
                if (in) T.keys0[off + run + __popcll(m & ((1ull << lane) - 1ull))] = qt_make_key(i, T.xs[i], T.ys[i], T.rs[i]);
                run += __popcll(m);
            }
            if (lane == 0) T.pcnt[r] = run;
            off += run;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int S = 0, off = 0;
        for (int r = 0; r < T.nIni; ++r) {
            const int c = T.nIni == 1 ? T.n : T.pcnt[r];
            qnode q; q.box = qt_root_box(r, hX, T.H);
            q.kbeg = off; q.kcnt = c; q.buf = 0; q.leaf = qt_leaf_of(c, 0, 0);
            off += c;
            T.pool[r] = q;
            if (c > 0) T.L[S++] = r;                // empty roots are erased (:581-582)
        }
        T.s.S = S; T.s.pool = T.nIni; T.s.done = 0; T.s.phase2 = 0; T.s.nexp = 0; T.s.have_keys = 1;
    }
    __syncthreads();
}

// ---- PRE-SORT.  The whole-list passes divide every node of the list, so after p of them the keys are bucket-sorted by
// their p-level path code.  With one root the code of a key follows from its coordinates alone (the boxes of DivideNode are a
// function of the path), so ONE counting sort by the D-level code replaces the first D passes, each of which streamed the
// level's keys twice and wrote them once through the single compute unit this workgroup runs on (the kernel's bound).  The
// passes keep their node bookkeeping and read the children's sizes from the bucket offsets.  Sorting deeper than the passes
// go is harmless: a node's keys are a contiguous range whatever their order inside it, and the point kept per node is picked
// by (response, candidate index), not by position.
// The keys themselves are NOT written unless a division below depth D turns up.  Everything the tree needs
// above depth D is the SIZE of a bucket range, and the point a node keeps is the maximum of (response, smallest index) over its
// buckets -- both come out of ONE pass over the candidates (LDS histogram + LDS atomicMax).  A level-0 instance of a 2000 x 1024
// frame (92 k candidates, quota 501: sorted to depth 5, divided to depth 5) read its candidates twice, wrote 8-byte keys, streamed
// them twice more and wrote them again in the size-ordered round, and read them once more for the kept points -- through the one
// compute unit it runs on; now it reads them once.  qt_ensure_keys is the second pass, run on demand.
__device__ __forceinline__ void qt_presort(qt_tree& T)
{
    if (T.nIni == 1) { int cells = 1; while (cells < T.N && T.D < QT_SORT_DEPTH) { cells *= 4; ++T.D; } }
    if (T.D == 0) return;
    const int nb = 1 << (2 * T.D);
    for (int i = threadIdx.x; i <= nb; i += QT_THREADS) { T.s.off[i] = 0; if (i < nb) T.s.best[i] = 0u; }
    __syncthreads();
    qt_for_candidates(T, [&](int i, float x, float y, float r) {
        const int code = qt_code((float)(int)x, (float)(int)y, T.W, T.H, T.D);
        atomicAdd(&T.s.off[code], 1);
        atomicMax(&T.s.best[code], qt_rank((unsigned)(int)r, (unsigned)i));
    });
    __syncthreads();
    {   // exclusive scan of the nb bucket sizes, four consecutive buckets per thread
        const int b0 = 4 * threadIdx.x;
        int v[4], sum = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) { v[u] = b0 + u < nb ? T.s.off[b0 + u] : 0; sum += v[u]; }
        int tot;
        int run = dsss_block_scan_excl<QT_WAVES, int>(sum, &tot, T.s.w);
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; ++u) if (b0 + u < nb) { T.s.off[b0 + u] = run; run += v[u]; }
        if (threadIdx.x == 0) T.s.off[nb] = T.n;
    }
    if (threadIdx.x == 0) { T.pool[0].buf = 1; T.s.have_keys = 0; }        // the root's keys are the sorted array (once it exists)
    __syncthreads();
}

// ---- whole-list passes (:594-672)
__device__ __forceinline__ void qt_whole_list_passes(qt_tree& T)
{
    for (int pass = 0; !(T.s.done || T.s.phase2); ++pass) {
        const int S = T.s.S;
        int np = 0;                                  // non-leaf nodes in list order -> parents[]
        for (int b = 0; b < S; b += QT_THREADS) {
            const int i = b + threadIdx.x;
            const int isp = (i < S && !(T.pool[T.L[i]].leaf & 1)) ? 1 : 0;
            int tp;
            const int rp = dsss_block_scan_excl<QT_WAVES, int>(isp, &tp, T.s.w);
            if (isp) T.parents[np + rp] = T.L[i];
            np += tp;
        }
        __syncthreads();
        if (np == 0 || !qt_pool_has_room(T, np)) return;      // (np == 0: every node holds one point, size == prevSize)
        const bool from_buckets = pass < T.D;        // the parents of this pass sit at depth `pass`: above the sort depth their children are bucket ranges
        if (from_buckets) qt_sizes_from_buckets(T, T.parents, np);
        else {
            qt_ensure_keys(T);
            if (np < QT_WAVES) qt_divide_by_block(T, T.parents, np); else qt_divide_by_wave(T, T.parents, np);
        }
        __syncthreads();
        int Cn, nexp;
        qt_make_children(T, T.parents, np, from_buckets, Cn, nexp);
        if (!qt_finish_round(T, S, Cn, nexp)) return;
    }
}

// descending (size, creation order) of the m nodes at(0 .. m) = (size, id): order[rank] = id
template <class F> __device__ __forceinline__ void qt_rank_nodes(const qt_tree& T, int m, F at)
{
    for (int e = threadIdx.x; e < m; e += QT_THREADS) {
        const int2 me = at(e);
        int rank = 0;
        for (int f = 0; f < m; ++f) { const int2 o = at(f); rank += (o.x > me.x) || (o.x == me.x && o.y > me.y); }
        T.order[rank] = me.y;
    }
}
// ---- size-ordered refinement (:673-738)
__device__ __forceinline__ void qt_refine(qt_tree& T)
{
    while (T.s.phase2 && !T.s.done) {
        const int S = T.s.S, m = T.s.nexp;
        if (m == 0 || !qt_pool_has_room(T, m)) return;
        // processing order.  The m x m comparison runs on (size, id) pairs staged in LDS when they fit: straight from the node pool
        // every comparison is two dependent global loads (0.6 ms per round at m = 600)
        const auto from_pool = [&](int e) { const int id = T.expv[e]; return make_int2(T.pool[id].kcnt, id); };
        if (m <= QT_RANK_CAP) {
            int2* staged = reinterpret_cast<int2*>(T.s.rank);
            for (int e = threadIdx.x; e < m; e += QT_THREADS) staged[e] = from_pool(e);
            __syncthreads();
            qt_rank_nodes(T, m, [&](int e) { return staged[e]; });
        } else qt_rank_nodes(T, m, from_pool);
        __syncthreads();
        // the nodes of a round were created together: when they sit above depth D (a pre-sorted level) their children are bucket ranges
        // and nothing is streamed; otherwise every one of them is divided on the keys (only the first t + 1 take effect)
        bool from_buckets = false;
        if (!T.s.have_keys) {
            int deep = 0;
            for (int e = threadIdx.x; e < m; e += QT_THREADS) deep |= qt_leaf_depth(T.pool[T.order[e]].leaf) >= T.D;
            from_buckets = __syncthreads_or(deep) == 0;
        }
        if (from_buckets) qt_sizes_from_buckets(T, T.order, m);
        else { qt_ensure_keys(T); qt_divide_by_wave(T, T.order, m); }      // (a wave a node however few: the nodes of a refinement are small)
        if (threadIdx.x == 0) T.s.t = m - 1;
        __syncthreads();
        // running node count; the reference breaks once it reaches the quota (:730-731)
        int run = S;
        for (int b = 0; b < m; b += QT_THREADS) {
            const int r = b + threadIdx.x;
            int d = 0;
            if (r < m) { for (int c = 0; c < 4; ++c) d += T.pcnt[4 * r + c] > 0; d -= 1; }
            int td;
            const int ex = dsss_block_scan_excl<QT_WAVES, int>(d, &td, T.s.w);
            if (r < m && run + ex + d >= T.N) atomicMin(&T.s.t, r);
            run += td;
            __syncthreads();
        }
        __syncthreads();
        int Cn, nexp;
        qt_make_children(T, T.order, T.s.t + 1, from_buckets, Cn, nexp);      // parents order[0..t] are divided
        if (!qt_finish_round(T, S, Cn, nexp)) return;
    }
}

// ---- retain the best point of each node, list order (:741-760): first maximum response in key order.  One wavefront per node.
// The keys of a node are in candidate order in the reference (stable partitions): its "first maximum" = the smallest candidate
// index among the maxima = the largest qt_rank.  Where no key was ever written a node is a range of buckets, its point the best of their maxima
__device__ __forceinline__ void qt_emit(const qt_tree& T, int* out, int* out_n, int out_cap)
{
    const int lane = threadIdx.x & 63, S = T.s.S;
    const bool have_keys = T.s.have_keys;
    for (int i = threadIdx.x >> 6; i < S; i += QT_WAVES) {
        const qnode q = T.pool[T.L[i]];
        unsigned best = 0;
        if (have_keys) {
            const qkey* kk = (q.buf ? T.keys1 : T.keys0) + q.kbeg;
            for (int k = lane; k < q.kcnt; k += 64) best = max(best, qt_key_rank(kk[k]));
        } else {
            const int sh = 2 * (T.D - qt_leaf_depth(q.leaf)), b1 = (qt_leaf_path(q.leaf) + 1) << sh;
            for (int k = (qt_leaf_path(q.leaf) << sh) + lane; k < b1; k += 64) best = max(best, T.s.best[k]);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) best = max(best, (unsigned)__shfl_xor((int)best, o, 64));
        if (lane == 0 && i < out_cap) out[i] = T.base + qt_rank_idx(best);
    }
    if (threadIdx.x == 0) { *out_n = S < out_cap ? S : out_cap; if (S > out_cap) *T.err = QT_E_OUT; }
}

__global__ __launch_bounds__(QT_THREADS) void quadtree_kernel(const qt_inst* __restrict__ tab)
{
    __shared__ qt_lds s;
    const qt_inst I = tab[blockIdx.x];
    const int base = I.offs[I.cell_begin];
    const int n = min(I.offs[I.cell_end], I.cand_cap) - base;         // never index past the candidate arrays (the overflow itself is flagged by scan_counts_kernel)
    if (n <= 0) { if (threadIdx.x == 0) *I.out_n = 0; return; }
    if (n >= (1 << 24)) { if (threadIdx.x == 0) { *I.out_n = 0; *I.err = QT_E_INDEX; } return; }
    const qt_work wk = qt_work_layout(I.pool_cap, I.list_cap);
    qt_tree T = { I.xs + base, I.ys + base, I.rs + base, base, n, I.keys0 + base, I.keys1 + base,
                  reinterpret_cast<qnode*>(I.work + wk.pool), I.work + wk.listA, I.work + wk.listB, I.work + wk.parents, I.work + wk.expv, I.work + wk.order, I.work + wk.pcnt,
                  I.W, I.H, I.quota, qt_n_roots(I.W, I.H), 0, I.list_cap, I.pool_cap, I.err, s };
    qt_roots(T);
    qt_presort(T);
    qt_whole_list_passes(T);
    qt_refine(T);
    __syncthreads();
    qt_emit(T, I.out_idx, I.out_n, I.out_cap);
}

// concatenate the kept candidates of the levels of one frame into kp_in records (ORBextractor.cpp:840-847,1082-1111)
__global__ __launch_bounds__(256) void quadtree_collect_kernel(const qt_frame* __restrict__ tab)
{
    const qt_frame Fm = tab[blockIdx.x];
    int off = 0;
    for (int l = 0; l < Fm.nlevels; ++l) {
        const int cnt = Fm.out_n[l];
        const int* idx = Fm.out_idx + (size_t)l * Fm.out_cap;
        for (int i = threadIdx.x; i < cnt; i += 256) {
            if (off + i >= Fm.kcap) break;
            const int c = idx[i];
            qt_kp_in q;
            q.x = Fm.xs[c] + (float)Fm.min_border; q.y = Fm.ys[c] + (float)Fm.min_border; q.resp = Fm.rs[c]; q.level = l;
            Fm.kin[off + i] = q;
        }
        off += cnt;
    }
    if (threadIdx.x == 0) { if (off > Fm.kcap) { *Fm.err = QT_E_KCAP; off = Fm.kcap; } *Fm.nk = off; }
}

void dsss_launch_quadtree(hipStream_t st, const qt_inst* d_inst, int ninst)
{
    if (ninst > 0) hipLaunchKernelGGL(quadtree_kernel, dim3(ninst), dim3(QT_THREADS), 0, st, d_inst);
}
void dsss_launch_quadtree_collect(hipStream_t st, const qt_frame* d_frames, int nframes)
{
    if (nframes > 0) hipLaunchKernelGGL(quadtree_collect_kernel, dim3(nframes), dim3(256), 0, st, d_frames);
}

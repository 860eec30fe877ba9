// diasss_amd/csrc/dsss_quadtree.h -- the rules of the quadtree cull that the device kernel (dsss_quadtree.hip), its host twin (quadtree.cpp)
// and the layout of the extraction's scratch (dsss_extract.hip) share, and the launch descriptors of the device quadtree
#pragma once
#include <hip/hip_runtime.h>

struct qt_kp_in { float x, y, resp; int level; };

// what the extraction kernels leave in a frame's error flag: 1..5 the quadtree of one of its levels, 7 the candidate compaction
enum qt_err {
    QT_E_POOL = 1,               // the node pool of a level is full
    QT_E_LIST = 2,               // the node list of a level is full
    QT_E_OUT = 3,                // a level keeps more candidates than out_idx holds
    QT_E_KCAP = 4,               // the levels of a frame keep more keypoints than its store holds
    QT_E_INDEX = 5,              // a level has 2^24 candidates or more (the key keeps 24 bits of the index)
    QT_E_CAND = 7                // more FAST candidates than the candidate arrays hold
};

// ---- the rules of ORBextractor::DistributeOctTree / ExtractorNode::DivideNode (ORBextractor.cpp:481-763), each said once
struct qt_box { int x0, y0, x1, y1; };           // [x0, x1) x [y0, y1) in candidate coordinates

// initial nodes on a level whose FAST range is W x H (:543-546): round(W / H) in float, at least one (the reference divides by zero
// for tall levels); the width of one (:544), the root a candidate falls into (:566-569) and the box of root r (:550-560)
__host__ __device__ inline int qt_n_roots(int W, int H) { const int n = (int)roundf((float)W / (float)H); return n < 1 ? 1 : n; }
__host__ __device__ inline float qt_root_width(int W, int nroots) { return (float)W / nroots; }
__host__ __device__ inline int qt_root_of(float x, float hX, int nroots) { const int r = (int)(x / hX); return r >= nroots ? nroots - 1 : r; }
__host__ __device__ inline qt_box qt_root_box(int r, float hX, int H) { const qt_box b = { (int)(hX * (float)r), 0, (int)(hX * (float)(r + 1)), H }; return b; }

// DivideNode (:481-537): where a box side [lo, hi) is cut, the child a point goes to against the cut (mx, my) in n1..n4 order
// (0 top-left, 1 top-right, 2 bottom-left, 3 bottom-right), and the box of child c
__host__ __device__ inline int qt_mid(int lo, int hi) { return lo + (int)ceilf((float)(hi - lo) / 2); }
__host__ __device__ inline int qt_quadrant(float x, float y, float mx, float my) { const bool left = x < mx, top = y < my; return left ? (top ? 0 : 2) : (top ? 1 : 3); }
__host__ __device__ inline qt_box qt_child_box(const qt_box& b, int c)
{
    const int mx = qt_mid(b.x0, b.x1), my = qt_mid(b.y0, b.y1);
    const qt_box q = { (c & 1) ? mx : b.x0, (c & 2) ? my : b.y0, (c & 1) ? b.x1 : mx, (c & 2) ? b.y1 : my };
    return q;
}

// ---- the work area of one instance, in ints: pool (qnode x pool_cap) | listA listB parents expv order (list_cap each) | pcnt (4 x list_cap).
// make_layout sizes it by `ints`, quadtree_kernel adds the offsets to qt_inst::work
struct qnode { qt_box box; int kbeg, kcnt; int buf; int leaf; };   // 32 B
struct qt_work { size_t pool, listA, listB, parents, expv, order, pcnt, ints; };
__host__ __device__ inline qt_work qt_work_layout(int pool_cap, int list_cap)
{
    qt_work w; size_t o = 0;
    w.pool = o; o += sizeof(qnode) / sizeof(int) * (size_t)pool_cap;
    w.listA = o; o += list_cap; w.listB = o; o += list_cap; w.parents = o; o += list_cap; w.expv = o; o += list_cap; w.order = o; o += list_cap;
    w.pcnt = o; o += (size_t)4 * list_cap;
    w.ints = o;
    return w;
}

struct qt_inst {                 // one (frame, level)
    const int* offs;             // candidate offsets per FAST cell of the frame (scan_counts_kernel output)
    int cell_begin, cell_end;    // cells of this level
    const float *xs, *ys, *rs;   // candidates of the frame, reference order
    int W, H, quota;             // maxBorderX - minBorderX, maxBorderY - minBorderY, mnFeaturesPerLevel[level]
    unsigned long long *keys0, *keys1;   // frame-wide ping-pong key arrays (candidate capacity each); key = y << 48 | x << 32 | response << 24 | candidate index
    int* work;                   // qt_work_layout(pool_cap, list_cap).ints ints
    int list_cap, pool_cap;      // both hold the level's roots and their children on top of what the quota needs
    int* out_idx; int* out_n; int out_cap;
    int* err;
    int cand_cap;                // capacity of xs / ys / rs / keys0 / keys1 (candidates of the whole frame)
};

struct qt_frame {                // one frame: gathers its levels into kp_in records
    int nlevels, out_cap, kcap, min_border;
    const int* out_idx; const int* out_n;
    const float *xs, *ys, *rs;
    qt_kp_in* kin; int* nk; int* err;
};

void dsss_launch_quadtree(hipStream_t st, const qt_inst* d_inst, int ninst);                      // one workgroup per instance
void dsss_launch_quadtree_collect(hipStream_t st, const qt_frame* d_frames, int nframes);         // after every level of the frames has run

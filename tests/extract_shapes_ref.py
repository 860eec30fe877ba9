"""Frames, shape tables and oracle references that hold the extraction kernels (dsss_extract.hip, dsss_quadtree.hip) to the oracle at the
shapes the survey-sized tests never reach: small levels (one to three FAST cells an axis, windows of 30 to 59 px, both LDS strides of
fast_cells_kernel), wide frames (two to 53 quadtree roots), level quotas of one and zero and a quota whose size-ordered refinement starts
with more nodes than quadtree_kernel stages in LDS, keypoints in the border band (the byte-wise reflect-101 patch loading of
orient_desc_kernel), cells that are empty at iniThFAST and not at minThFAST, hot pixels at the image borders, mask parameters other than
the defaults.  Shared by tests/test_extract_shapes_cpu.py (oracle only: every frame is in the class it is named for, so that no GPU
comparison is vacuous) and tests/test_gpu_extract_shapes.py.  Plain functions, no fixtures; references are computed once per session.
"""
import ctypes as C

import numpy as np

from tests import helpers as H

EDGE = 19                      # EDGE_THRESHOLD of the extractor; FAST runs on [EDGE - 3, dim - EDGE + 3)
BORDER = EDGE - 3
PR = 24                        # patch radius of orient_desc_kernel: 18 (rotated BRIEF reach) + 6 (blur)

# ---------------------------------------------------------------- parameters
SMALL_MASK = dict(factor=2.5, width=3, r=2, side=4)          # small frames keep keypoints, border keypoints survive the filter
MASK_INEXACT = dict(factor=2.3, width=3, r=2, side=4)        # (double)(float)2.3 != 2.3
MASK_R0 = dict(factor=2.5, width=3, r=0, side=4)             # the eraser's loops never run
NO_STATIC_MASK = dict(factor=2.5, width=0, r=6, side=0)      # nothing but erasures in the mask


def mask_params(orc, **kw):
    p = orc.mask_params()
    for k, v in kw.items(): setattr(p, k, v)
    return p


def orb_params(orc, **kw):
    p = orc.orb_params()
    for k, v in kw.items(): setattr(p, k, v)
    return p


def device_params(ctx, mask, orb):
    """the library's parameter structs with the fields of the two dicts"""
    mp, op, _, _ = ctx.default_params()
    for k, v in mask.items(): setattr(mp, k, v)
    for k, v in orb.items(): setattr(op, k, v)
    return mp, op


# ---------------------------------------------------------------- geometry: what orc_fast_level / build_geom and DistributeOctTree derive from a size
def fast_cells(rows, cols):
    """cell windows of one level (ORBextractor.cpp:769-806 as oracle/orc_orb.c:orc_fast_level and build_geom restate them):
    dict(ncols, nrows, windows=[(x0, y0, w, h, offx, offy), ...] in launch order)"""
    f = np.float32
    min_b, max_bx, max_by = BORDER, cols - EDGE + 3, rows - EDGE + 3
    width, height = f(max_bx - min_b), f(max_by - min_b)
    ncols, nrows = int(width / f(30)), int(height / f(30))
    out = dict(ncols=ncols, nrows=nrows, windows=[])
    if ncols <= 0 or nrows <= 0:
        return out
    wcell, hcell = int(np.ceil(width / f(ncols))), int(np.ceil(height / f(nrows)))
    for i in range(nrows):
        ini_y = min_b + i * hcell
        if ini_y >= max_by - 3: continue
        max_y = min(ini_y + hcell + 6, max_by)
        for j in range(ncols):
            ini_x = min_b + j * wcell
            if ini_x >= max_bx - 6: continue
            max_x = min(ini_x + wcell + 6, max_bx)
            out["windows"].append((ini_x, ini_y, max_x - ini_x, max_y - ini_y, j * wcell, i * hcell))
    return out


def n_roots(rows, cols):
    """initial nodes of DistributeOctTree on a level (ORBextractor.cpp:543-546; at least one)"""
    r = np.float32(cols - 2 * BORDER) / np.float32(rows - 2 * BORDER)
    return max(1, int(np.floor(r + np.float32(0.5))))           # roundf: halves away from zero, the ratio is positive


def level_sizes(orc, rows, cols, op):
    lr = (C.c_int * 8)(); lc = (C.c_int * 8)()
    orc.lib().orc_orb_level_sizes(rows, cols, C.byref(op), lr, lc)
    return [(lr[l], lc[l]) for l in range(op.nlevels)]


def shape_class(orc, rows, cols, nlevels=1, scale=1.2):
    """what the launches of a frame are sized by: the widest and tallest window over its levels, the LDS stride that selects
    (fast_cells_kernel<40> up to 40 px, <68> above), cells per axis and roots per level"""
    op = orb_params(orc, nlevels=nlevels, scale=scale)
    lv = level_sizes(orc, rows, cols, op)
    cells = [fast_cells(r, c) for r, c in lv]
    max_cw = max(w[2] for g in cells for w in g["windows"]); max_ch = max(w[3] for g in cells for w in g["windows"])
    return dict(levels=lv, max_cw=max_cw, max_ch=max_ch, stride=40 if max_cw <= 40 else 68, ncols=[g["ncols"] for g in cells],
                nrows=[g["nrows"] for g in cells], roots=[n_roots(r, c) for r, c in lv])


def level_quotas(nfeatures, nlevels, scale=1.2):
    """mnFeaturesPerLevel (ORBextractor.cpp:431-444) as build_geom restates it, in float"""
    f = np.float32
    factor = f(1.0) / f(scale)
    desired = f(nfeatures) * (f(1) - factor) / (f(1) - f(float(factor) ** nlevels))
    out = []
    for _ in range(nlevels - 1):
        out.append(int(np.rint(desired))); desired = desired * factor
    return out + [max(nfeatures - sum(out), 0)]


def whole_list_passes(xs, ys, W, H, depth):
    """[(S_p, X_p) for p = 1 .. depth]: non-empty cells and cells of two or more candidates at depth p of DivideNode's boxes under ONE
    root (0, 0, W, H).  While every pass of DistributeOctTree divides the whole list these are its nodes and its expandable nodes after
    pass p: a node of one candidate is never divided and stays one cell at every depth below"""
    x, y = xs.astype(np.int64), ys.astype(np.int64)
    assert (x == xs).all() and (y == ys).all()
    x0 = np.zeros_like(x); y0 = np.zeros_like(x); x1 = np.full_like(x, W); y1 = np.full_like(x, H); code = np.zeros_like(x)
    out = []
    for _ in range(depth):
        mx, my = x0 + (x1 - x0 + 1) // 2, y0 + (y1 - y0 + 1) // 2          # lo + ceil((hi - lo) / 2)
        left, top = x < mx, y < my
        code = code * 4 + np.where(left, np.where(top, 0, 2), np.where(top, 1, 3))
        x1 = np.where(left, mx, x1); x0 = np.where(left, x0, mx); y1 = np.where(top, my, y1); y0 = np.where(top, y0, my)
        sizes = np.unique(code, return_counts=True)[1]
        out.append((len(sizes), int((sizes > 1).sum())))
    return out


def first_verdict(passes, quota):
    """(p, S_p, X_p, refinement) at the first pass after which DistributeOctTree stops dividing the whole list: at its quota (False) or
    within 3 X_p of it (True: the size-ordered refinement starts with X_p expandable nodes); None when neither comes within `passes`"""
    for p, (S, X) in enumerate(passes, 1):
        if S >= quota: return p, S, X, False
        if S + 3 * X > quota: return p, S, X, True
    return None


def resize_strips(sw, dw):
    """whether a level of dw columns made from one of sw takes resize_strip_kernel (True) or the flat resize_kernel: the x table of
    cv::resize(INTER_LINEAR) as dsss_extract.hip:resize_tables builds it (scale in double, fx in float), and the strips' condition that
    the source columns of four consecutive output columns span at most five"""
    fx = ((np.arange(dw) + 0.5) * (1.0 / (float(dw) / sw)) - 0.5).astype(np.float32)
    sx = np.clip(np.floor(fx).astype(int), 0, sw - 1)
    return bool(dw >= 8 and (sx[3:] + 1 - sx[:-3]).max() <= 5)


def patch_inside(x, y, rows, cols):
    """orient_desc_kernel loads the 49 x 49 patch of a keypoint at level coordinates (x, y) as dwords when this holds (the last dword of a
    patch row reaches three bytes past the patch), and byte by byte through reflect-101 indices otherwise"""
    return (x - PR >= 0) & (x + PR + 3 < cols) & (y - PR >= 0) & (y + PR < rows)


def level_coords(kps, op):
    """integer level coordinates of final keypoints (x = x_level * scaleFactor[octave] in float; the product rounds back to the integer)"""
    sf = np.ones(op.nlevels, np.float32)
    for l in range(1, op.nlevels): sf[l] = sf[l - 1] * np.float32(op.scale)
    s = sf[kps["octave"]]
    return np.rint(kps["x"] / s).astype(int), np.rint(kps["y"] / s).astype(int)


def band_sides(orc, kps, rows, cols, op):
    """per keypoint: bit 0 left, 1 top, 2 right, 3 bottom of the border band of its level (0 = the dword path)"""
    lv = level_sizes(orc, rows, cols, op)
    x, y = level_coords(kps, op)
    lr = np.array([lv[o][0] for o in kps["octave"]], int); lc = np.array([lv[o][1] for o in kps["octave"]], int)
    side = (x - PR < 0) * 1 | (y - PR < 0) * 2 | (x + PR + 3 >= lc) * 4 | (y + PR >= lr) * 8
    assert ((side == 0) == patch_inside(x, y, lr, lc)).all()
    return side


# ---------------------------------------------------------------- shape tables
# (rows, cols, nlevels, scale).  Level 0 of a frame has an even number of columns, so its FAST range is even too and the 59-px window
# across a 91-px level can only be a level above: 100 x 100 at 1.1 has a level 1 of 91 x 91, one cell of 59 x 59.
SMALL_ROWS = (69, 70, 91, 92, 121, 122)
SMALL_COLS = (70, 72, 74, 90, 92, 120, 122, 272)
SMALL_SHAPES = [(r, c, 1, 1.2) for r in SMALL_ROWS for c in SMALL_COLS] + [(100, 100, 2, 1.1)]
SMALL_NFEATURES = 60
# (rows, cols, nlevels, scale, resize_strips of levels 1 ..): pyramids whose levels the flat resize_kernel makes, the smallest whose top
# level is still a FAST cell (69 px): at 2.0 and 1.5 no level fits the strips' windows; at 1.334 one level of the frame does and the other not
PYRAMID_SHAPES = [(278, 282, 3, 2.0, (False, False)), (158, 170, 3, 1.5, (False, False)), (124, 126, 3, 1.334, (False, True)), (124, 132, 3, 1.334, (True, False))]

# (rows, cols, nlevels, nfeatures, roots of level 0)
WIDE_SHAPES = [(69, 86, 1, 50, 1), (69, 88, 1, 50, 2), (69, 124, 1, 50, 2), (69, 126, 1, 50, 3), (69, 1234, 1, 100, 32), (69, 1236, 1, 100, 33),
               (69, 2000, 1, 150, 53), (100, 700, 2, 150, 10)]

# the same row, frames of one root whose QUOTA takes quadtree_kernel where no other frame does (wide_case makes them too).
#   100 x 100, nfeatures 1 on two levels: the quotas are (1, 0) -- the keys are written without a pre-sort, the root is divided once by the
#     whole workgroup and the tree is over its quota at once, keeping up to four nodes a level;
#   900 x 640, nfeatures 25000 on one level: six passes leave 4096 nodes, the seventh more than RANK_STAGED expandable ones and fewer
#     nodes than the quota -- the size-ordered refinement starts with more (size, id) pairs than the kernel stages in LDS
QUOTA_SHAPES = [(100, 100, 2, 1, 1), (900, 640, 1, 25000, 1)]
RANK_STAGED = 4096

RAMP_SHAPES = ((160, 272), (200, 400))
THRESHOLDS = ((12, 7), (20, 20), (7, 12), (40, 3), (254, 1))

BAND_SHAPE = (300, 400)
BAND_ORB = dict(nfeatures=1500, nlevels=8, scale=1.2)

HOT_SHAPE = (120, 160)
HOT_R = 6
HOT_ERASED = [((0, 0), 0), ((5, 80), 0), ((60, 5), 0), ((6, 80), 144), ((60, 6), 144), ((6, 6), 144), ((119, 159), 49), ((117, 80), 108), ((60, 158), 96)]
HOT_WRAP_SHAPE = (70, 74)          # M = 2 (mod 4): the 16-byte groups of mask_init_kernel and the 4-byte groups of normalize_kernel wrap rows


# ---------------------------------------------------------------- frames
def dr_inputs(N, M):
    return H.track(N, M, 0, seed=3)


def speckle(N, M, seed):
    """Rayleigh speckle x 1000: corners everywhere, a hundredth of the pixels above 2.5 x mean"""
    return np.random.default_rng(seed).rayleigh(1.0, (N, M)) * 1000.0


def _smooth(a):
    """3 x 3 binomial, edges replicated"""
    p = np.pad(a, 1, mode="edge")
    h = p[:, :-2] + 2.0 * p[:, 1:-1] + p[:, 2:]
    return (h[:-2] + 2.0 * h[1:-1] + h[2:]) / 16.0


def gain_ramp(N, M, seed):
    """lightly smoothed uniform texture whose contrast rises linearly across the columns from 0 to about 0.25 of the mean: cells with
    corners above iniThFAST on the right, cells empty at every threshold on the left, and cells in between that only minThFAST fills"""
    t = _smooth(np.random.default_rng(seed).uniform(-1.0, 1.0, (N, M)))
    t /= np.abs(t).max()
    return 1000.0 * (1.0 + 0.25 * np.linspace(0.0, 1.0, M)[None, :] * t)


def flat_with_hot(N, M, seed, hot, knife=None, factor=2.3, orc=None):
    """texture of +-5 % about 1000 with pixels of 4 x mean at the positions `hot`.  knife = (i, j): one more pixel whose value lies between
    mean * (double)(float)factor and mean * factor -- above the threshold the reference's float factor gives, below the one a double would"""
    raw = 1000.0 * np.random.default_rng(seed).uniform(0.95, 1.05, (N, M))
    for i, j in hot: raw[i, j] = 4000.0
    if knife is not None:
        ff, fd = float(np.float32(factor)), float(factor)
        assert ff < fd
        for _ in range(4):
            m = orc.lib().orc_mean(orc.dp(raw), N, M)
            raw[knife] = m * 0.5 * (ff + fd)
        m = orc.lib().orc_mean(orc.dp(raw), N, M)
        assert m * ff < raw[knife] < m * fd
    return raw


# ---------------------------------------------------------------- oracle references, stage by stage
_REFS = {}


def oracle_stages(orc, raw, mask, orb, sift=False, key=None):
    """the oracle on one frame with the parameter dicts `mask` and `orb`: dict(norm, mask, levels, cands=[(x, y, resp) per level], kps, desc
    [, d128], op, mp).  key: computed once per session under that name; the arrays are read-only"""
    if key is not None and key in _REFS:
        return _REFS[key]
    mp, op = mask_params(orc, **mask), orb_params(orc, **orb)
    N, M = raw.shape
    out = dict(op=op, mp=mp, norm=orc.normalize(raw), mask=orc.mask(raw, mp))
    lv = level_sizes(orc, N, M, op)
    levels = [out["norm"]]
    for l in range(1, op.nlevels):
        dst = np.zeros(lv[l], np.uint8); prev = levels[-1]
        orc.lib().orc_resize_linear_u8(orc.u8(prev), prev.shape[0], prev.shape[1], orc.u8(dst), lv[l][0], lv[l][1])
        levels.append(dst)
    out["levels"] = levels
    cands = []
    for l in range(op.nlevels):
        cap = (lv[l][0] // 2 + 1) * (lv[l][1] // 2 + 1)          # no two 8-neighbours are both strict maxima
        xs = np.zeros(cap, np.float32); ys = np.zeros(cap, np.float32); rs = np.zeros(cap, np.float32)
        k = orc.lib().orc_fast_level(orc.u8(levels[l]), lv[l][0], lv[l][1], op.ini_th, op.min_th, orc.fp(xs), orc.fp(ys), orc.fp(rs), cap)
        assert k < cap
        cands.append((xs[:k].copy(), ys[:k].copy(), rs[:k].copy()))
    out["cands"] = cands
    res = orc.detect_feature(raw, mp, op, sift=sift)
    out["kps"], out["desc"] = res[0], res[1]
    if sift: out["d128"] = res[4]
    for v in list(out.values()) + levels + [a for c in cands for a in c]:
        if isinstance(v, np.ndarray): v.setflags(write=False)
    if key is not None:
        _REFS[key] = out
    return out


def unfiltered_keypoints(orc, ref):
    """the extractor's keypoints before the mask filter"""
    return orc.orb_extract(ref["norm"], ref["op"], cap=ref["op"].nfeatures * 4 + 4096)[0]


def small_case(orc, rows, cols, nlevels, scale):
    raw = speckle(rows, cols, 7 * rows + cols)
    orb = dict(nfeatures=SMALL_NFEATURES, nlevels=nlevels, scale=scale)
    return raw, orb, oracle_stages(orc, raw, SMALL_MASK, orb, key=("small", rows, cols, nlevels, scale))


def wide_case(orc, rows, cols, nlevels, nfeatures):
    raw = speckle(rows, cols, 11 * rows + cols)
    orb = dict(nfeatures=nfeatures, nlevels=nlevels)
    return raw, orb, oracle_stages(orc, raw, SMALL_MASK, orb, key=("wide", rows, cols, nlevels))


def ramp_case(orc, N, M, ini, mn):
    raw = gain_ramp(N, M, N + M)
    orb = dict(nfeatures=300, nlevels=2, ini_th=ini, min_th=mn)
    return raw, orb, oracle_stages(orc, raw, SMALL_MASK, orb, key=("ramp", N, M, ini, mn))


def band_case(orc, nlevels=BAND_ORB["nlevels"], sift=False):
    N, M = BAND_SHAPE
    raw = speckle(N, M, 77)
    orb = dict(BAND_ORB, nlevels=nlevels)
    return raw, orb, oracle_stages(orc, raw, SMALL_MASK, orb, sift=sift, key=("band", nlevels, sift))


def cell_survivors(orc, img, thr):
    """per cell window of a level image: corners that survive non-max suppression at threshold thr"""
    rows, cols = img.shape
    buf = (C.c_int * 1600)()
    out = []
    for x0, y0, w, h, _, _ in fast_cells(rows, cols)["windows"]:
        win = img[y0:, x0:]
        out.append(orc.lib().orc_fast_window(C.c_void_p(win.ctypes.data), cols, h, w, thr, buf, buf, buf, 1600))
    return np.array(out)

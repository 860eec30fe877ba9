"""Frames, window classes and oracle references that hold sift_desc_kernel (dsss_sift.hip) to the oracle (oracle/orc_sift.c) where the
survey-sized tests of tests/test_gpu_sift.py never go: levels of 69 to 122 px, on which the 71 x 71 raw window of a keypoint leaves the
image on one, two, three or four sides; the two ways of loading that window on either side of each of their eight equalities (also at an IC
angle on a diagonal, the only angles at which the window's outermost ring reaches a sample: the diag frames); the reset of
ori = 360 - angle at angle == 0; the wrap of the orientation bin below 0; the clip at 0.2 of the norm; batches of frames of different
shapes.  Shared by tests/test_sift_shapes_cpu.py (oracle only: every class named here is present, or asserted absent) and
tests/test_gpu_sift_shapes.py.  Plain functions; every reference is computed once per session.

THE WINDOW CLASS of a keypoint at integer level coordinates (cx, cy) on a level of rows x cols, stated here once and held to nothing in the
library: with R = 35 (28 sample radius + 1 gradient neighbour + 6 blur taps) the bits are left cx - R < 0, top cy - R < 0, right
cx + R >= cols, bottom cy + R >= rows.  Class 0 loads the window as unaligned dwords, every other class byte by byte through reflect-101.

CLASSES THAT THE EXTRACTION CANNOT REACH (tests/test_sift_shapes_cpu.py asserts their absence on every frame of the table):

  o0 >= 8.  obin = (Ori - ori) * (8 / 360.f) with Ori = fastAtan2(dy, dx) of integer dx, dy in -255 .. 255 and ori = 360 - angle in
  [0, 360) (360 itself is reset to 0; the IC angle is a fastAtan2 too, so never negative and never above 360).  The largest Ori below 360
  belongs to dy = -1, dx = 255: 360 - 0.2246 = 359.7754, so obin <= 359.7754 * 0.0222222 = 7.995 and floor(obin) <= 7 whatever ori is.
  The branch would need a keypoint angle above 360.  Given such an angle directly (orc.sift_hist(.., 361.0)) the oracle takes it, and the
  restatement below shows what it is worth there: with o0 = 8 the two shares land in slots 8 and 9 of the cell's ten, which the circular
  fold adds to slots 0 and 1 -- the histogram is the same with and without the wrap.  No test can fail on its removal; the wrap below 0
  is the live one (without it the shares land in the slots of the cell before).

  rr > 255 (the saturation of the tail).  An element is at most thr = 0.2 |h| after the clip, and rr = 512 v / |min(h, thr)|: with m
  elements at the clip and nothing else rr = 512 / sqrt(m), so rr > 255.5 needs at most three elements at the clip and the remaining
  125 together below 0.016 thr.  A FAST corner in the middle of a 57 x 57 Gaussian window spreads every edge over several of the 4 x 4
  cells (trilinear shares in two cell rows and two cell columns at least).  Designs tried (SATURATION_DESIGNS, largest rr reached in
  brackets as tests/test_sift_shapes_cpu.py prints it; speckle reaches 122): isolated bright rectangles of 5 x 5 to 9 x 21 px on an
  exactly flat field, whose corner keypoints see gradients along two lines only [142]; single bright pixels and 2 x 2 dots, a blob after
  the blur [136]; one-pixel line segments of 3 to 9 px [152]; rectangles near the corners of a 69 x 70 frame, where the image clips
  the window on two sides [150].
"""
import ctypes as C

import numpy as np

from tests import extract_shapes_ref as X

R = 35
LEFT, TOP, RIGHT, BOTTOM = 1, 2, 4, 8
CLASS_NAME = {0: "inside (dword path)"}
for _c in range(1, 16):
    CLASS_NAME[_c] = "+".join(n for b, n in ((LEFT, "left"), (TOP, "top"), (RIGHT, "right"), (BOTTOM, "bottom")) if _c & b) + " (reflect-101 path)"
SINGLE = (LEFT, TOP, RIGHT, BOTTOM)
CORNERS = (LEFT | TOP, RIGHT | TOP, LEFT | BOTTOM, RIGHT | BOTTOM)


def window_class(cx, cy, rows, cols):
    return (cx - R < 0) * LEFT | (cy - R < 0) * TOP | (cx + R >= cols) * RIGHT | (cy + R >= rows) * BOTTOM


# the eight equalities of the dword condition (met from inside) and their neighbours (the first keypoint outside)
EQUALITIES = {"cx == 35": lambda x, y, r, c: x == R, "cx == 34": lambda x, y, r, c: x == R - 1,
              "cx == cols - 36": lambda x, y, r, c: x == c - R - 1, "cx == cols - 35": lambda x, y, r, c: x == c - R,
              "cy == 35": lambda x, y, r, c: y == R, "cy == 34": lambda x, y, r, c: y == R - 1,
              "cy == rows - 36": lambda x, y, r, c: y == r - R - 1, "cy == rows - 35": lambda x, y, r, c: y == r - R}

# ---------------------------------------------------------------- frames
SIFT_ROWS = (69, 70, 91, 122)
SIFT_COLS = (70, 74, 92, 272)
BAND_NFEATURES = 600           # (the band frame of extract_shapes_ref asks for 1500: every keypoint's histogram is compared, in Python)
# 76 x 76 at 1.1: level 1 is 69 x 69, where a keypoint at (34, 34) -- the one position there is -- has all four sides clipped.  The seed is the
# first of 400 tried whose speckle has it next to other keypoints with cx == 34 and with cy == 34; the static mask of width 3 hides the
# centre columns of a frame (x_level = 34 is bin 37 of 76), so this frame alone has width = 0 and the keypoint survives the filter
ALLFOUR = (76, 76, 2, 1.1, 5234)
ALLFOUR_MASK = dict(X.SMALL_MASK, width=0)
LEFTRIGHT = (100, 76, 2, 1.1, 6000)      # level 1 is 91 x 69: cx == 34 with cy from 35 to 55 is clipped left and right and on no other side
MIRROR_SHAPE = (121, 122)      # an odd number of rows: the axis of the mirror image is row 60
MIRROR_SEEDS = (1, 2, 3)
# one set of parameters per batch: a level 1 of a 69-row frame still has 69 rows below a scale of 1.0073 only (at 1.1 it would be refused as too
# small), and the 33 + 32 quadtree roots of the two levels of 69 x 1236 can keep 260 keypoints, which the store holds from nfeatures = 187 on
BATCH_ORB = dict(nfeatures=200, nlevels=2, scale=1.004)
BATCH_SHAPES = ((69, 70), (69, 1236), (100, 100), (72, 76))  # the last one is flat
SATURATION_DESIGNS = ("rects", "dots", "segments", "corner-rects")


def mirror(N, M, seed):
    """speckle that is its own mirror image about row (N - 1) / 2: the patch moments of a keypoint on that row have m01 == 0 exactly"""
    raw = X.speckle(N, M, 900 + seed)
    raw[N // 2 + 1:] = raw[:N // 2][::-1]
    return raw


# the outermost ring of the 71 x 71 window feeds only the samples at (+-28, ~0) of a window turned by 45 degrees (a sample is live within 20 px
# of the centre along both turned axes: 28 cos 45 = 19.8), so a dword condition that is off by ONE moves a histogram only at keypoints whose IC
# angle is within 0.6 degrees of a diagonal.  A patch that is its own transpose has m01 == m10, an angle of 45 or 225: four such patches around a
# bright pixel one step outside each side of the condition ("out"), and four at the equalities themselves ("in"), on 122 x 122
DIAG_SHAPE = (122, 122)
DIAG_AT = {"out": ((34, 40), (87, 80), (80, 34), (40, 87)), "in": ((35, 40), (86, 80), (80, 35), (40, 86))}      # (cx, cy): left, right, top, bottom
# of 400 seeds tried none moves all four (the ring's weight in the blur is 1 / 256: most of the time no rounded byte changes); under flat
# addresses seed 25 has another histogram at its left, right and top keypoint, seed 72 at its right, top and bottom one
DIAG_FRAMES = {"diag-out-25": ("out", 25), "diag-out-72": ("out", 72), "diag-in-0": ("in", 0)}


def diagonal(which, seed):
    N, M = DIAG_SHAPE
    raw = X.speckle(N, M, 700 + seed)
    for cx, cy in DIAG_AT[which]:
        P = raw[cy - 15:cy + 16, cx - 15:cx + 16]
        P[:] = np.triu(P) + np.triu(P, 1).T
        P[:] = np.minimum(P, 2000.0)
        P[15, 15] = 3000.0
    return raw


def designed(kind, seed=0):
    """the flat-field designs for the saturating row: value 1000, features at 2000 to 2400 (under the mask's 2.5 x mean).  A plain rectangle
    gives no keypoint at all (the FAST scores tie along its edges and nothing is a strict maximum): two of its corner pixels are brighter"""
    rng = np.random.default_rng(40 + seed)
    if kind == "corner-rects":
        raw = np.full((69, 70), 1000.0)                   # (a frame has an even number of bins)
        raw[20:29, 20:31] = 2000.0; raw[42:49, 38:47] = 2000.0
        raw[20, 20] = raw[28, 30] = raw[42, 38] = raw[48, 46] = 2300.0
        return raw
    raw = np.full((160, 200), 1000.0)
    for k in range(12):
        y, x = 25 + 40 * (k // 4) + int(rng.integers(0, 6)), 25 + 45 * (k % 4) + int(rng.integers(0, 6))
        if kind == "rects":
            h, w = ((5, 5), (7, 9), (9, 21), (6, 13))[k % 4]
            raw[y:y + h, x:x + w] = 2000.0
            raw[y, x] = raw[y + h - 1, x + w - 1] = 2300.0
        elif kind == "dots":
            s = 1 + k % 2
            raw[y:y + s, x:x + s] = 2400.0
        else:
            n = 3 + 2 * (k % 4)
            if k % 2: raw[y, x:x + n] = 2400.0
            else: raw[y:y + n, x] = 2400.0
    return raw


def _table():
    t = {}
    for r in SIFT_ROWS:
        for c in SIFT_COLS:
            t["small-%dx%d" % (r, c)] = ("small", (r, c, 1, 1.2))
    t["small-100x100@1.1"] = ("small", (100, 100, 2, 1.1))
    for s in X.PYRAMID_SHAPES:
        t["pyramid-%dx%d@%g" % (s[0], s[1], s[3])] = ("small", s[:4])
    for s in X.WIDE_SHAPES:
        if s[:2] in ((69, 126), (69, 1236)):
            t["wide-%dx%d" % s[:2]] = ("wide", s[:4])
    t["band-8"] = ("band", 8); t["band-2"] = ("band", 2)
    t["allfour-76x76@1.1"] = ("allfour", ALLFOUR); t["allfour-100x76@1.1"] = ("allfour", LEFTRIGHT)
    for s in MIRROR_SEEDS:
        t["mirror-%d" % s] = ("mirror", s)
    for n, a in DIAG_FRAMES.items(): t[n] = ("diag", a)
    for k in SATURATION_DESIGNS:
        t["design-" + k] = ("design", k)
    return t


TABLE = _table()
NAMES = tuple(TABLE)
PART1 = tuple(n for n in NAMES if n.split("-")[0] in ("small", "pyramid", "wide", "band", "allfour"))
BATCH = tuple("batch-%dx%d" % s for s in BATCH_SHAPES)


def inputs(name):
    """(raw, mask dict, orb dict) of a frame of the table or of the batch"""
    if name in BATCH:
        N, M = BATCH_SHAPES[BATCH.index(name)]
        raw = np.full((N, M), 7.0) if name == BATCH[3] else X.speckle(N, M, (7 if M < 1000 else 11) * N + M)
        return raw, X.SMALL_MASK, dict(BATCH_ORB)
    kind, a = TABLE[name]
    if kind == "small":
        return X.speckle(a[0], a[1], 7 * a[0] + a[1]), X.SMALL_MASK, dict(nfeatures=X.SMALL_NFEATURES, nlevels=a[2], scale=a[3])
    if kind == "wide":
        return X.speckle(a[0], a[1], 11 * a[0] + a[1]), X.SMALL_MASK, dict(nfeatures=a[3], nlevels=a[2])
    if kind == "band":
        return X.speckle(X.BAND_SHAPE[0], X.BAND_SHAPE[1], 77), X.SMALL_MASK, dict(X.BAND_ORB, nlevels=a, nfeatures=BAND_NFEATURES)
    if kind == "allfour":
        return X.speckle(a[0], a[1], a[4]), ALLFOUR_MASK, dict(nfeatures=X.SMALL_NFEATURES, nlevels=a[2], scale=a[3])
    if kind == "diag":
        return diagonal(*a), X.SMALL_MASK, dict(nfeatures=X.SMALL_NFEATURES, nlevels=1)
    if kind == "mirror":
        return mirror(MIRROR_SHAPE[0], MIRROR_SHAPE[1], a), X.SMALL_MASK, dict(nfeatures=X.SMALL_NFEATURES, nlevels=1)
    return designed(a), X.SMALL_MASK, dict(nfeatures=X.SMALL_NFEATURES, nlevels=1)


# ---------------------------------------------------------------- oracle references
_CASES = {}


def case(orc, name):
    """the oracle on one frame in SIFT mode, once per session: dict(raw, mask, orb, ref = extract_shapes_ref.oracle_stages(sift=True),
    pre = the PRE-FILTER keypoints in the order of the device's list, pre_d128, x, y, rows, cols = integer level coordinates and level size
    per pre-filter keypoint, cls = window class (surv_cls: of the keypoints behind the mask filter), blur = the blurred levels, hist = int32[n][128] of orc.sift_hist)"""
    if name in _CASES:
        return _CASES[name]
    raw, mask, orb = inputs(name)
    ref = X.oracle_stages(orc, raw, mask, orb, sift=True, key=("sift-shapes", name))
    op = ref["op"]
    pre, _, pre_d128 = orc.orb_extract_sift(ref["norm"], op, cap=op.nfeatures * 4 + 4096)
    lv = X.level_sizes(orc, raw.shape[0], raw.shape[1], op)
    x, y = X.level_coords(pre, op)
    rows = np.array([lv[o][0] for o in pre["octave"]], int); cols = np.array([lv[o][1] for o in pre["octave"]], int)
    sx, sy = X.level_coords(ref["kps"], op)
    so = ref["kps"]["octave"]
    surv_cls = window_class(sx, sy, np.array([lv[o][0] for o in so], int), np.array([lv[o][1] for o in so], int)) if len(so) else np.zeros(0, int)
    blur = [orc.blur13(im) for im in ref["levels"]]
    hist = np.zeros((len(pre), 128), np.int32)
    for i in range(len(pre)):
        hist[i] = orc.sift_hist(blur[pre["octave"][i]], x[i], y[i], float(pre["angle"][i]))
    out = dict(name=name, raw=raw, mask=mask, orb=orb, ref=ref, pre=pre, pre_d128=pre_d128, x=x, y=y, rows=rows, cols=cols,
               cls=window_class(x, y, rows, cols) if len(pre) else np.zeros(0, int), surv_cls=surv_cls, blur=blur, hist=hist)
    for v in out.values():
        if isinstance(v, np.ndarray): v.setflags(write=False)
    _CASES[name] = out
    return out


# ---------------------------------------------------------------- orc_sift_hist and orc_sift_finalize restated in numpy float32 / float64
def _fast_atan2(y, x):
    f = np.float32
    scale = f(180.0 / 3.1415926535897932384626433832795)
    p1, p3, p5, p7 = f(0.9997878412794807) * scale, f(-0.3258083974640975) * scale, f(0.1555786518463281) * scale, f(-0.04432655554792128) * scale
    eps = f(2.2204460492503131e-16)
    ax, ay = np.abs(x), np.abs(y)
    big = ax >= ay
    c = np.where(big, ay / (ax + eps), ax / (ay + eps)).astype(f)
    c2 = c * c
    a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
    a = np.where(big, a, f(90.0) - a).astype(f)
    a = np.where(x < 0, f(180.0) - a, a).astype(f)
    return np.where(y < 0, f(360.0) - a, a).astype(f)


def hist_restated(orc, blurred, x, y, angle, wrap_low=True, wrap_high=True):
    """orc_sift_hist operation for operation on arrays of float32 (numpy fuses nothing): dict(h = int32[128], o0 = floor(obin) of every live
    sample BEFORE the wrap, ori).  wrap_low / wrap_high = False drop `if (o0 < 0) o0 += 8` / `if (o0 >= 8) o0 -= 8`"""
    f = np.float32
    rows, cols = blurred.shape
    w = orc.sift_weights(2 * 28 * 28 + 1)
    ori = f(360.0) - f(angle)
    if abs(ori - f(360.0)) < f(1.1920928955078125e-7): ori = f(0.0)
    factor_pi = f(3.1415926535897932384626433832795 / 180.0)
    sd, cd = C.c_double(), C.c_double()
    orc.lib().orc_sincos(float(ori * factor_pi), C.byref(sd), C.byref(cd))
    cos_t, sin_t = f(cd.value) / f(8.0), f(sd.value) / f(8.0)
    bins_per_deg = f(8.0) / f(360.0)
    i, j = np.meshgrid(np.arange(-28, 29), np.arange(-28, 29), indexing="ij")
    fi, fj = i.astype(f), j.astype(f)
    c_rot = fj * cos_t - fi * sin_t
    r_rot = fj * sin_t + fi * cos_t
    rbin, cbin = r_rot + f(1.5), c_rot + f(1.5)
    r, c = y + i, x + j
    live = (rbin > -1) & (rbin < 4) & (cbin > -1) & (cbin < 4) & (r > 0) & (r < rows - 1) & (c > 0) & (c < cols - 1)
    i, j, r, c, rbin, cbin = i[live], j[live], r[live], c[live], rbin[live], cbin[live]
    b = blurred.astype(np.int32)
    dx = (b[r, c + 1] - b[r, c - 1]).astype(f); dy = (b[r - 1, c] - b[r + 1, c]).astype(f)
    Ori = _fast_atan2(dy, dx)
    Mag = np.sqrt(dx * dx + dy * dy)
    obin = (Ori - ori) * bins_per_deg
    mag = Mag * w[i * i + j * j]
    r0, c0, o0 = np.floor(rbin).astype(int), np.floor(cbin).astype(int), np.floor(obin).astype(int)
    rbin = rbin - r0.astype(f); cbin = cbin - c0.astype(f); obin = obin - o0.astype(f)
    o0_raw = o0.copy()
    if wrap_low: o0 = np.where(o0 < 0, o0 + 8, o0)
    if wrap_high: o0 = np.where(o0 >= 8, o0 - 8, o0)
    v_r1 = mag * rbin; v_r0 = mag - v_r1
    v_rc11 = v_r1 * cbin; v_rc10 = v_r1 - v_rc11
    v_rc01 = v_r0 * cbin; v_rc00 = v_r0 - v_rc01
    v111 = v_rc11 * obin; v110 = v_rc11 - v111
    v101 = v_rc10 * obin; v100 = v_rc10 - v101
    v011 = v_rc01 * obin; v010 = v_rc01 - v011
    v001 = v_rc00 * obin; v000 = v_rc00 - v001
    idx = ((r0 + 1) * 6 + c0 + 1) * 10 + o0
    hist = np.zeros(360, np.int64)
    for off, v in ((0, v000), (1, v001), (10, v010), (11, v011), (60, v100), (61, v101), (70, v110), (71, v111)):
        assert v.dtype == f
        np.add.at(hist, idx + off, np.rint(v * f(4096.0)).astype(np.int64))
    h3 = hist.reshape(6, 6, 10)
    h3[:, :, 0] += h3[:, :, 8]; h3[:, :, 1] += h3[:, :, 9]
    return dict(h=h3[1:5, 1:5, :8].reshape(128).astype(np.int32), o0=o0_raw, ori=float(ori))


def finalize_restated(h):
    """orc_sift_finalize in float64: dict(out = uint8[128], rr = the rounded element before the clamp to 0 .. 255, clipped = elements that
    the clip at 0.2 of the norm changes)"""
    h = np.asarray(h, np.int64)
    nrm = np.sqrt(float((h * h).sum()))
    thr = int(nrm * 0.2)
    v = np.minimum(h, thr)
    den = max(np.sqrt(float((v * v).sum())), 1.1920928955078125e-7)
    rr = np.rint(v.astype(np.float64) * (512.0 / den)).astype(np.int64)
    return dict(out=np.clip(rr, 0, 255).astype(np.uint8), rr=rr, clipped=h > thr)


# ---------------------------------------------------------------- the two ways of loading the 71 x 71 raw window, restated
def raw_window(level, cx, cy, dwords):
    """the raw window of sift_desc_kernel around (cx, cy): through reflect-101 indices, or (dwords) by flat addresses from the window's
    corner as the unaligned dword loads read it, whatever the class of the keypoint is -- a byte left or right of a row is the
    neighbouring row's, a byte before or behind the level buffer is taken as 0"""
    rows, cols = level.shape
    py, px = np.mgrid[0:2 * R + 1, 0:2 * R + 1]
    if not dwords:
        def refl(p, n):
            p = np.where(p < 0, -p, p)
            return np.where(p >= n, 2 * (n - 1) - p, p)
        return level[refl(cy + py - R, rows), refl(cx + px - R, cols)]
    flat = np.concatenate([np.zeros(R * cols + R, np.uint8), level.ravel(), np.zeros((R + 1) * cols + R, np.uint8)])
    return flat[R * cols + R + (cy - R + py) * cols + (cx - R + px)]


def hist_from_window(orc, c, i, dwords):
    """the histogram of pre-filter keypoint i of a case when its window is loaded the given way: the window blurred where all 13 x 13 taps
    lie inside it (the kernel's 59 x 59), laid over the oracle's blurred level, then orc_sift_hist"""
    l = int(c["pre"]["octave"][i]); cx, cy = int(c["x"][i]), int(c["y"][i])
    level = c["ref"]["levels"][l]
    rows, cols = level.shape
    B = orc.blur13(np.ascontiguousarray(raw_window(level, cx, cy, dwords)))[6:-6, 6:-6]
    img = c["blur"][l].copy()
    y0, x0 = cy - 29, cx - 29
    ys, xs = slice(max(y0, 0), min(y0 + 59, rows)), slice(max(x0, 0), min(x0 + 59, cols))
    img[ys, xs] = B[ys.start - y0:ys.stop - y0, xs.start - x0:xs.stop - x0]
    return orc.sift_hist(img, cx, cy, float(c["pre"]["angle"][i]))

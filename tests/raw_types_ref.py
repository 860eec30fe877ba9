"""Frames, quantisers and the case table of the typed-waterfall tests (u8, u16 and f32 raw images next to f64): what
tests/test_raw_types_cpu.py holds to its preconditions on the oracle and tests/test_gpu_raw_types.py runs on the device.  A typed frame
must give bit for bit what the f64 path gives for the same samples widened to double, so every reference is the oracle on widen(q).
Plain functions, no fixtures; references are computed once per session (extract_shapes_ref.oracle_stages keeps them)."""
import numpy as np

from tests import extract_shapes_ref as X

RAW_F64, RAW_F32, RAW_U16, RAW_U8 = 0, 1, 2, 3
DTYPES = {"f64": np.float64, "f32": np.float32, "u16": np.uint16, "u8": np.uint8}
RAW_TYPE = {"f64": RAW_F64, "f32": RAW_F32, "u16": RAW_U16, "u8": RAW_U8}
ESIZE = {"f64": 8, "f32": 4, "u16": 2, "u8": 1}
NARROW = ("u8", "u16", "f32")
INTEGER = ("u8", "u16")
KINDS = ("speckle", "flat_with_hot")

# (rows, cols, nlevels, nfeatures).  M = 70 and 74 are 2 (mod 4) and 6 / 10 (mod 16): every pixel group of normalize_kernel (4, 8, 16)
# wraps rows and ends in a short tail, and the rows of a u8 image start at every even address (mod 16); 69, 91 and 121 rows leave a
# partly filled workgroup of four rows in the row reduce; M = 272 takes a lane of the f32 form through three iterations of the
# 128-stride; 100 x 700 has two pyramid levels
SHAPES = [(69, 70, 1, 60), (70, 74, 1, 60), (91, 72, 1, 60), (121, 90, 1, 60), (120, 160, 1, 60), (122, 272, 1, 60), (100, 700, 2, 150)]
MASK = X.SMALL_MASK


def hot_pixels(N, M):
    """two pixels of 4 x mean away from the static mask (centre stripe, sides) and further than r from the borders"""
    return [(N // 2, M // 4), (N // 3, (3 * M) // 4)]


def quantise(raw, t):
    """a float64 waterfall of about 1000 x texture as a sonar of type t records it (diasss_amd.synth.quantise): u16 rounds and clamps
    to 65535, u8 rounds a sixteenth and clamps to 255, f32 rounds to nearest"""
    if t == "f64": return np.ascontiguousarray(raw, np.float64)
    if t == "f32": return raw.astype(np.float32)
    if t == "u16": return np.clip(np.rint(raw), 0, 65535).astype(np.uint16)
    if t == "u8": return np.clip(np.rint(raw / 16.0), 0, 255).astype(np.uint8)
    raise KeyError(t)


def widen(q):
    """(double)sample: exact for every type"""
    return np.ascontiguousarray(q, np.float64)


def base_frame(kind, N, M):
    if kind == "speckle": return X.speckle(N, M, 13 * N + M)
    if kind == "flat_with_hot": return X.flat_with_hot(N, M, 5 * N + M, hot_pixels(N, M))
    raise KeyError(kind)


def shadows(raw, seed):
    """an eighth of the samples scaled by 2^-23 (acoustic shadow next to full returns: the range a float sample has and an integer one
    has not).  Widened f32 samples of ONE magnitude add exactly in double -- 24 bits each, sums below 2^23 -- in whatever order; with
    samples 2^23 times smaller among them the partial sums round, and the order of the additions shows in the bits of the mean.
    The brightest samples (the hot pixels) stay as they are."""
    dark = (np.random.default_rng(seed).random(raw.shape) < 0.125) & (raw < 3.0 * raw.mean())
    return np.where(dark, raw * 2.0 ** -23, raw)


def frame(kind, t, N, M):
    """the frame of a case in its own sample type; the f32 frames carry shadows"""
    raw = base_frame(kind, N, M)
    # (a rounded sum can still divide to the same mean, as it does for about one frame in ten: with this seed none of the case frames
    # does, which tests/test_raw_types_cpu.py asserts)
    return quantise(shadows(raw, N + 3 * M + 2) if t == "f32" else raw, t)


def orb(nlevels, nfeatures):
    return dict(nfeatures=nfeatures, nlevels=nlevels)


def case(orc, kind, t, shape):
    """(typed frame, widened frame, orb dict, oracle stages of the widened frame)"""
    N, M, nl, nf = shape
    q = frame(kind, t, N, M); w = widen(q)
    return q, w, orb(nl, nf), X.oracle_stages(orc, w, MASK, orb(nl, nf), key=("raw_types", kind, t, N, M))


def exact_mean(q):
    """the mean of an integer frame as the exact quotient, correctly rounded (Python's int / int)"""
    return int(q.astype(np.int64).sum()) / (q.shape[0] * q.shape[1])


def sequential_mean(w):
    """row-major running sum in double, divided as the extraction divides"""
    s = 0.0
    for v in w.ravel().tolist(): s += v
    return s / (float(w.shape[0]) * float(w.shape[1]))


def bits(*vals):
    return np.array(vals, np.float64).tobytes()


# the mixed batch: eight frames, four types, two geometries
MIXED_ORDER = ("f64", "u8", "u16", "f32", "u8", "f64", "f32", "u16")
MIXED_SHAPES = ((69, 70), (91, 72))


def mixed_frames():
    """[(typed frame, widened frame)] of the mixed batch: frame k has type MIXED_ORDER[k] and geometry MIXED_SHAPES[k % 2], so every type
    meets both geometries"""
    out = []
    for k, t in enumerate(MIXED_ORDER):
        N, M = MIXED_SHAPES[k % 2]
        raw = X.speckle(N, M, 900 + k)
        q = quantise(shadows(raw, k) if t == "f32" else raw, t)
        out.append((q, widen(q)))
    return out

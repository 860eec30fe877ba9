"""The cases of the altitude-banded range gain, shared by tests/test_mosaic_gain_bands_cpu.py (the precondition, on the references
alone) and tests/test_gpu_mosaic_gain_bands.py (the device against the same numbers).

The effect survey: synth.Survey(2, 640, 400, seed=7) with altitudes of the test's own (the mosaic never reads altitudes for geometry),
alt_f[i] = 10 + 3 sin(2 pi s_i / 20 + 0.9 f), s_i = (i + 0.5) 0.05, whose raw frames carry synth.angle_profile(amp 0.5, k 6): a profile
fixed to the grazing angle, which no table per column describes.  Binned under the TRUE poses at cell 0.1 with the mask on; bands
(7.0, 1.0, 6), min_count 64, smooth 8.  Everything expected is the oracle's (normalize, mask, geo_img) and the numpy references';
nothing here calls the library.  Computed once per session.

The shape table: the shapes at which mosaic_gainstat_kernel takes another path and the altitude series that drive its band logic."""
import numpy as np

from tests import mosaic_gain_bands_ref as B
from tests import mosaic_gain_cases as K
from tests import mosaic_gain_ref as G

F, N, M, SEED, CELL = 2, 640, 400, 7, 0.1
AMP, KCOS = 0.5, 6.0
BANDS = (7.0, 1.0, 6)
MIN_COUNT, SMOOTH, TARGET = 64, 8, 0
_CACHE = {}

# rows x columns: M < 256 (32 lanes a row), five column chunks on the byte path (1234) and on the dword path (1236), the byte path
# with rows left over (501 x 402), a partial row block in batches and one by one (333), a full row block and a partial one (640)
SHAPES = [(69, 86), (69, 1234), (69, 1236), (501, 402), (333, 400), (640, 400)]
SERIES = ("one", "cycle", "runs", "edges", "wild")
SHAPE_BANDS = (4.0, 0.75, 16)               # the bands of the shape tests (0.75 and its multiples are exact in f64: the edges are edges)


def effect_alt(f):
    s = (np.arange(N) + 0.5) * 0.05
    return 10.0 + 3.0 * np.sin(2 * np.pi * s / 20.0 + 0.9 * f)


def series(kind, n, bands, seed=0):
    """n altitudes: "one": one band for all pings; "cycle": the band changes on every ping, through all of them; "runs": bands in long
    runs (37 pings, in no monotone order); "edges": altitudes exactly on band edges alt0 + k dalt, k from -1 to nbands + 1; "wild": NaN,
    +-inf and far out-of-range altitudes among ordinary ones"""
    alt0, dalt, nb = bands
    i = np.arange(n)
    if kind == "one":
        return np.full(n, alt0 + (min(2, nb - 1) + 0.5) * dalt)
    if kind == "cycle":
        return alt0 + (i % nb + 0.5) * dalt
    if kind == "runs":
        return alt0 + ((i // 37) * 7 % nb + 0.25) * dalt
    if kind == "edges":
        return alt0 + ((i // 3) % (nb + 3) - 1).astype(np.float64) * dalt
    if kind == "wild":
        rng = np.random.default_rng(seed + n)
        a = alt0 + rng.uniform(-2.0, nb + 2.0, n) * dalt
        odd = np.array([np.nan, np.inf, -np.inf, 1e300, -1e300, 0.0, -0.0, 1e-320])
        where = rng.random(n) < 0.3
        a[where] = odd[rng.integers(0, len(odd), int(where.sum()))]
        return a
    raise ValueError(kind)


def built_table(nb, m, seed=3):
    """a table whose gains differ in every (band, column), with a gain of 0, gains below and above 256 and gains that clamp"""
    t = np.random.default_rng(seed).permutation(min(65536, 4 * nb * m))[:nb * m].astype(np.uint16)
    if not (t == 0).any():
        t[5] = 0
    assert len(set(t.tolist())) == nb * m
    return t.reshape(nb, m)


def effect_case(orc):
    """dict(sv, alts, raws (with the angle profile), flat (without), legs / legs_flat = [dict(gx, gy, norm, mask)], p = the grid,
    col = (S, C, gain, T) of the column table, S, C, gain, T = the banded statistics and table by the reference,
    corrected / corrected_col = the grey levels under the banded / the column table)"""
    if "case" in _CACHE:
        return _CACHE["case"]
    from diasss_amd.synth import Survey, angle_profile
    sv = Survey(F, N, M, seed=SEED)
    alts = [effect_alt(f) for f in range(F)]
    flat = [sv.frame(f).numpy() for f in range(F)]
    raws = [np.ascontiguousarray(flat[f] * angle_profile(M, alts[f], sv.gr, AMP, KCOS)) for f in range(F)]
    geo = [orc.geo_img(sv.poses_true[f], sv.gr, M) for f in range(F)]

    def legs_of(rs):
        return [dict(gx=geo[f][0], gy=geo[f][1], norm=orc.normalize(rs[f]), mask=orc.mask(rs[f])) for f in range(F)]
    legs, legs_flat = legs_of(raws), legs_of(flat)
    gx = np.concatenate([g[0].ravel() for g in geo]); gy = np.concatenate([g[1].ravel() for g in geo])
    p = K.grid(gx.min(), gx.max(), gy.min(), gy.max(), CELL)
    fr = [(L["norm"], L["mask"]) for L in legs]
    cS, cC = G.col_stats(fr, 1)
    cgain, cT = G.table(cS, cC, M, MIN_COUNT, SMOOTH, TARGET)
    S, C = B.band_stats(fr, alts, BANDS, 1)
    gain, T = B.table_banded(S, C, M, BANDS[2], MIN_COUNT, SMOOTH, TARGET)
    out = dict(sv=sv, alts=alts, raws=raws, flat=flat, legs=legs, legs_flat=legs_flat, p=p, col=(cS, cC, cgain, cT), S=S, C=C, gain=gain, T=T,
               corrected=[B.apply_banded(L["norm"], alts[f], gain, BANDS) for f, L in enumerate(legs)],
               corrected_col=[G.apply(L["norm"], cgain) for L in legs])
    _CACHE["case"] = out
    return out


def scores(orc):
    """the consistency scores of the effect case on the references: flat (no profile), none (profile, no table), column, banded"""
    if "scores" in _CACHE:
        return _CACHE["scores"]
    E = effect_case(orc)
    out = dict(flat=K.consistency(K.frames_of(E["legs_flat"]), E["p"], 1)[3], none=K.consistency(K.frames_of(E["legs"]), E["p"], 1)[3],
               column=K.consistency(K.frames_of(E["legs"], E["corrected_col"]), E["p"], 1)[3],
               banded=K.consistency(K.frames_of(E["legs"], E["corrected"]), E["p"], 1)[3])
    _CACHE["scores"] = out
    return out

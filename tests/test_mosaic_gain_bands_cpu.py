"""The altitude-banded range gain off the device: the band rule and the references against values worked out by hand, dsss_gain_band and
dsss_mosaic_gain_table_banded (pure host arithmetic of libdsss.so) against the reference bit for bit, and the precondition of the GPU
effect test on the references alone."""
import math

import numpy as np
import pytest

from tests import mosaic_gain_bands_cases as K
from tests import mosaic_gain_bands_ref as B
from tests import mosaic_gain_ref as G

E_ARG = -2
ODD = [float("nan"), float("inf"), float("-inf"), 1e300, -1e300, 0.0, -0.0, 5e-324]


# ---------------------------------------------------------------- the band rule
def _edge_alts(bands):
    alt0, dalt, nb = bands
    out = []
    for k in range(-2, nb + 3):
        e = alt0 + k * dalt
        out += [e, B.next_up(e), B.next_down(e)]
    return out + ODD + [alt0 - 100 * dalt, alt0 + 100 * dalt, alt0 + 0.5 * dalt]


@pytest.mark.parametrize("bands", [(7.0, 1.0, 6), (4.0, 0.75, 16), (-3.0, 0.1, 16), (10.0, 2.5, 1), (0.0, 1e-3, 2), (1e6, 1e5, 5)], ids=str)
def test_band_rule_by_hand(bands):
    alt0, dalt, nb = bands
    if (alt0, dalt) in ((7.0, 1.0), (4.0, 0.75), (10.0, 2.5)):                   # edges that are exact in f64
        for k in range(nb):
            e = alt0 + k * dalt
            assert B.band(bands, e) == k                                         # an edge belongs to the band above it
            assert B.band(bands, B.next_down(e)) == max(k - 1, 0)
            assert B.band(bands, B.next_up(e)) == k
        top = alt0 + nb * dalt
        assert B.band(bands, top) == nb - 1 and B.band(bands, B.next_down(top)) == nb - 1 and B.band(bands, top + 7 * dalt) == nb - 1
    assert B.band(bands, B.next_down(alt0)) == 0 and B.band(bands, alt0 - 3 * dalt) == 0
    assert B.band(bands, float("nan")) == 0 and B.band(bands, float("-inf")) == 0 and B.band(bands, float("inf")) == nb - 1
    assert B.band(bands, -1e300) == 0 and B.band(bands, 1e300) == nb - 1
    for a in _edge_alts(bands):
        assert 0 <= B.band(bands, a) < nb


@pytest.mark.parametrize("bands", [(7.0, 1.0, 6), (4.0, 0.75, 16), (-3.0, 0.1, 16), (10.0, 2.5, 1), (0.0, 1e-3, 2), (1e6, 1e5, 5), (0.3, 0.7, 16)], ids=str)
def test_library_band_matches_reference(bands):
    from diasss_amd import capi
    rng = np.random.default_rng(5)
    alts = _edge_alts(bands) + (bands[0] + rng.uniform(-2, bands[2] + 2, 200) * bands[1]).tolist()
    for a in alts:
        assert capi.gain_band(bands, a) == B.band(bands, a), (bands, a)
    assert capi.gain_band(capi.GainBands(*bands, 0), bands[0]) == 0


def test_library_band_argument_errors():
    from diasss_amd import capi
    L = capi.lib()
    out = capi.C.c_int32(77)

    def rc(alt0=7.0, dalt=1.0, nb=6, o=out, null=False):
        b = capi.GainBands(alt0, dalt, nb, 0)
        return L.dsss_gain_band(None if null else capi.C.byref(b), 8.5, capi.C.byref(o) if o is not None else None)
    assert rc() == 0 and out.value == 1
    assert rc(nb=0) == E_ARG and rc(nb=17) == E_ARG and rc(nb=-1) == E_ARG and rc(nb=16) == 0 and rc(nb=1) == 0
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert rc(alt0=bad) == E_ARG and rc(dalt=bad) == E_ARG
    assert rc(dalt=0.0) == E_ARG and rc(dalt=-1.0) == E_ARG and rc(dalt=-0.0) == E_ARG
    assert rc(null=True) == E_ARG and rc(o=None) == E_ARG
    with pytest.raises(capi.DsssError) as e:
        capi.gain_band((7.0, 0.0, 6), 8.0)
    assert e.value.code == E_ARG


# ---------------------------------------------------------------- the references of statistics, table and corrected sample
def _toy(rng, n, m):
    return rng.integers(0, 256, (n, m)).astype(np.uint8), (rng.random((n, m)) < 0.6).astype(np.uint8) * 9


@pytest.mark.parametrize("use_mask", [0, 1])
def test_band_stats_sum_to_col_stats(use_mask):
    rng = np.random.default_rng(2)
    bands = (4.0, 0.75, 16)
    frames = [_toy(rng, n, 10) for n in (50, 31)]
    for kind in K.SERIES:
        alts = [K.series(kind, f[0].shape[0], bands) for f in frames]
        S, C = B.band_stats(frames, alts, bands, use_mask)
        rS, rC = G.col_stats(frames, use_mask)
        assert [sum(S[b][c] for b in range(16)) for c in range(10)] == rS and [sum(C[b][c] for b in range(16)) for c in range(10)] == rC
        used = {B.band(bands, a) for alt in alts for a in alt}
        for b in range(16):
            assert (sum(C[b]) > 0) == (b in used), (kind, b)
        if kind == "cycle":
            assert used == set(range(16))
    # by hand: two pings in band 1, one in band 0
    norm = np.array([[1, 2], [10, 20], [100, 200]], np.uint8); mask = np.array([[1, 0], [1, 1], [0, 1]], np.uint8)
    S, C = B.band_stats([(norm, mask)], [[8.5, 7.0, 8.0]], (7.0, 1.0, 2), 1)
    assert S == [[10, 20], [1, 200]] and C == [[1, 1], [1, 1]]
    S, C = B.band_stats([(norm, mask)], [[8.5, 7.0, 8.0]], (7.0, 1.0, 2), 0)
    assert S == [[10, 20], [101, 202]] and C == [[1, 1], [2, 2]]


def _stat_cases():
    rng = np.random.default_rng(17)
    out = []
    for M in (2, 3, 6, 7, 31, 64, 401):
        for nb in (1, 2, 6, 16):
            C = rng.integers(0, 2 ** 31 // nb, (nb, M), endpoint=True)
            C[rng.random((nb, M)) < 0.2] = 0
            C[rng.random((nb, M)) < 0.3] //= 2 ** 21                          # counts around min_count
            if nb > 1:
                C[rng.integers(0, nb)] //= 2 ** 24                            # a thin band
            mean = rng.integers(0, 256, (nb, M))
            S = C * mean
            S[rng.random((nb, M)) < 0.1] = 0
            out.append((S.tolist(), C.tolist(), M, nb))
    out.append(([[255 * 2 ** 31] * 5] * 2, [[2 ** 31] * 5] * 2, 5, 2))          # counts near 2^31 in every band
    out.append(([[1] * 5, [255 * (2 ** 31 - 1)] * 5], [[2 ** 31 - 1] * 5] * 2, 5, 2))
    out.append(([[0] * 6] * 3, [[100] * 6] * 3, 6, 3))                         # nothing to normalise to: T = 0
    return out


def test_table_banded_one_band_is_the_column_table():
    for S, C, M, nb in _stat_cases():
        if nb != 1:
            continue
        for min_count, smooth, target in ((1, 0, 0), (256, 1, 0), (64, 16, 117)):
            g, T = B.table_banded(S, C, M, 1, min_count, smooth, target)
            assert (g[0], T) == G.table(S[0], C[0], M, min_count, smooth, target)


def test_table_banded_fallback_by_hand():
    # two bands of six columns; band 1 is thin (C' < min_count everywhere) and carries the pooled gains, never 256
    S = [[100, 300, 0, 400, 90, 50], [30, 30, 0, 40, 9, 5]]; C = [[10, 10, 10, 10, 10, 10], [1, 1, 1, 1, 1, 1]]
    g, T = B.table_banded(S, C, 6, 2, min_count=5, smooth=0, target=20)
    gp, Tp = G.table([130, 330, 0, 440, 99, 55], [11] * 6, 6, 5, 0, 20)
    assert T == Tp == 20 and g[1] == gp and 256 in gp and any(v != 256 for v in gp)
    assert g[0][0] == (20 * 10 * 256 + 50) // 100 == 512 and g[0][2] == gp[2] == 256 and g[0][3] == 128
    assert gp[0] == (20 * 11 * 256 + 65) // 130 == 433 != g[0][0]                                                    # (a band with samples of its own has gains of its own)
    # no eligible pooled column, no target: T = 0 and every gain is 256, whatever the bands hold
    g, T = B.table_banded([[0] * 6] * 3, [[100] * 6] * 3, 6, 3, min_count=1)
    assert T == 0 and g == [[256] * 6] * 3
    g, T = B.table_banded([[5] * 6] * 2, [[1] * 6] * 2, 6, 2, min_count=4, target=0)
    assert T == 0 and g == [[256] * 6] * 2
    # a band's window reaches min_count through smoothing, within its side only
    S = [[10, 20, 30, 1000, 2000, 3000], [0] * 6]; C = [[1] * 6, [0] * 6]
    g, T = B.table_banded(S, C, 6, 2, min_count=2, smooth=1, target=100)
    assert g[0] == G.table(S[0], C[0], 6, 2, 1, 100)[0] and g[1] == g[0]       # the empty band: the pooled column, which here is band 0's


def test_apply_banded_by_hand():
    v = np.array([[0, 1, 100, 255]] * 4, np.uint8)
    gain = [[256, 256, 256, 256], [0, 128, 384, 257], [65535] * 4]
    out = B.apply_banded(v, [7.5, 8.0, 9.999, float("nan")], gain, (7.0, 1.0, 3))
    assert out.tolist() == [[0, 1, 100, 255], [0, 1, 150, 255], [0, 255, 255, 255], [0, 1, 100, 255]]
    assert (B.apply_banded(v, [1.0] * 4, [[300, 2, 5, 7]], (0.0, 1.0, 1)) == G.apply(v, [300, 2, 5, 7])).all()


# ---------------------------------------------------------------- dsss_mosaic_gain_table_banded against the reference
@pytest.mark.parametrize("smooth", [0, 1, 16])
def test_library_table_banded_matches_reference(smooth):
    from diasss_amd import capi
    seen = set()
    for S, C, M, nb in _stat_cases():
        for min_count, target in ((1, 0), (256, 0), (64, 117), (2 ** 31 - 1, 255)):
            g, T = capi.mosaic_gain_table(np.array(S, np.uint64), np.array(C, np.uint64), capi.GainParams(min_count, smooth, target, 0), nbands=nb)
            rg, rT = B.table_banded(S, C, M, nb, min_count, smooth, target)
            assert g.dtype == np.uint16 and g.shape == (nb, M) and g.tolist() == rg and T == rT, (S, C, min_count, smooth, target)
            if nb == 1:
                g1, T1 = capi.mosaic_gain_table(np.array(S[0], np.uint64), np.array(C[0], np.uint64), capi.GainParams(min_count, smooth, target, 0))
                assert g1.tolist() == g[0].tolist() and T1 == T
            gp = B.table_banded([[sum(S[b][c] for b in range(nb)) for c in range(M)]], [[sum(C[b][c] for b in range(nb)) for c in range(M)]], M, 1, min_count, smooth, target)[0][0]
            flat = [v for r in rg for v in r]
            seen.update(["sat"] if 65535 in flat else []); seen.update(["none"] if rT == 0 else [])
            seen.update(["own"] if any(r != gp for r in rg) else []); seen.update(["fallback"] if nb > 1 and rT > 0 and any(r == gp and any(v != 256 for v in gp) for r in rg) else [])
    assert seen == {"sat", "none", "own", "fallback"}                                    # no branch of the rule went unvisited


def test_library_table_banded_default_params_and_errors():
    from diasss_amd import capi
    L = capi.lib()
    P = capi._ptr
    S = np.array([[1000 * k for k in range(1, 9)]] * 2, np.uint64); C = np.full((2, 8), 300, np.uint64)
    g, T = capi.mosaic_gain_table(S, C, None, nbands=2)                                  # NULL parameters: the defaults
    assert (g.tolist(), T) == B.table_banded(S.tolist(), C.tolist(), 8, 2, 256, 0, 0)
    out = np.zeros((2, 8), np.uint16)

    def rc(s=S, c=C, M=8, nb=2, o=out, **kw):
        p = capi.gain_params_default()
        for k, v in kw.items():
            setattr(p, k, v)
        return L.dsss_mosaic_gain_table_banded(P(s), P(c), M, nb, p, P(o), None)
    assert rc() == 0                                                                     # (target_out may be NULL)
    assert rc(s=None) == E_ARG and rc(c=None) == E_ARG and rc(o=None) == E_ARG
    assert rc(M=1) == E_ARG and rc(M=0) == E_ARG and rc(M=-8) == E_ARG
    assert rc(nb=0) == E_ARG and rc(nb=-1) == E_ARG and rc(nb=17) == E_ARG
    assert rc(min_count=0) == E_ARG and rc(smooth=-1) == E_ARG and rc(smooth=17) == E_ARG and rc(smooth=16) == 0
    assert rc(target=-1) == E_ARG and rc(target=256) == E_ARG and rc(target=255) == 0
    big = np.zeros((16, 8), np.uint64); bigo = np.zeros((16, 8), np.uint16)
    assert rc(s=big, c=big, nb=16, o=bigo) == 0 and (bigo == 256).all()


# ---------------------------------------------------------------- the precondition of the GPU effect test
def test_effect_precondition(orc):
    """An angle-fixed profile under a changing altitude: the column table takes part of it back, the banded table most of it.  Only the
    ordering is asserted.  Measured on the references, in grey levels: flat (no profile) 5.42, profile and no table 32.01, column table
    19.83, banded table (6 bands of 1 m from 7 m, min_count 64, smooth 8) 9.29."""
    s = K.scores(orc)
    E = K.effect_case(orc)
    print("T %d (column table %d); score flat %.3f, none %.3f, column %.3f, banded %.3f" % (E["T"], E["col"][3], s["flat"], s["none"], s["column"], s["banded"]))
    assert s["banded"] < s["column"] < s["none"]
    assert s["flat"] < s["banded"]
    assert math.isfinite(s["banded"]) and E["T"] == E["col"][3] > 0
    used = {B.band(K.BANDS, a) for alt in E["alts"] for a in alt}
    assert used == set(range(K.BANDS[2]))                                                # every band of the table holds pings

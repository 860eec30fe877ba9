"""The range-gain normalisation off the device: the Python-integer reference against values worked out by hand, dsss_mosaic_gain_table
(pure host arithmetic of libdsss.so) against the reference bit for bit, and the precondition of the GPU effect test on the references
alone."""
import numpy as np
import pytest

from tests import mosaic_gain_cases as K
from tests import mosaic_gain_ref as G

E_ARG = -2


# ---------------------------------------------------------------- the reference itself, by hand on six columns
S6 = [100, 300, 0, 400, 1, 50]
C6 = [10, 10, 10, 10, 1000000, 2]


def test_reference_table_by_hand():
    # min_count 5: columns 0, 1, 3, 4 are eligible (2: S = 0, 5: C = 2 < 5); a given target
    g, T = G.table(S6, C6, 6, min_count=5, smooth=0, target=20)
    assert T == 20
    assert g[0] == (20 * 10 * 256 + 50) // 100 == 512              # mean 10 -> 20: a gain of 2
    assert g[1] == (20 * 10 * 256 + 150) // 300 == 171             # mean 30 -> 20: 170.67 rounds to 171
    assert g[2] == 256                                              # S' = 0: not eligible
    assert g[3] == (20 * 10 * 256 + 200) // 400 == 128
    assert g[4] == 65535                                            # S' = 1 under a million samples: 5.12e9 saturates
    assert g[5] == 256                                              # C' = 2 < min_count
    # pooled target: the eligible columns' UNsmoothed sums
    g, T = G.table([100, 300, 0, 400, 90, 50], [10, 10, 10, 10, 4, 2], 6, min_count=5, smooth=0, target=0)
    assert T == (800 + 15) // 30 == 27 and g[4] == 256 and g[5] == 256
    assert g[0] == (27 * 10 * 256 + 50) // 100 == 691 and g[3] == (27 * 10 * 256 + 200) // 400 == 173
    # target given against pooled: the same columns, another level
    g2, T2 = G.table([100, 300, 0, 400, 90, 50], [10, 10, 10, 10, 4, 2], 6, min_count=5, smooth=0, target=54)
    assert T2 == 54 and g2[0] == (54 * 10 * 256 + 50) // 100 and g2[0] != g[0] and g2[4] == 256


def test_reference_smooth_does_not_cross_the_nadir():
    S = [10, 20, 30, 1000, 2000, 3000]; C = [1, 1, 1, 1, 1, 1]
    g, T = G.table(S, C, 6, min_count=1, smooth=1, target=100)
    # column 2 is the last of its side: its window is {1, 2}, not {1, 2, 3}; column 3 the first of the other: {3, 4}
    assert g[2] == (100 * 2 * 256 + 25) // 50 == 1024
    assert g[3] == (100 * 2 * 256 + 1500) // 3000 == 17
    assert g[0] == (100 * 2 * 256 + 15) // 30 and g[1] == (100 * 3 * 256 + 30) // 60 and g[5] == (100 * 2 * 256 + 2500) // 5000
    # eligibility is by the smoothed count: alone no column has 2 samples
    assert G.table(S, C, 6, min_count=2, smooth=0, target=100) == ([256] * 6, 0)
    assert G.table(S, C, 6, min_count=2, smooth=1, target=100)[0] == g
    # a window wider than a side covers the side and nothing else
    gw, _ = G.table(S, C, 6, min_count=1, smooth=16, target=100)
    assert gw[0] == gw[1] == gw[2] == (100 * 3 * 256 + 30) // 60 and gw[3] == gw[4] == gw[5] == (100 * 3 * 256 + 3000) // 6000


def test_reference_no_eligible_column():
    assert G.table([0] * 6, [100] * 6, 6, min_count=1) == ([256] * 6, 0)
    assert G.table([5] * 6, [3] * 6, 6, min_count=4, target=9) == ([256] * 6, 0)
    # eligible through its neighbours only, and none of the eligible columns holds a sample of its own: no pooled mean exists
    assert G.table([0, 50, 0, 50, 0, 0, 0, 0, 0, 0], [0, 5, 0, 5, 0, 0, 0, 0, 0, 0], 10, min_count=10, smooth=1, target=0) == ([256] * 10, 0)
    g, T = G.table([0, 50, 0, 50, 0, 0, 0, 0, 0, 0], [0, 5, 0, 5, 0, 0, 0, 0, 0, 0], 10, min_count=10, smooth=1, target=10)
    assert T == 10 and g == [256, 256, (10 * 10 * 256 + 50) // 100, 256, 256, 256, 256, 256, 256, 256]


def test_reference_stats_and_apply():
    norm = np.array([[1, 2, 3, 4], [5, 6, 7, 8]], np.uint8); mask = np.array([[1, 0, 255, 0], [0, 0, 7, 1]], np.uint8)
    assert G.col_stats([(norm, mask)], 0) == ([6, 8, 10, 12], [2, 2, 2, 2])
    assert G.col_stats([(norm, mask)], 1) == ([1, 0, 10, 8], [1, 0, 2, 1])
    assert G.col_stats([(norm, mask), (norm, mask)], 1) == ([2, 0, 20, 16], [2, 0, 4, 2])
    v = np.array([[0, 1, 100, 255]] * 3, np.uint8)
    assert G.apply(v, [256] * 4).tolist() == v.tolist()
    assert G.apply(v, [0, 128, 384, 257]).tolist() == [[0, 1, 150, 255]] * 3          # (128 + 128) >> 8 = 1; 255 x 257 clamps
    assert G.apply(v, [65535] * 4).tolist() == [[0, 255, 255, 255]] * 3


def test_unity_gain_returns_every_value():
    v = np.arange(256, dtype=np.uint8).reshape(1, 256)
    assert (G.apply(v, [256] * 256) == v).all()


# ---------------------------------------------------------------- dsss_mosaic_gain_table against the reference
def _lib_table(capi, S, C, **kw):
    p = capi.gain_params_default()
    for k, v in kw.items():
        setattr(p, k, v)
    return capi.mosaic_gain_table(np.array(S, np.uint64), np.array(C, np.uint64), p)


def _cases():
    rng = np.random.default_rng(11)
    out = [(S6, C6), ([100, 300, 0, 400, 90, 50], [10, 10, 10, 10, 4, 2]), ([0] * 6, [100] * 6), ([0, 50, 0, 50, 0, 0, 0, 0, 0, 0], [0, 5, 0, 5, 0, 0, 0, 0, 0, 0]),
           ([1, 255 * 2 ** 31], [2 ** 31, 2 ** 31]), ([255 * 2 ** 31] * 7, [2 ** 31] * 7), ([1] * 5, [2 ** 31] * 5)]
    for M in (2, 3, 6, 7, 31, 64, 401):
        C = rng.integers(0, 2 ** 31, M, endpoint=True)
        C[rng.random(M) < 0.2] = 0
        C[rng.random(M) < 0.2] //= 2 ** 22                               # counts around min_count
        mean = rng.integers(0, 256, M)
        S = np.array([int(c) * int(m) for c, m in zip(C, mean)], dtype=object)
        S[rng.random(M) < 0.1] = 0
        out.append(([int(v) for v in S], [int(v) for v in C]))
    return out


def test_default_params():
    from diasss_amd import capi
    p = capi.gain_params_default()
    assert (p.min_count, p.smooth, p.target, p.pad_) == (256, 0, 0, 0)
    S, C = [1000 * k for k in range(1, 9)], [300] * 8
    g, T = capi.mosaic_gain_table(np.array(S, np.uint64), np.array(C, np.uint64))          # NULL parameters: the defaults
    assert (g.tolist(), T) == G.table(S, C, 8, 256, 0, 0)


@pytest.mark.parametrize("smooth", [0, 1, 16])
def test_library_table_matches_reference(smooth):
    from diasss_amd import capi
    seen = set()
    for S, C in _cases():
        for min_count, target in ((1, 0), (256, 0), (64, 117), (2 ** 31 - 1, 255)):
            g, T = _lib_table(capi, S, C, min_count=min_count, smooth=smooth, target=target)
            rg, rT = G.table(S, C, len(S), min_count, smooth, target)
            assert g.dtype == np.uint16 and g.tolist() == rg and T == rT, (S, C, min_count, smooth, target)
            seen.update(["sat"] if 65535 in rg else []); seen.update(["plain"] if any(v not in (256, 65535) for v in rg) else [])
            seen.update(["none"] if rT == 0 else [])
    assert seen == {"sat", "plain", "none"}                                              # no branch of the rule went unvisited


def test_library_table_argument_errors():
    from diasss_amd import capi
    L = capi.lib()
    S = np.array([10, 20, 30, 40], np.uint64); C = np.array([1, 1, 1, 1], np.uint64); g = np.zeros(4, np.uint16)
    P = capi._ptr

    def rc(s=S, c=C, M=4, out=g, **kw):
        p = capi.gain_params_default()
        for k, v in kw.items():
            setattr(p, k, v)
        return L.dsss_mosaic_gain_table(P(s), P(c), M, p, P(out), None)
    assert rc() == 0                                                 # (target_out may be NULL)
    assert rc(s=None) == E_ARG and rc(c=None) == E_ARG and rc(out=None) == E_ARG
    assert rc(M=1) == E_ARG and rc(M=0) == E_ARG and rc(M=-4) == E_ARG
    assert rc(min_count=0) == E_ARG and rc(min_count=-1) == E_ARG
    assert rc(smooth=-1) == E_ARG and rc(smooth=17) == E_ARG and rc(smooth=16) == 0
    assert rc(target=-1) == E_ARG and rc(target=256) == E_ARG and rc(target=255) == 0
    with pytest.raises(capi.DsssError) as e:
        capi.mosaic_gain_table(S[:1], C[:1])
    assert e.value.code == E_ARG


# ---------------------------------------------------------------- the precondition of the GPU effect test
def test_effect_precondition(orc):
    """The profile makes true poses score badly, the table takes most of that back: conditions under which the GPU test's equalities
    mean something, not tolerances.  Measured: score 21.914 -> 10.843 (x 0.495; 5.420 without a profile), ZNCC 0.7667 -> 0.9377 (0.9827), 0.04 % of
    the corrected samples at 255, T = 117."""
    E = K.effect_case(orc)
    p = E["p"]
    raw_f = K.frames_of(E["legs"]); cor_f = K.frames_of(E["legs"], E["corrected"]); flat_f = K.frames_of(E["legs_flat"])
    s_raw, s_cor, s_flat = (K.consistency(f, p, 1)[3] for f in (raw_f, cor_f, flat_f))
    z_raw, z_cor, z_flat = (K.zncc0(f, p, 1) for f in (raw_f, cor_f, flat_f))
    kept = [L["mask"] != 0 for L in E["legs"]]
    at255 = sum(int((c[k] == 255).sum()) for c, k in zip(E["corrected"], kept)) / sum(int(k.sum()) for k in kept)
    print("T %d; score %.3f -> %.3f (none: %.3f); zncc0 %.4f -> %.4f (none: %.4f); %.2f %% at 255" % (E["T"], s_raw, s_cor, s_flat, z_raw, z_cor, z_flat, 100 * at255))
    assert s_cor < 0.6 * s_raw
    assert z_cor >= z_raw + 0.1
    assert at255 < 0.02
    assert s_flat < s_cor and z_flat > z_cor                         # (for scale: the table does not beat having no profile)

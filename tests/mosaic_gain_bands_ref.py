"""Numpy / Python-integer reference of the altitude-banded range gain (include/dsss.h, "altitude-banded range gain"), written from the
definition and from nothing else: built on tests/mosaic_gain_ref.py.  Nothing in it calls the library."""
import math

import numpy as np

from tests import mosaic_gain_ref as G


def band(bands, alt):
    """bands = (alt0, dalt, nbands): the band of the altitude alt.  t = floor((alt - alt0) / dalt) in f64; 0 when not t >= 0 (NaN, -inf,
    below alt0), nbands - 1 when t >= nbands"""
    alt0, dalt, nbands = bands
    with np.errstate(all="ignore"):
        t = np.floor((np.float64(alt) - np.float64(alt0)) / np.float64(dalt))
    if not (t >= 0.0):
        return 0
    if t >= float(nbands):
        return nbands - 1
    return int(t)


def bands_of(bands, alt):
    return np.array([band(bands, a) for a in np.asarray(alt, np.float64)], np.int64)


def band_stats(frames, alts, bands, use_mask):
    """frames: list of (norm, mask) as mosaic_gain_ref.col_stats takes them, alts: the altitudes of each frame's pings -> (S, C):
    nbands lists of M Python integers each, the statistics of the pings of every band"""
    nb = bands[2]
    M = frames[0][0].shape[1]
    S = [[0] * M for _ in range(nb)]; C = [[0] * M for _ in range(nb)]
    for (norm, mask), alt in zip(frames, alts):
        assert len(alt) == norm.shape[0]
        bs = bands_of(bands, alt)
        for b in range(nb):
            rows = bs == b
            if not rows.any():
                continue
            s, c = G.col_stats([(norm[rows], mask[rows])], use_mask)
            S[b] = [x + y for x, y in zip(S[b], s)]; C[b] = [x + y for x, y in zip(C[b], c)]
    return S, C


def table_banded(S, C, M, nbands, min_count=256, smooth=0, target=0):
    """(gain, T): nbands lists of M gains and the grey level.  Pooled table gp, T = mosaic_gain_ref.table on the sums over the bands;
    entry (b, c) is eligible iff C'_b[c] >= min_count and S'_b[c] > 0 and T > 0 and gets min(65535, (T C' 256 + S' // 2) // S'),
    every other entry gp[c]"""
    S = [[int(v) for v in r] for r in S]; C = [[int(v) for v in r] for r in C]
    assert len(S) == nbands and len(C) == nbands and all(len(r) == M for r in S + C)
    Sp = [sum(S[b][c] for b in range(nbands)) for c in range(M)]; Cp = [sum(C[b][c] for b in range(nbands)) for c in range(M)]
    gp, T = G.table(Sp, Cp, M, min_count, smooth, target)
    half = M // 2
    gain = []
    for b in range(nbands):
        row = []
        for c in range(M):
            side = range(0, half) if c < half else range(half, M)
            win = [k for k in range(c - smooth, c + smooth + 1) if k in side]
            s = sum(S[b][k] for k in win); n = sum(C[b][k] for k in win)
            row.append(min(65535, (T * n * 256 + s // 2) // s) if (n >= min_count and s > 0 and T > 0) else gp[c])
        gain.append(row)
    return gain, T


def apply_banded(norm, alt, gain, bands):
    """the corrected samples of a frame: v' = min(255, (v gain[band(alt[row])][c] + 128) >> 8), uint8"""
    gain = np.asarray(gain, np.int64).reshape(bands[2], -1)
    rows = gain[bands_of(bands, alt)]                                   # N x M
    v = (np.asarray(norm).astype(np.int64) * rows + 128) >> 8
    return np.minimum(v, 255).astype(np.uint8)


def next_up(x):
    return math.nextafter(x, math.inf)


def next_down(x):
    return math.nextafter(x, -math.inf)

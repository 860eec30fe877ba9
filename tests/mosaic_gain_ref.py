"""Numpy / Python-integer reference of the range-gain normalisation (include/dsss.h, "range-gain normalisation"), written from the
definition and from nothing else.  Nothing in it calls the library."""
import numpy as np


def col_stats(frames, use_mask):
    """frames: list of (norm uint8 N x M, mask uint8 N x M), all of one M -> (S, C): Python integers per column, the sum and the
    number of the kept samples (use_mask: the samples whose mask is not 0)"""
    M = frames[0][0].shape[1]
    S = [0] * M; C = [0] * M
    for norm, mask in frames:
        assert norm.shape[1] == M and mask.shape == norm.shape
        keep = (mask != 0) if use_mask else np.ones(norm.shape, bool)
        s = np.where(keep, norm.astype(np.int64), 0).sum(axis=0); c = keep.sum(axis=0)
        for k in range(M):
            S[k] += int(s[k]); C[k] += int(c[k])
    return S, C


def table(S, C, M, min_count=256, smooth=0, target=0):
    """(gain, T): M gains (Python integers, Q8, at most 65535) and the grey level the columns are brought to"""
    S = [int(v) for v in S]; C = [int(v) for v in C]
    assert len(S) == M and len(C) == M
    half = M // 2
    Ss, Cs, elig = [], [], []
    for c in range(M):
        side = range(0, half) if c < half else range(half, M)
        win = [k for k in range(c - smooth, c + smooth + 1) if k in side]          # never across the nadir
        Ss.append(sum(S[k] for k in win)); Cs.append(sum(C[k] for k in win))
        elig.append(Cs[c] >= min_count and Ss[c] > 0)
    tS = sum(S[c] for c in range(M) if elig[c]); tC = sum(C[c] for c in range(M) if elig[c])
    if not any(elig) or (target == 0 and tC == 0):
        return [256] * M, 0
    T = target if target != 0 else (tS + tC // 2) // tC
    return [min(65535, (T * Cs[c] * 256 + Ss[c] // 2) // Ss[c]) if elig[c] else 256 for c in range(M)], T


def apply(norm, gain):
    """the corrected samples: v' = min(255, (v gain[c] + 128) >> 8), uint8, gain per column of the last axis"""
    v = (np.asarray(norm).astype(np.int64) * np.asarray(gain, np.int64) + 128) >> 8
    return np.minimum(v, 255).astype(np.uint8)


def profile(M, amp):
    """the sensor profile of the effect tests: prof[c] = 1 + amp cos(3 r) (1 on starboard, 0.8 on port), r = |c - M/2| / (M/2)"""
    c = np.arange(M, dtype=np.float64)
    r = np.abs(c - M / 2) / (M / 2)
    return 1.0 + amp * np.cos(3.0 * r) * np.where(c >= M / 2, 1.0, 0.8)

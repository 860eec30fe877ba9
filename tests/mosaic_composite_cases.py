"""The two legs of the composite-mosaic tests, shared by tests/test_mosaic_composite_cpu.py (the preconditions, on the reference alone)
and tests/test_gpu_mosaic_composite.py (the device against the same numbers): the legs of tests/test_gpu_mosaic.py
(helpers.MOSAIC_SIZES, seeded Rayleigh images) with the oracle's geo_img, normalised image and mask.  Nothing here calls the library.
Computed once per session; nobody writes into the arrays."""
import numpy as np

from tests import mosaic_composite_ref as CR
from tests import mosaic_gain_cases as K
from tests.helpers import MOSAIC_SIZES as SIZES

# the pings of leg 0 a trajectory override makes NaN: gaps of 1, 3, 6 and 12 pings, which fill radii 1, 2 and 4 close differently
BAD_PINGS = [100] + list(range(200, 203)) + list(range(300, 306)) + list(range(400, 412))
_CACHE = {}
grid = K.grid                                    # dsss_mosaic_grid's rule, restated (tests/mosaic_gain_cases.py)


def legs(orc):
    """leg 0 at 640 x 400 heading +x, leg 1 at 500 x 700 heading back over it -> dicts of N, M, pose, alt, gr, raw, gx, gy, norm, mask"""
    if "legs" not in _CACHE:
        from tests import helpers as H
        out = []
        for leg, (N, M) in enumerate(SIZES):
            pose, alt, gr = H.track(N, M, leg, seed=9)
            raw = np.random.default_rng(leg).rayleigh(1.0, (N, M)) * 100.0
            gx, gy = orc.geo_img(pose, gr, M)
            out.append(dict(N=N, M=M, pose=pose, alt=alt, gr=gr, raw=raw, gx=gx, gy=gy, norm=orc.normalize(raw), mask=orc.mask(raw)))
        _CACHE["legs"] = out
    return _CACHE["legs"]


def frames(L, ids=(0, 1), keep=None):
    """the reference's frame records of the legs under their dead-reckoning poses: leg k as frame ids[k]; keep[k]: bool per ping"""
    return [dict(id=i, gx=l["gx"], gy=l["gy"], norm=l["norm"], mask=l["mask"], keep=None if keep is None else keep[k])
            for k, (i, l) in enumerate(zip(ids, L))]


def full_grid(L, cell, use_mask):
    gx = np.concatenate([l["gx"].ravel() for l in L]); gy = np.concatenate([l["gy"].ravel() for l in L])
    return grid(gx.min(), gx.max(), gy.min(), gy.max(), cell, use_mask)


def bad_keep(L):
    keep = [np.ones(l["N"], bool) for l in L]
    keep[0][BAD_PINGS] = False
    return keep


def reference(orc, cell, use_mask, mode, R=0, bad=False):
    """CR.composite of the two legs on their full grid, cached by its arguments"""
    key = (cell, use_mask, mode, R, bad)
    if key not in _CACHE:
        L = legs(orc)
        _CACHE[key] = CR.composite(frames(L, keep=bad_keep(L) if bad else None), full_grid(L, cell, use_mask), use_mask, mode, R)
    return _CACHE[key]

"""The case table of the peak rule (include/dsss.h, "overlap registration": score, peak, ties, sub-cell offset) and a reference of it
written from the header's definition alone, with a trace of the branches a table takes.  Python integers for num, da, db; float(int)
for the one conversion each (nearest, ties to even); math.sqrt, /, the order and the parabola left to right.

Designed sums stay below 2^60, so signed 128-bit products of two of them cannot overflow.  A designed shift is (n, 0, 0, k, q, q):
num = n k, da = db = n q, so z = float(n k) / sqrt(float(n q)^2), and equal sums give equal bits."""
import math
import numpy as np

from tests import mosaic_register_ref as R

RADII = (0, 1, 3, 8, 16)
MIN_CELLS = 50
CELL = 0.1
REC_BYTES = 64


# ---------------------------------------------------------------- the reference
def conv(v, trace=None, truncate=False):
    """float(v) of an exact integer, with the rounding case it is noted in trace.  Two wrong conversions to hold it against:
    truncate="53": the bits beyond 53 dropped; truncate="64": above 2^64 cut to 64 bits WITHOUT a sticky bit, then rounded"""
    a = abs(v)
    bits = a.bit_length()
    if bits > 53:
        sh = bits - 53
        q, rem, half = a >> sh, a & ((1 << sh) - 1), 1 << (sh - 1)
        if trace is not None and bits > 64:
            if rem == half:
                trace.add("conv_tie_even" if q % 2 == 0 else "conv_tie_odd")
            cut = bits - 64                                   # a 64-bit cut without a sticky bit would see a tie here
            if (a >> cut) & 0x7ff == 0x400 and a & ((1 << cut) - 1):
                trace.add("conv_sticky")
        if truncate == "53":
            return math.copysign(float(q << sh), v)
        if truncate == "64" and bits > 64:
            return math.copysign(float((a >> (bits - 64)) << (bits - 64)), v)
    return float(v)


def score(s6, min_cells, trace=None, truncate=False):
    n, Sa, Sb, Sab, Saa, Sbb = (int(v) for v in s6)
    num = n * Sab - Sa * Sb; da = n * Saa - Sa * Sa; db = n * Sbb - Sb * Sb
    if n < min_cells or da <= 0 or db <= 0:
        if trace is not None:
            trace.add("unusable_n" if n < min_cells else "unusable_da" if da <= 0 else "unusable_db")
        return -2.0, False
    return conv(num, trace, truncate) / math.sqrt(conv(da, trace, truncate) * conv(db, trace, truncate)), True


def peak(sums, radius, min_cells, cell, truncate=False):
    """-> (record as a dict of the fields of dsss_reg_result, the set of branches taken)"""
    S = 2 * radius + 1
    sums = np.asarray(sums, dtype=object).reshape(S, S, 6)
    tr = set()
    z = [[score(sums[j, i], min_cells, tr, truncate) for i in range(S)] for j in range(S)]
    usable = sorted((-z[dy + radius][dx + radius][0], dx * dx + dy * dy, dy, dx)
                    for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1) if z[dy + radius][dx + radius][1])
    n0 = int(sums[radius, radius, 0])
    res = dict(dx=0, dy=0, off_x=0.0, off_y=0.0, zncc=-2.0, zncc0=z[radius][radius][0], n=n0, n0=n0, on_border=0)
    if not usable:
        tr.add("none_usable")
        return res, tr
    if len(usable) == 1 and S > 1:
        tr.add("one_usable")
    w = usable[0]
    if len(usable) > 1 and usable[1][0] == w[0]:
        u = usable[1]
        tr.add("tie_d2" if w[1] < u[1] else "tie_dy" if w[2] < u[2] else "tie_dx")
        if len(usable) == S * S and usable[-1][0] == w[0]:
            tr.add("all_equal")
    _, _, dy, dx = w
    j, i = dy + radius, dx + radius
    z0 = z[j][i][0]
    if z0 < 0.0:
        tr.add("negative_peak")
    res.update(dx=dx, dy=dy, zncc=z0, n=int(sums[j, i, 0]), on_border=int(abs(dx) == radius or abs(dy) == radius))
    px = py = 0.0
    if res["on_border"]:
        tr.add("border_corner" if abs(dx) == radius and abs(dy) == radius else "border_side")
        tr.add("border_%s%s" % ("" if dy != radius and dy != -radius else "n" if dy < 0 else "s", "" if dx != radius and dx != -radius else "w" if dx < 0 else "e"))
    else:
        ok = []
        for (zm, okm), (zp, okp) in ((z[j][i - 1], z[j][i + 1]), (z[j - 1][i], z[j + 1][i])):
            p = 0.0
            ok.append(okm and okp)
            if okm and okp:
                den = zm - 2.0 * z0 + zp
                if den < 0.0:
                    p = 0.5 * (zm - zp) / den
                    tr.add("parabola")
                else:
                    tr.add("plateau")
            if len(ok) == 1:
                px = p
            else:
                py = p
        if ok[0] != ok[1]:
            tr.add("neighbour_unusable_one_axis")
    res["off_x"] = (float(dx) + px) * cell; res["off_y"] = (float(dy) + py) * cell
    return res, tr


def record_bytes(res):
    """the 64 bytes of a dsss_reg_result with these fields, pad_ = 0"""
    return (np.array([res["dx"], res["dy"]], np.int32).tobytes() + np.array([res["off_x"], res["off_y"], res["zncc"], res["zncc0"]], np.float64).tobytes()
            + np.array([res["n"], res["n0"]], np.int64).tobytes() + np.array([res["on_border"], 0], np.int32).tobytes())


# ---------------------------------------------------------------- designed shifts
def e(k, q=1000, n=400):
    """a usable shift with z = k / q (for n q below 2^26 exactly the nearest double of it)"""
    return [n, 0, 0, k, q, q]


NEG = [400, 1000, 1000, 0, 10000, 10000]          # num = -10^6, da = db = 3 10^6: z = -1/3
NEG2 = [400, 1000, 1000, 0, 20000, 20000]         # z = -1/7
FEW = [MIN_CELLS - 1, 0, 0, 900, 1000, 1000]      # n below min_cells
FLAT = [400, 4000, 4000, 40000, 40000, 40000]     # constant layers (10 everywhere): da = db = 0


def _near_tie(odd, above):
    """(n, Saa) with n Saa above 2^64: an exact tie of the conversion whose kept part is odd / even, or (above) a tie plus a rest
    that lies wholly below a 64-bit cut, where only the sticky bit decides"""
    tie = ((1 << 53) + (3 if odd else 1)) << 20                                 # 74 bits: 53 kept, then 1 0 0 ... 0
    if not above:
        return 1 << 20, (1 << 53) + (3 if odd else 1)
    n = (1 << 20) + 1
    while True:
        Saa = -(-tie // n)
        rest = n * Saa - tie
        if 0 < rest < (1 << 10) and Saa < (1 << 60):
            return n, Saa
        n += 2


def conv_shift(which, odd=False, above=False):
    """a usable shift with the rounding case in num (which = 'num') or in da ('da'); the other quantities are plain"""
    n, big = _near_tie(odd, above)
    if which == "num":
        return [n, 0, 0, big, 1 << 54, 1 << 54]                                # da = db = n 2^54 convert exactly: z about 1/2 shows num's rounding
    return [n, 0, 0, big >> 1, big, 1 << 54]


def table(radius, entries, fill=None):
    S = 2 * radius + 1
    t = np.zeros((S, S, 6), np.uint64)
    if fill is not None:
        t[:, :] = fill
    for (dx, dy), s6 in entries.items():
        t[dy + radius, dx + radius] = s6
    return t


def real_table(radius, seed):
    """the sums of two random u8 layers with holes, b = a moved by a shift inside the square (the numpy reference's sums)"""
    rng = np.random.default_rng(seed)
    n = 40 + 2 * radius
    big = rng.integers(0, 256, (n + 2 * radius, n + 2 * radius))
    dx, dy = (int(v) for v in rng.integers(-radius, radius + 1, 2)) if radius else (0, 0)
    ma = big[radius:radius + n, radius:radius + n]
    mb = big[radius - dy:radius - dy + n, radius - dx:radius - dx + n] if seed % 3 else rng.integers(0, 256, (n, n))      # every third: unrelated layers
    mb = np.where(rng.random((n, n)) < 0.7, mb, rng.integers(0, 256, (n, n)))                                             # and noise, so that z < 1
    va = rng.random((n, n)) > 0.15; vb = rng.random((n, n)) > 0.15
    va[5:12, 8:30] = False; vb[20:33, 3:9] = False
    return R.shift_sums(ma, va, mb, vb, radius).astype(np.uint64)


def cases(radius):
    """[(name, table)] for one radius; every table is (2 radius + 1)^2 x 6 uint64"""
    r = radius
    out = [("real %d" % s, real_table(r, 100 * r + s)) for s in range(4)]
    z = lambda ent=None, fill=None: table(r, ent or {}, fill)
    out += [("zeros", z()), ("few everywhere", z(fill=FEW)), ("flat everywhere", z(fill=FLAT)), ("negative alone", z({(0, 0): NEG})),
            ("negative best", z({(0, 0): NEG2}, fill=NEG)),
            ("conv num tie even", z({(0, 0): conv_shift("num")})), ("conv num tie odd", z({(0, 0): conv_shift("num", odd=True)})),
            ("conv num sticky", z({(0, 0): conv_shift("num", above=True)})), ("conv num sticky odd", z({(0, 0): conv_shift("num", odd=True, above=True)})),
            ("conv da tie even", z({(0, 0): conv_shift("da")})), ("conv da tie odd", z({(0, 0): conv_shift("da", odd=True)})),
            ("conv da sticky", z({(0, 0): conv_shift("da", above=True)}))]
    if r == 0:
        return out
    m = r - 1 if r > 1 else 0                                                   # a shift whose neighbours exist (r == 1: the centre)
    out += [("few but one", z({(r, -r): e(700)}, fill=FEW)), ("few but the centre", z({(0, 0): e(700)}, fill=FEW)), ("few but one inside", z({(-m, m): e(700)}, fill=FEW)),
            # ties: equal sums at several shifts
            ("tie by d2", z({(r, r): e(900), (0, 1): e(900)}, fill=e(100))),
            ("tie by d2, centre", z({(r, -r): e(900), (0, 0): e(900)}, fill=e(100))),
            ("tie by d2, negative", z({(1, 1): NEG2, (0, -1): NEG2}, fill=NEG)),
            ("tie by dy", z({(0, 1): e(900), (0, -1): e(900), (1, 0): e(900), (-1, 0): e(900)}, fill=e(100))),
            ("tie by dy, corners", z({(r, r): e(900), (-r, -r): e(900)}, fill=FEW)),
            ("tie by dy, column", z({(m, 1): e(900), (m, -1): e(900)}, fill=e(100))),
            ("tie by dx", z({(1, 0): e(900), (-1, 0): e(900)}, fill=e(100))),
            ("tie by dx, row", z({(r, -r): e(900), (-r, -r): e(900)}, fill=e(100))),
            ("tie by dx, bottom", z({(1, r): e(900), (-1, r): e(900)}, fill=FEW)),
            ("all equal", z(fill=e(500))), ("all equal negative", z(fill=NEG)), ("all equal, large", z(fill=conv_shift("num", odd=True))),
            # p = 0: the border
            ("side w", z({(-r, 0): e(900)}, fill=e(100))), ("side e", z({(r, 0): e(900)}, fill=e(100))),
            ("side n", z({(0, -r): e(900)}, fill=e(100))), ("side s", z({(0, r): e(900)}, fill=e(100))),
            ("corner nw", z({(-r, -r): e(900)}, fill=e(100))), ("corner ne", z({(r, -r): e(900)}, fill=e(100))),
            ("corner sw", z({(-r, r): e(900)}, fill=e(100))), ("corner se", z({(r, r): e(900)}, fill=e(100))),
            # p = 0 on one axis: a neighbour that is not usable
            ("x- not usable", z({(m, -m): e(900), (m - 1, -m): FEW}, fill=e(100))), ("x+ not usable", z({(-m, m): e(900), (-m + 1, m): FLAT}, fill=e(100))),
            ("y- not usable", z({(m, m): e(900), (m, m - 1): FEW}, fill=e(100))),
            ("y+ not usable", z({(0, 0): e(900), (0, 1): FLAT, (1, 0): e(300)}, fill=e(100))),
            # the denominator is not below 0: a plateau along an axis (the peak is the middle one by the order)
            ("plateau x", z({(-1, 0): e(900), (0, 0): e(900), (1, 0): e(900)}, fill=e(100))),
            ("plateau y", z({(0, -1): e(900), (0, 0): e(900), (0, 1): e(900), (1, 0): e(400)}, fill=e(100))),
            ("plateau both", z({(-1, 0): e(900), (0, 0): e(900), (1, 0): e(900), (0, -1): e(900), (0, 1): e(900)}, fill=e(100))),
            # a proper parabola of designed values, and one of large products
            ("parabola", z({(0, 0): e(900), (1, 0): e(700), (-1, 0): e(500), (0, 1): e(800), (0, -1): e(300)}, fill=e(100))),
            ("parabola, large", z({(0, 0): conv_shift("num", odd=True), (1, 0): conv_shift("da", odd=True), (-1, 0): conv_shift("da")}, fill=e(100)))]
    return out


_CACHE = {}


def case_table(radius):
    """-> (names, sums[ntables, S, S, 6] uint64, reference records, traces, bytes of all records): computed once per radius"""
    if radius not in _CACHE:
        cs = cases(radius)
        sums = np.ascontiguousarray(np.stack([t for _, t in cs]))
        assert int(sums.max()) < (1 << 60)
        ref = [peak(t, radius, MIN_CELLS, CELL) for t in sums]
        sums.setflags(write=False)
        _CACHE[radius] = ([n for n, _ in cs], sums, [r for r, _ in ref], [t for _, t in ref], b"".join(record_bytes(r) for r, _ in ref))
    return _CACHE[radius]

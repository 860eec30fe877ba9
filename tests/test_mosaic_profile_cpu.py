"""The per-ping profile (include/dsss_profile.h), the part that needs no GPU: the preconditions of the designed cases of
tests/mosaic_profile_cases.py on the reference alone, so the GPU cases cannot pass vacuously (samples are compared, pings and sides
with nothing to compare exist, min_count bites, both signs occur), the structure sizes, the host summary against the reference's, and
the coverage of the new header: every function it declares is exported and named in the GPU file's table of driven entries."""
import ctypes as C
import os

import numpy as np

from tests import inflight_cases
from tests import mosaic_canvas_cases as K
from tests import mosaic_profile_cases as P
from tests import mosaic_profile_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _per_frame(orc, name):
    """(records, residual layer, samples) per profiled frame of a case"""
    stats, diff, _ = P.reference(orc, name)
    return [(stats[o:o + N], d, d.size) for (o, N), d in zip(P.pings_of(orc, P.CASES[name]), diff)]


def test_own_without_the_mask_compares_a_third_and_leaves_pings_and_sides_empty(orc):
    p = P.grid(orc, P.CASES["own_um0"])
    assert (p.W, p.H) == (641, 823)
    for f, (st, d, samples) in enumerate(_per_frame(orc, "own_um0")):
        n = st["n"].astype(np.int64)
        share = n.sum() / samples
        print("own/own use_mask 0, frame %d: %.1f %% of %d samples compared, %d of %d pings and %d of %d sides with nothing compared"
              % (f, 100 * share, samples, int((n.sum(1) == 0).sum()), len(st), int((n == 0).sum()), 2 * len(st)))
        assert share >= 0.30
        assert int((n.sum(1) > 0).sum()) >= 100
        assert int((n == 0).sum()) >= 100
        assert (d != PR.NONE).sum() == n.sum()


def test_own_under_the_mask_still_compares(orc):
    for f, (st, d, samples) in enumerate(_per_frame(orc, "own_um1")):
        n, b = int(st["n"].astype(np.int64).sum()), int(st["binned"].astype(np.int64).sum())
        print("own/own use_mask 1, frame %d: %d of %d binned samples compared (%.1f %%)" % (f, n, b, 100.0 * n / b))
        assert n >= 1000 and b < samples


def test_t1_leaves_most_pings_of_frame_0_empty_and_the_nan_rows_among_them(orc):
    st, d, _ = _per_frame(orc, "t1_um0")[0]
    n = st["n"].astype(np.int64).sum(1)
    print("t1/own use_mask 0, frame 0: %d of %d pings with nothing compared" % (int((n == 0).sum()), len(st)))
    assert np.isnan(K.rows_of(orc, 0, "t1")[500:503]).all()
    assert (n[500:503] == 0).all() and (st["binned"][500:503] == 0).all() and (d[500:503] == PR.NONE).all()
    assert int((n == 0).sum()) >= 300 and int((n > 0).sum()) >= 100


def test_min_count_bites_and_the_sums_fit(orc):
    one, three = P.reference(orc, "three")[2], P.reference(orc, "three_min3")[2]
    print("three frames, use_mask 0: %d samples compared at min_count 1, %d at 3" % (one["n"], three["n"]))
    assert 0 < three["n"] < one["n"] and three["binned"] == one["binned"]
    two = P.reference(orc, "two_min3")[2]                                          # point samples at this cell: no cell holds three of the other leg
    assert two["n"] == 0 and two["binned"] == P.reference(orc, "own_um0")[2]["binned"]
    top = 0
    for name in P.CASES:
        st = P.reference(orc, name)[0]
        top = max(top, int(st["ssd"].max()))
        assert (st["n"] <= st["binned"]).all()
    print("the largest per-side ssd over all cases: %d" % top)
    assert top < 1 << 32
    sd = P.reference(orc, "own_um0")[0]["sd"]
    assert (sd > 0).any() and (sd < 0).any()


def test_every_case_compares_something_but_the_frame_alone(orc):
    for name, case in P.CASES.items():
        stats, diff, info = P.reference(orc, name)
        assert info["pings"] == len(stats) == sum(N for _, N in P.pings_of(orc, case)) and len(diff) == len(P.pings_of(orc, case))
        if name in ("alone", "two_min3"):
            assert info["binned"] > 0 and not stats["n"].any() and all((d == PR.NONE).all() for d in diff)
            assert info["rms"] == 0.0
        else:
            print("%s: %d binned, %d compared, rms %.3f" % (name, info["binned"], info["n"], info["rms"]))
            assert info["n"] > 0 and info["rms"] > 0.0
    # the middle third drops samples the full grid bins, and the tables change the levels that are compared
    assert 0 < P.reference(orc, "mid")[2]["binned"] < P.reference(orc, "own_um0")[2]["binned"]
    assert P.reference(orc, "gain_col")[0].tobytes() != P.reference(orc, "gain_two")[0].tobytes()
    # a subset and a reversed list are the same records per frame
    three, sub, rev = P.reference(orc, "three"), P.reference(orc, "subset"), P.reference(orc, "reversed")
    spans = P.pings_of(orc, P.CASES["three"])
    assert sub[0].tobytes() == three[0][spans[1][0]:spans[1][0] + spans[1][1]].tobytes()
    assert rev[0].tobytes() == b"".join(three[0][o:o + N].tobytes() for o, N in reversed(spans))
    assert all((a == b).all() for a, b in zip(rev[1], reversed(three[1])))


def test_structures_and_defaults():
    from diasss_amd import capi
    assert (C.sizeof(capi.PingStat), C.sizeof(capi.ProfileParams), C.sizeof(capi.ProfileInfo)) == (40, 8, 56)
    assert capi.PING_DTYPE.itemsize == PR.REC.itemsize == 40
    assert [(n, capi.PING_DTYPE.fields[n][1]) for n in capi.PING_DTYPE.names] == [(n, PR.REC.fields[n][1]) for n in PR.REC.names]
    assert capi.profile_params_default().min_count == 1
    capi.lib().dsss_profile_params_default(None)                                   # NULL: nothing happens
    assert capi.PROFILE_NONE == PR.NONE


def test_every_entry_of_the_header_is_exported_and_driven():
    from diasss_amd import capi
    from tests import test_gpu_mosaic_profile as T
    with open(os.path.join(ROOT, "include", "dsss_profile.h")) as f:
        text = f.read()
    assert '#include "dsss.h"' in text and '#include "dsss_canvas.h"' in text
    declared = inflight_cases.declared_entries(text)
    assert len(declared) == 4 and all(n.startswith("dsss_profile_") for n in declared), declared
    L = capi.lib()
    for n in declared:
        assert hasattr(L, n), "%s is declared and not exported" % n
    assert sorted(T.DRIVEN) == declared, "declared and not driven: %s; driven and not declared: %s" % (
        sorted(set(declared) - set(T.DRIVEN)), sorted(set(T.DRIVEN) - set(declared)))


def test_summary_equals_the_reference(orc):
    from diasss_amd import capi
    for name in P.CASES:
        stats, _, want = P.reference(orc, name)
        got = capi.profile_summary(stats)
        assert {k: getattr(got, k) for k in PR.INFO_FIELDS} == want, name          # rms with ==: one division and one square root
    empty = capi.profile_summary(np.zeros(0, PR.REC))
    assert {k: getattr(empty, k) for k in PR.INFO_FIELDS} == dict(pings=0, binned=0, n=0, sad=0, ssd=0, sd=0, rms=0.0)
    L = capi.lib()
    one = np.zeros(1, PR.REC)
    assert L.dsss_profile_summary(capi._ptr(one), 1, None) == -2 and L.dsss_profile_summary(None, 1, C.byref(capi.ProfileInfo())) == -2
    assert L.dsss_profile_summary(capi._ptr(one), -1, C.byref(capi.ProfileInfo())) == -2

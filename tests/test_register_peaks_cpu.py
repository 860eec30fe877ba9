"""The preconditions of tests/test_gpu_register_peaks.py, off the device: on the case table of tests/register_peaks_ref.py the host
entry dsss_mosaic_register_peak equals the reference byte for byte, every branch of the rule that the table is meant to reach is taken
by at least three tables (read from the reference's own trace), and the 128-bit rounding cases bite: some table's zncc would be
another number under a truncating conversion."""
import ctypes as C
import numpy as np
import pytest

from tests import mosaic_register_ref as R
from tests import register_peaks_ref as P

BRANCHES = ("none_usable", "unusable_n", "unusable_da", "one_usable", "tie_d2", "tie_dy", "tie_dx", "all_equal", "negative_peak",
            "border_side", "border_corner", "border_w", "border_e", "border_n", "border_s", "border_nw", "border_ne", "border_sw", "border_se",
            "neighbour_unusable_one_axis", "plateau", "parabola", "conv_tie_even", "conv_tie_odd", "conv_sticky")


def _host_bytes(t, radius):
    from diasss_amd import capi
    rec = capi.mosaic_register_peak(t, radius, P.MIN_CELLS, P.CELL)
    return C.string_at(C.addressof(rec), C.sizeof(rec))


@pytest.mark.parametrize("radius", P.RADII)
def test_host_entry_equals_the_reference(radius):
    names, sums, ref, traces, blob = P.case_table(radius)
    assert len(blob) == P.REC_BYTES * len(names)
    for k, name in enumerate(names):
        got = _host_bytes(sums[k], radius)
        assert got == blob[k * P.REC_BYTES:(k + 1) * P.REC_BYTES], "radius %d, table %r: library %s, reference %s" % (
            radius, name, np.frombuffer(got, _dtype())[0], ref[k])


def _dtype():
    from diasss_amd import capi
    return capi.REG_DTYPE


def test_the_reference_agrees_with_the_existing_one():
    """two references written apart: tests/mosaic_register_ref.py has no trace and no byte form"""
    for radius in P.RADII:
        names, sums, ref, traces, blob = P.case_table(radius)
        for k in range(len(names)):
            assert R.peak(sums[k].astype(object), radius, P.MIN_CELLS, P.CELL) == ref[k], (radius, names[k])


def test_every_branch_is_taken_by_three_tables():
    count = {b: 0 for b in BRANCHES}
    for radius in P.RADII:
        names, sums, ref, traces, blob = P.case_table(radius)
        for tr in traces:
            for b in tr:
                if b in count:
                    count[b] += 1
    print(count)
    short = {b: n for b, n in count.items() if n < 3}
    assert not short, "branches taken by fewer than three tables: %s" % short
    # the real tables are not all of one kind: some have a peak inside the square with a proper parabola, some lie on the border
    for radius in P.RADII[1:]:
        names, sums, ref, traces, blob = P.case_table(radius)
        real = [ref[k] for k, n in enumerate(names) if n.startswith("real")]
        assert len(real) == 4 and any(r["zncc"] > 0.3 for r in real) and all(r["n"] > P.MIN_CELLS for r in real)


def test_truncating_the_conversion_would_change_a_score():
    """... and so would a cut to 64 bits without the sticky bit: the two wrong conversions of the reference module"""
    for how, must in (("53", ("tie odd", "sticky")), ("64", ("sticky",))):
        changed = []
        for radius in P.RADII:
            names, sums, ref, traces, blob = P.case_table(radius)
            for k, name in enumerate(names):
                cut, _ = P.peak(sums[k], radius, P.MIN_CELLS, P.CELL, truncate=how)
                if cut["zncc"] != ref[k]["zncc"]:
                    changed.append((radius, name, ref[k]["zncc"].hex(), cut["zncc"].hex()))
        print(how, changed[:8])
        assert len(changed) >= 3
        for word in must:
            assert any(word in n for _, n, _, _ in changed), (how, word)

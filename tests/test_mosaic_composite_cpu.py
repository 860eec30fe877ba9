"""The composite mosaic off the device: dsss_mosaic_comp_rank and dsss_mosaic_fill_host (pure host arithmetic of libdsss.so) against
tests/mosaic_composite_ref.py and against values worked out by hand, every argument error of both, and the preconditions of the GPU
cases on the reference alone."""
import numpy as np
import pytest

from tests import mosaic_composite_cases as K
from tests import mosaic_composite_ref as CR

E_ARG = -2


# ---------------------------------------------------------------- rank
def test_reference_rank_by_hand():
    # M = 6: half = 3; port columns 0, 1, 2 have idx 2, 2, 1 (0 and 1 share the last bin), starboard 3, 4, 5 have 0, 1, 2
    assert [CR.ground_index(6, c) for c in range(6)] == [2, 2, 1, 0, 1, 2]
    assert [CR.rank(CR.NEAR, 6, c) for c in range(6)] == [2, 2, 1, 0, 1, 2]
    assert [CR.rank(CR.FAR, 6, c) for c in range(6)] == [0, 0, 1, 2, 1, 0]
    assert [CR.rank(CR.MID, 6, c) for c in range(6)] == [2, 2, 0, 2, 0, 2]
    assert [CR.rank(CR.FIRST, 6, c) for c in range(6)] == [0] * 6
    for M in (4, 6, 86, 400, 65534):
        for mode in CR.MODES:
            assert CR.rank(mode, M, 0) == CR.rank(mode, M, 1)                   # the port columns 0 and 1 share idx and hence q
            q = CR.ranks(mode, M) if M < 1000 else np.array([CR.rank(mode, M, c) for c in (0, 1, M // 2 - 1, M // 2, M - 1)])
            assert q.min() >= 0 and q.max() <= 32766


@pytest.mark.parametrize("M", [4, 6, 86, 400, 65534])
def test_library_rank_matches_reference(M):
    from diasss_amd import capi
    L = capi.lib()
    q = capi.C.c_int32(-1)
    for mode in CR.MODES:
        ref = CR.ranks(mode, M)
        dev = np.empty(M, np.int64)
        for col in range(M):
            assert L.dsss_mosaic_comp_rank(mode, M, col, capi.C.byref(q)) == 0
            dev[col] = q.value
        assert (dev == ref).all(), "mode %d, M %d: columns %s differ" % (mode, M, np.nonzero(dev != ref)[0][:8].tolist())
    assert capi.mosaic_comp_rank("mid", M, M - 1) == CR.rank(CR.MID, M, M - 1)      # (by name through the binding)


def test_rank_argument_errors():
    from diasss_amd import capi
    L = capi.lib()
    q = capi.C.c_int32(77)
    ok = lambda mode=0, M=400, col=5, out=capi.C.byref(q): L.dsss_mosaic_comp_rank(mode, M, col, out)      # noqa: E731
    assert ok() == 0
    assert ok(out=None) == E_ARG
    assert ok(mode=-1) == E_ARG and ok(mode=4) == E_ARG and ok(mode=3) == 0
    assert ok(M=2) == E_ARG and ok(M=0) == E_ARG and ok(M=401) == E_ARG and ok(M=65536, col=0) == E_ARG and ok(M=4, col=3) == 0
    assert ok(col=-1) == E_ARG and ok(col=400) == E_ARG and ok(col=399) == 0
    with pytest.raises(capi.DsssError) as e:
        capi.mosaic_comp_rank(0, 400, 400)
    assert e.value.code == E_ARG
    p = capi.comp_params_default()
    assert (p.mode, p.fill_radius) == (capi.COMP_NEAR, 0)


# ---------------------------------------------------------------- fill
def _both(valid, R):
    """the library's donor and fill layers, after they were found equal to the reference's"""
    from diasss_amd import capi
    valid = np.asarray(valid, np.uint8)
    donor, fill = capi.mosaic_fill_host(valid, R)
    rd, rf = CR.fill(valid, R)
    assert donor.dtype == np.int32 and fill.dtype == np.uint8
    assert (donor == rd).all(), "donors differ at %s" % np.argwhere(donor != rd)[:5].tolist()
    assert (fill == rf).all(), "fill differs at %s" % np.argwhere(fill != rf)[:5].tolist()
    return donor, fill


def test_fill_single_hole():
    v = np.ones((5, 6), np.uint8); v[2, 3] = 0
    donor, fill = _both(v, 1)
    assert fill[2, 3] == 1 and donor[2, 3] == 1 * 6 + 3                           # up (dy = -1, dx = 0) before left (dy = 0, dx = -1)
    assert (np.delete(fill.ravel(), 2 * 6 + 3) == 0).all() and (np.delete(donor.ravel(), 15) == np.delete(np.arange(30), 15)).all()
    donor, fill = _both(v, 0)
    assert fill[2, 3] == 255 and donor[2, 3] == -1                                # R = 0: no fill


def test_fill_strip_of_three():
    """a strip three cells wide over the whole height: at R = 2 its outer cells have nothing within 2 on their far side and stay
    empty -- the strip is not closed -- while the middle one, two cells from either edge, is enclosed by the definition; at R = 3
    every cell of it is filled"""
    v = np.ones((4, 9), np.uint8); v[:, 3:6] = 0
    donor, fill = _both(v, 1)
    assert (fill[:, 3:6] == 255).all() and (donor[:, 3:6] == -1).all()
    donor, fill = _both(v, 2)
    assert fill[1, 3:6].tolist() == [255, 4, 255] and donor[1, 3:6].tolist() == [-1, 9 + 2, -1]
    donor, fill = _both(v, 3)
    assert fill[1, 3:6].tolist() == [1, 4, 1] and donor[1, 3:6].tolist() == [9 + 2, 9 + 2, 9 + 6]      # the middle: dx = -2 before dx = +2


def test_fill_border_hole_stays_empty():
    v = np.ones((5, 5), np.uint8); v[0:3, 0] = 0; v[0, 3] = 0; v[4, 4] = 0        # (0, 0), (0, 1), (0, 2): samples below and to the right only
    donor, fill = _both(v, 4)
    assert (fill[0:3, 0] == 255).all() and (donor[0:3, 0] == -1).all()            # left of and above them is outside the grid: not in V0
    assert fill[0, 3] == 1 and donor[0, 3] == 2                                   # on the border, but enclosed along x
    assert fill[4, 4] == 255


def test_fill_tie_order():
    # an L-shaped hole two cells thick: (x 1..2, y 1..4) and (x 1..4, y 3..4) of a 7 x 7 layer.  The cell (2, 3) has no sample on
    # its row or column within 2; within 3 it is enclosed along x ((0, 3) and (5, 3)) and its nearest donor is diagonal: (3, 2)
    v = np.ones((7, 7), np.uint8); v[1:5, 1:3] = 0; v[3:5, 1:5] = 0
    donor, fill = _both(v, 2)
    assert fill[3, 2] == 255
    donor, fill = _both(v, 3)
    assert fill[3, 2] == 2 and donor[3, 2] == 2 * 7 + 3
    # a plus-shaped hole: the centre's four diagonal neighbours tie at d2 = 2, and (dy, dx) = (-1, -1) is the first of them
    v = np.ones((5, 5), np.uint8); v[2, 1:4] = 0; v[1:4, 2] = 0
    donor, fill = _both(v, 2)
    assert fill[2, 2] == 2 and donor[2, 2] == 1 * 5 + 1
    # dy before dx: candidates (dy, dx) = (-1, 1) and (1, -1) alone at d2 = 2 -> the one with dy = -1
    v = np.zeros((5, 5), np.uint8); v[1, 3] = 1; v[3, 1] = 1; v[2, 0] = 1; v[2, 4] = 1
    donor, fill = _both(v, 2)
    assert fill[2, 2] == 2 and donor[2, 2] == 1 * 5 + 3


def test_fill_lines():
    row = np.array([[1, 0, 1, 0, 0, 1, 0]], np.uint8)                             # 1 x 7
    for v in (row, row.T.copy()):                                                 # and 7 x 1
        donor, fill = _both(v, 1)
        assert fill.ravel().tolist() == [0, 1, 0, 255, 255, 0, 255] and donor.ravel().tolist() == [0, 0, 2, -1, -1, 5, -1]
        donor, fill = _both(v, 2)
        assert fill.ravel().tolist() == [0, 1, 0, 1, 1, 0, 255] and donor.ravel().tolist() == [0, 0, 2, 2, 5, 5, -1]


@pytest.mark.parametrize("R", [0, 1, 2, 3, 4])
def test_fill_random_layer(R):
    rng = np.random.default_rng(70 * 45)
    v = (rng.random((45, 70)) < 0.35).astype(np.uint8)
    v[10:20, 30:44] = 0; v[:, 60:] *= (rng.random((45, 10)) < 0.2)               # a hole larger than any radius, a sparse edge
    donor, fill = _both(v * 200, R)                                               # (any value != 0 is valid)
    if R:
        assert ((fill > 0) & (fill < 255)).sum() > 100 and (fill == 255).sum() > 100
        assert fill[fill < 255].max() <= R * R                                    # an enclosed cell has a donor on one of its axes within R
    if R >= 2:
        assert np.isin(fill, [2, 5, 8, 10, 13]).any()                             # and donors off the axes are taken where they are nearer


def test_fill_argument_errors():
    from diasss_amd import capi
    L = capi.lib()
    P = capi._ptr
    v = np.ones((3, 4), np.uint8); d = np.zeros((3, 4), np.int32); f = np.zeros((3, 4), np.uint8)
    rc = lambda valid=v, W=4, H=3, R=1, donor=d, fill=f: L.dsss_mosaic_fill_host(P(valid), W, H, R, P(donor), P(fill))      # noqa: E731
    assert rc() == 0
    assert rc(valid=None) == E_ARG and rc(donor=None) == E_ARG and rc(fill=None) == E_ARG
    assert rc(W=0) == E_ARG and rc(H=0) == E_ARG and rc(W=-4) == E_ARG
    assert rc(W=1 << 15, H=(1 << 13) + 1) == E_ARG                                # W H > 2^28 (refused before anything is read)
    assert rc(R=-1) == E_ARG and rc(R=5) == E_ARG and rc(R=4) == 0 and rc(R=0) == 0
    with pytest.raises(capi.DsssError) as e:
        capi.mosaic_fill_host(v, 5)
    assert e.value.code == E_ARG


# ---------------------------------------------------------------- the preconditions of the GPU cases, on the reference alone
def test_precondition_holes(orc):
    """at cell 0.05 without a mask the two legs leave holes, some enclosed and some not"""
    lay, (direct, filled, empty), _ = K.reference(orc, 0.05, 0, CR.NEAR, R=1)
    print("cell 0.05: %d direct, %d filled at R = 1, %d left empty" % (direct, filled, empty))
    assert direct > 0 and filled > 0 and empty > 0
    assert direct + filled + empty == lay["fill"].size


def test_precondition_radii_differ(orc):
    """with the pings of BAD_PINGS dropped (cell 0.05, no mask: the grid of 641 x 823 cells the GPU case runs on) the number of filled
    cells grows strictly from R = 1 to 2 to 4"""
    n = [K.reference(orc, 0.05, 0, CR.NEAR, R=R, bad=True)[1][1] for R in (1, 2, 4)]
    p = K.full_grid(K.legs(orc), 0.05, 0)
    print("grid %d x %d, filled cells at R = 1, 2, 4: %s" % (p.W, p.H, n))
    assert 0 < n[0] < n[1] < n[2]
    assert n[0] > K.reference(orc, 0.05, 0, CR.NEAR, R=1)[1][1]                  # the dropped pings add holes of their own


def test_precondition_ties_and_frames(orc):
    """at cell 0.13 a fraction of the cells has a runner-up with the winner's q, so g decides there; and in the overlap cells are won
    by each frame"""
    for mode in CR.MODES:
        lay, info, st = K.reference(orc, 0.13, 0, mode)
        won = [int((lay["src_frame"] == f).sum()) for f in (0, 1)]
        print("mode %d: %d cells contended, %d decided by g, %d by col; frame 0 wins %d cells, frame 1 %d; fullest cell %d" % (
            mode, st["contended"], st["ties_q"], st["ties_qg"], won[0], won[1], st["fullest"]))
        assert st["ties_q"] > 0 and st["contended"] > st["ties_q"] * (mode != CR.FIRST)
        assert min(won) > 1000
    # both frames win cells that both frames see: the winner is not decided by coverage alone
    L = K.legs(orc)
    p = K.full_grid(L, 0.13, 0)
    alone = [CR.winners(K.frames(L)[k:k + 1], p, 0, CR.NEAR)[0]["valid"] for k in (0, 1)]
    both = alone[0] & alone[1]
    lay = K.reference(orc, 0.13, 0, CR.NEAR)[0]
    assert both.sum() > 1000 and min(int(((lay["src_frame"] == f) & both).sum()) for f in (0, 1)) > 100
    assert K.reference(orc, 1.7, 0, CR.NEAR)[2]["fullest"] > 1000               # thousands of samples contend for a cell at 1.7

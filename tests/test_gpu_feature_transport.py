"""GPU: what moves between ranks, held bit for bit to records built and parsed in numpy (tests/feature_transport_ref.py).

One context plays rank r of W; the test plays its peers: the callback of the host transport (dsss_comm_init_callback) receives the
(world, slice) byte array with the own row filled in, keeps a copy of that row and writes into every other row the records the test
built for those ranks' frames.  Both passes of ag_copy_kernel are judged on their own: the PACK pass by parsing the own row, the UNPACK
pass by reading every frame back, and the device tables behind them (nkp_dev, rows_dev, bbox_dev, geo, desc, desc128) by running the
matcher over own and gathered frames against the oracle.  Nothing expected comes from the library: keypoints, descriptors, geo
samples and boxes are designed (feature_transport_ref.design_frames) or the oracle's.  Every assertion is equality of bytes or integers.

Also: the per-frame entries dsss_features_pack / _unpack / _pack_bytes with host and device buffers, and the two refusals of
dsss_features_allgather -- a peer's header with a count outside [0, K] or another N x M leaves every frame, on the device and on the
host, as it was; in SIFT mode an owned frame without SIFT rows is refused before anything is sent."""
import ctypes

import numpy as np
import pytest

from tests import feature_transport_ref as R

pytestmark = pytest.mark.gpu

E_ARG, E_STATE, E_CAPACITY = -2, -4, -5          # include/dsss.h
MAXF = 8
SENTINEL = MAXF - 1                              # a frame id >= F of every case


def _context(small, sift=False):
    """(context of MAXF frames, its per-frame capacity K read off pack_bytes()): nfeatures = 100, nlevels = 2 gives K = 192, the whole
    copy of a record is one pass of ag_copy_kernel's grid-stride loop (8 x 256 threads x 16 bytes); the default K = 2112 takes several"""
    from diasss_amd import capi
    c = capi.Context(max_frames=MAXF)
    mp, op, mt, pg = c.default_params()
    if small:
        op.nfeatures, op.nlevels = 100, 2
    if sift:
        op.descriptor = capi.DESC_SIFT128; mt.use_l2 = 2
    c.set_params(orb=op, match=mt)
    K = R.capacity(c.pack_bytes(), sift)
    assert K == (192 if small else 2112) and (sift or (K * R.ROW_BYTES // 16 <= 8 * 256) == small)
    return c, K


def _set_geometry(c, f, fr):
    c.frame_set(f, None, fr["N"], fr["M"], fr["pose"], fr["alt"], fr["gr"])


def _set(c, f, fr, sift):
    _set_geometry(c, f, fr)
    c.features_set(f, fr["N"], fr["M"], fr["kps"], fr["desc"], fr["geo"], fr["bb"])
    if sift:
        c.features_set_sift(f, fr["d128"].astype(np.float32))


def _read(c, f, sift):
    kps, desc, geo = c.features_get(f)
    out = [kps.tobytes(), desc.tobytes(), geo.tobytes(), c.frame_bbox(f).tobytes()]
    if sift:
        d = c.features_get_sift(f)
        assert d.shape == (len(kps), 128)
        out.append(d.astype(np.uint8).tobytes())
    return out


def _designed(fr, sift):
    return [fr["kps"].tobytes(), fr["desc"].tobytes(), fr["geo"].tobytes(), fr["bb"].tobytes()] + ([fr["d128"].tobytes()] if sift else [])


def _assert_record(buf, K, sift, fr):
    """header, box and the first n rows of every section of a record the library packed"""
    p = R.parse_record(buf, K, sift)
    n = len(fr["kps"])
    assert (p["n"], p["N"], p["M"], p["pad"]) == (n, fr["N"], fr["M"], 0)
    assert p["bbox"].tobytes() == fr["bb"].tobytes()
    assert p["kps"][:n].tobytes() == fr["kps"].tobytes()
    assert p["desc"][:n].tobytes() == fr["desc"].tobytes()
    assert p["geo"][:n].tobytes() == fr["geo"].tobytes()
    if sift:
        assert p["d128"][:n].tobytes() == fr["d128"].tobytes()


class _Peers:
    """the transport of one gather: hands the library `rows` (W, slice) for every rank but r and keeps what r itself sent"""

    def __init__(self, c, r, W, rows, device=False):
        self.r, self.W, self.rows, self.calls, self.own = r, W, rows, 0, None
        if not device:
            c.comm_init_callback(r, W, self.host)
            return
        import torch
        from diasss_amd import capi
        self.hip = capi._HIP                            # the process-wide HIP runtime the library runs on
        self.hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
        self.dev = torch.from_numpy(rows).to("cuda:0")
        self.pinned = torch.zeros(rows.shape[1], dtype=torch.uint8).pin_memory()
        torch.cuda.synchronize()
        c.comm_init_device_callback(r, W, self.device)

    def host(self, op, arr):
        assert op == 1 and arr.shape == self.rows.shape and arr.dtype == np.uint8
        self.calls += 1
        self.own = arr[self.r].copy()
        for q in range(self.W):
            if q != self.r:
                arr[q] = self.rows[q]

    def device(self, op, ptr, n, stream):
        """the peers' rows copied into the device buffer on the library's stream (as tools/emulate_ranks.py:Replay), the own row copied out"""
        assert op == 1 and n == self.rows.shape[1] and ptr
        self.calls += 1
        assert self.hip.hipMemcpyAsync(self.pinned.data_ptr(), ptr + self.r * n, n, 2, stream) == 0          # hipMemcpyDeviceToHost
        for q in range(self.W):
            if q != self.r:
                assert self.hip.hipMemcpyAsync(ptr + q * n, self.dev[q].data_ptr(), n, 3, stream) == 0       # hipMemcpyDeviceToDevice
        self.own = self.pinned.numpy()                  # (complete once the gather has synchronised its stream)


def _gather(c, orc, F, W, r, frames, K, sift, fill, device=False):
    """One gather of rank r of W over `frames`, with the assertions of both passes.  Own frames are set with the designed features,
    the peers' with their geometry alone (what the pipeline gives them); SENTINEL is a frame outside the gather."""
    nb = c.pack_bytes()
    assert nb == R.record_bytes(K, sift)
    lo, hi = R.block(F, r, W)
    for f in range(F):
        (_set(c, f, frames[f], sift) if lo <= f < hi else _set_geometry(c, f, frames[f]))
    guard = R.design_frames(orc, (7, 3), 1, K, sift)[6]
    _set(c, SENTINEL, guard, sift)
    own_before = {f: _read(c, f, sift) for f in range(lo, hi)}
    peers = _Peers(c, r, W, R.gathered(frames, F, W, K, sift, fill), device)
    assert peers.rows.shape == (W, R.slice_bytes(F, W, nb))
    c.features_allgather(F)
    assert peers.calls == 1
    # pack pass: the own row, record by record
    for f in range(lo, hi):
        _assert_record(R.record_at(peers.own, F, W, f, nb), K, sift, frames[f])
    # unpack pass: every frame reads back as built, the own ones as before, the frame outside the gather untouched
    for f in range(F):
        assert _read(c, f, sift) == _designed(frames[f], sift), "frame %d of %d, rank %d of %d" % (f, F, r, W)
    for f in range(lo, hi):
        assert _read(c, f, sift) == own_before[f]
    assert _read(c, SENTINEL, sift) == _designed(guard, sift)
    return peers


def _match(c, orc, pairs, frames, sift):
    """the matcher over own and gathered frames against the oracle: the device tables hold the records.  -> rows per pair, the results' bytes"""
    from tests.test_gpu_matcher import _check_pair
    po = None
    if sift:
        po = orc.match_params(); po.use_l2 = 2
    view = R.oracle_view(frames, sift)
    c.match_pairs([a for a, b in pairs], [b for a, b in pairs])
    n = [_check_pair(c, orc, p, a, b, view, po) for p, (a, b) in enumerate(pairs)]
    keep = [x for p in range(len(pairs)) for x in [c.match_rows(p).tobytes(), c.match_kp7(p).tobytes()] + [np.asarray(v).tobytes() for d in (0, 1) for v in c.match_dir(p, d)]]
    return n, keep


def _rank_through_two_rounds(orc, case, r, small, sift):
    F, W = case
    c, K = _context(small, sift)
    try:
        for rnd, fill in ((0, 0x5A), (1, 0xC3)):                    # the second gather reuses the staging buffer: other counts, another fill
            frames = R.design_frames(orc, case, rnd, K, sift)
            _gather(c, orc, F, W, r, frames, K, sift, fill)
            n, _ = _match(c, orc, R.MATCH_PAIRS[case][rnd], frames, sift)
            assert n[0] > 5, n
        W2 = W - 1                                                  # the communicator re-initialised with another world: other blocks, another slice
        frames = R.design_frames(orc, case, 0, K, sift)
        _gather(c, orc, F, W2, min(r, W2 - 1), frames, K, sift, 0x3C)
        n, _ = _match(c, orc, R.MATCH_PAIRS[case][0], frames, sift)
        assert n[0] > 5, n
    finally:
        c.close()


@pytest.mark.parametrize("small", [True, False], ids=["K192", "K2112"])
@pytest.mark.parametrize("case", R.SPLITS, ids=lambda c: "F%dW%d" % c)
def test_gather_as_every_rank(orc, case, small):
    """every rank r of the case: two gathers with other counts (0, 1, 63, 64, 65, K among them), a third after the communicator was
    re-initialised with W - 1 ranks; (3, 4): rank 0 owns nothing and packs nothing"""
    for r in range(case[1]):
        _rank_through_two_rounds(orc, case, r, small, sift=False)


def test_gather_in_sift_mode(orc):
    """DSSS_DESC_SIFT128 with use_l2 = 2: the record carries the desc128 section and the matcher reads it"""
    for r in range(4):
        _rank_through_two_rounds(orc, (5, 4), r, small=True, sift=True)


def test_device_transport_equals_host_transport(orc):
    """dsss_comm_init_device_callback: the callback copies the peers' rows into the device buffer on the given stream; every frame and
    every matcher result equals the host transport's bit for bit"""
    case, r = (7, 3), 1
    got = []
    for device in (False, True):
        c, K = _context(small=True)
        try:
            frames = R.design_frames(orc, case, 0, K)
            peers = _gather(c, orc, *case, r, frames, K, False, 0x5A, device=device)
            n, keep = _match(c, orc, R.MATCH_PAIRS[case][0], frames, False)
            lo, hi = R.block(case[0], r, case[1])
            own = [R.parse_record(R.record_at(peers.own, *case, f, c.pack_bytes()), K, False) for f in range(lo, hi)]
            got.append(([_read(c, f, False) for f in range(case[0])], keep,
                        [(p["n"], p["N"], p["M"], p["pad"], p["bbox"].tobytes(), p["kps"][:p["n"]].tobytes(), p["desc"][:p["n"]].tobytes(), p["geo"][:p["n"]].tobytes()) for p in own]))
        finally:
            c.close()
    assert got[0] == got[1]


# ---------------------------------------------------------------- the per-frame entries
def _refused(code, call):
    from diasss_amd import capi
    with pytest.raises(capi.DsssError) as ei:
        call()
    assert ei.value.code == code, ei.value


@pytest.mark.parametrize("sift", [False, True], ids=["orb", "sift"])
def test_pack_and_unpack_one_frame(orc, sift):
    """dsss_features_pack into a host (numpy) and a device (CUDA tensor) buffer gives the builder's header, box and first n rows per
    section; dsss_features_unpack of a built record, from host and from device memory, into another slot reads back equal; the
    refusals leave the slot as it was"""
    import torch
    c, K = _context(small=True, sift=sift)
    try:
        nb = c.pack_bytes()
        frames = R.design_frames(orc, (7, 3), 0, K, sift)           # counts K, 1, 63, 64, 65, 0, 150
        for f, fr in enumerate(frames):
            _set(c, f, fr, sift)
        for f, fr in enumerate(frames):
            host = np.full(nb, 0x3C, np.uint8)
            c.features_pack(f, host)
            _assert_record(host, K, sift, fr)
            dev = torch.full((nb,), 0x3C, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            c.features_pack(f, dev)
            _assert_record(dev.cpu().numpy(), K, sift, fr)
        slot = SENTINEL                                             # no geometry of its own: takes the record's N x M
        for f, fr in enumerate(frames):                             # (counts go down and up from one record to the next)
            rec = R.frame_record(fr, K, sift, fill=0xC3)
            c.features_unpack(slot, rec)
            assert _read(c, slot, sift) == _designed(fr, sift)
            c.features_unpack(slot, R.frame_record(frames[(f + 3) % 7], K, sift, fill=0x5A))
            dev = torch.from_numpy(rec).to("cuda:0")
            torch.cuda.synchronize()
            c.features_unpack(slot, dev)
            assert _read(c, slot, sift) == _designed(fr, sift)
        # refusals
        before = _read(c, slot, sift)
        _refused(E_CAPACITY, lambda: c.features_unpack(slot, R.frame_record(frames[2], K, sift, n=K + 1)))
        _refused(E_CAPACITY, lambda: c.features_unpack(slot, R.frame_record(frames[2], K, sift, n=-1)))
        assert _read(c, slot, sift) == before
        before3 = _read(c, 3, sift)                                 # frame 3 has geometry: 700 x 480
        _refused(E_ARG, lambda: c.features_unpack(3, R.frame_record(frames[2], K, sift, N=699)))
        _refused(E_ARG, lambda: c.features_unpack(3, R.frame_record(frames[2], K, sift, M=482)))
        assert _read(c, 3, sift) == before3
        if sift:                                                    # a frame whose features were set without the 128-byte rows
            fr = frames[4]
            c.features_set(4, fr["N"], fr["M"], fr["kps"], fr["desc"], fr["geo"], fr["bb"])
            before4 = _read(c, 4, False)
            host = np.full(nb, 0x3C, np.uint8)
            _refused(E_STATE, lambda: c.features_pack(4, host))
            c.sync()
            assert (host == 0x3C).all()                             # nothing was queued into the caller's buffer
            assert _read(c, 4, False) == before4
            _refused(E_STATE, lambda: c.features_get_sift(4))
    finally:
        c.close()


# ---------------------------------------------------------------- refusals of the gather
@pytest.mark.parametrize("lie,code", [(dict(n="K+1"), E_CAPACITY), (dict(n=-1), E_CAPACITY), (dict(N=699), E_ARG)], ids=["count-K+1", "count-minus-1", "other-N"])
def test_refused_gather_leaves_every_frame_as_it_was(orc, lie, code):
    """After a good gather, a peer's record with a lying header arrives for the MIDDLE frame of its block (frame 5 of rank 2's 4, 5, 6), among
    records that otherwise differ from what the context holds.  The headers are judged on the device before the unpack pass writes
    (ag_check_kernel), so: the right error code, every frame reads as before, the matcher over own and gathered frames gives the
    bytes it gave before, and a good gather afterwards succeeds."""
    case, r = (7, 3), 0
    F, W = case
    c, K = _context(small=True)
    try:
        frames0 = R.design_frames(orc, case, 0, K)
        _gather(c, orc, F, W, r, frames0, K, False, 0x5A)
        _, keep = _match(c, orc, R.MATCH_PAIRS[case][0], frames0, False)
        before = [_read(c, f, False) for f in range(F)] + [_read(c, SENTINEL, False)]
        lie = {k: (K + 1 if v == "K+1" else v) for k, v in lie.items()}
        frames1 = R.design_frames(orc, case, 1, K)
        peers = _Peers(c, r, W, R.gathered(frames1, F, W, K, False, 0xC3, lie=(5, lie)))
        _refused(code, lambda: c.features_allgather(F))
        assert peers.calls == 1
        assert [_read(c, f, False) for f in range(F)] + [_read(c, SENTINEL, False)] == before
        _, again = _match(c, orc, R.MATCH_PAIRS[case][0], frames0, False)
        assert again == keep
        _gather(c, orc, F, W, r, frames1, K, False, 0x3C)
        n, _ = _match(c, orc, R.MATCH_PAIRS[case][1], frames1, False)
        assert n[0] > 5
    finally:
        c.close()


def test_sift_gather_refuses_an_own_frame_without_rows(orc):
    """one frame per rank, SIFT mode: the own frame's features were set without the 128-byte rows -> DSSS_E_STATE before anything is sent
    (the transport is never called); with the rows the same gather goes through"""
    c, K = _context(small=True, sift=True)
    try:
        frames = R.design_frames(orc, (7, 3), 0, K, True)[2:4]      # 63 and 64 keypoints
        calls = []
        def never(op, arr):
            calls.append(op)
            raise AssertionError("the transport was called")
        c.comm_init_callback(0, 2, never)
        _set_geometry(c, 0, frames[0]); _set_geometry(c, 1, frames[1])
        fr = frames[0]
        c.features_set(0, fr["N"], fr["M"], fr["kps"], fr["desc"], fr["geo"], fr["bb"])
        _refused(E_STATE, lambda: c.features_allgather(2))
        assert calls == []
        _gather(c, orc, 2, 2, 0, frames, K, True, 0x5A)
    finally:
        c.close()

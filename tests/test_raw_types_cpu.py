"""Typed waterfalls (u8, u16, f32 next to f64), the part that needs no GPU: the new entry points are exported and bound, the host
mirror knows CV_16U and test_demo --raw-type refuses a sample its type cannot hold, and the frames of tests/raw_types_ref.py are what
tests/test_gpu_raw_types.py needs them to be -- asserted on the oracle with the widened data, so that no device comparison is vacuous."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import extract_shapes_ref as X
from tests import raw_types_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "diasss_amd", "host")


def test_typed_entry_points_are_exported_and_bound():
    from diasss_amd import capi
    L = capi.lib()
    for s in ("dsss_raw_type_size", "dsss_frame_set_typed", "dsss_frames_set_typed", "dsss_frame_raw_info", "dsss_frame_raw_stats"):
        assert hasattr(L, s), s
    assert [capi.raw_type_size(t) for t in (capi.RAW_F64, capi.RAW_F32, capi.RAW_U16, capi.RAW_U8)] == [8, 4, 2, 1]
    assert [capi.raw_type_size(t) for t in (4, -1, 1 << 20)] == [0, 0, 0]
    assert (capi.RAW_F64, capi.RAW_F32, capi.RAW_U16, capi.RAW_U8) == (R.RAW_F64, R.RAW_F32, R.RAW_U16, R.RAW_U8)
    for name in ("frame_raw_info", "frame_raw_stats"):
        assert callable(getattr(capi.Context, name))


def test_raw_type_is_derived_from_the_dtype():
    import torch
    from diasss_amd import capi
    for t, dt in R.DTYPES.items():
        assert capi.raw_type_of(np.zeros((2, 2), dt)) == R.RAW_TYPE[t]
        assert capi.raw_type_of(torch.zeros((2, 2), dtype=getattr(torch, np.dtype(dt).name))) == R.RAW_TYPE[t]
    assert capi.raw_type_of(torch.zeros((2, 2), dtype=torch.int16), capi.RAW_U16) == capi.RAW_U16      # a u16 image in int16 storage
    for bad in (np.int16, np.int32, np.int64, np.float16, np.bool_):
        with pytest.raises(TypeError):
            capi.raw_type_of(np.zeros((2, 2), bad))
    with pytest.raises(TypeError):
        capi.raw_type_of(torch.zeros((2, 2), dtype=torch.int16))
    with pytest.raises(TypeError):
        capi.raw_type_of(np.zeros((2, 2), np.uint8), capi.RAW_U16)                                  # an explicit type of another size
    z = [np.zeros((4, 6))] * 2
    a = capi.FramesArgs([0, 1], [np.zeros((4, 4), np.uint8), np.zeros((4, 4), np.float32)], [4, 4], [4, 4], z, [np.zeros(4)] * 2, [np.zeros(2)] * 2)
    assert a.raw_type.tolist() == [capi.RAW_U8, capi.RAW_F32] and a.raw_type.dtype == np.int32
    with pytest.raises(TypeError):
        capi.FramesArgs([0], [np.zeros((4, 4), np.int32)], [4], [4], z[:1], [np.zeros(4)], [np.zeros(2)])


def test_synthetic_survey_in_every_sample_type():
    from diasss_amd import synth
    S = synth.Survey(2, 80, 96, tile=128)
    f = S.frame(1)
    assert str(f.dtype) == "torch.float64" and (S.frame(1, "float64") == f).all()
    u16 = S.frame(1, np.uint16); u8 = S.frame(1, "uint8"); f32 = S.frame(1, "float32")
    assert [str(a.dtype) for a in (u16, u8, f32)] == ["torch.uint16", "torch.uint8", "torch.float32"]
    fn = f.numpy()
    assert (u16.numpy() == np.clip(np.rint(fn), 0, 65535)).all() and (u8.numpy() == np.clip(np.rint(fn / 16), 0, 255)).all()
    assert (f32.numpy() == fn.astype(np.float32)).all()
    with pytest.raises(TypeError):
        S.frame(1, "int16")


def _compile(tmp_path, name, srcs, libs=()):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unused-parameter", "-Werror", "-I" + HOST, "-o", exe] + srcs + list(libs))
    return exe


def test_cvlite_knows_16_bit_unsigned(tmp_path):
    src = tmp_path / "esz.cpp"
    src.write_text('#include "cvlite.h"\n#include <cstdio>\nint main() { cv::Mat a(3, 5, CV_16U), b(3, 5, CV_8U), c(3, 5, CV_32F), d(3, 5, CV_64F);\n'
                   '  a.at<unsigned short>(2, 4) = 65535; printf("%zu %zu %zu %zu %zu %d\\n", a.esz(), b.esz(), c.esz(), d.esz(), a.bytes(), (int)a.row(2).at<unsigned short>(0, 4)); return 0; }\n')
    out = subprocess.run([_compile(tmp_path, "esz", [str(src)])], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.split() == ["2", "1", "4", "8", "30", "65535"]


def test_test_demo_refuses_a_sample_its_raw_type_cannot_hold(tmp_path):
    """test_demo --raw-type converts what it loaded before it constructs a frame (so before it needs a device), exactly or not at all"""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    srcs = [os.path.join(HOST, s) for s in ("test_demo.cpp", "frame.cpp", "FEAmatcher.cpp", "optimizer.cpp", "util.cpp", "filestorage.cpp")]
    exe = _compile(tmp_path, "test_demo_raw", srcs, ["-L" + os.path.join(ROOT, "diasss_amd"), "-ldsss", "-L" + rocm + "/lib", "-lamdhip64",
                                                       "-Wl,-rpath," + os.path.join(ROOT, "diasss_amd"), "-Wl,-rpath," + rocm + "/lib"])
    N, M = 6, 8

    def run(raw, t):
        d = tmp_path / ("frames_" + t); d.mkdir(exist_ok=True)
        with open(d / "frame_000.bin", "wb") as f:
            f.write(struct.pack("ii", N, M)); f.write(raw.tobytes())
            f.write(np.zeros(N * 6).tobytes()); f.write(np.zeros(N).tobytes()); f.write(np.zeros(M // 2).tobytes())
        return subprocess.run([exe, str(d), "--raw-type", t], capture_output=True, text=True, timeout=60)

    raw = np.arange(N * M, dtype=np.float64).reshape(N, M)
    for t, v in (("u8", 3.5), ("u8", 256.0), ("u8", -1.0), ("u16", 65536.0), ("u16", 0.25), ("f32", 0.1), ("f32", 1e300), ("u8", float("nan"))):
        bad = raw.copy(); bad[4, 3] = v
        out = run(bad, t)
        assert out.returncode == 1 and "--raw-type refused" in out.stdout and "(4, 3)" in out.stdout and "not representable" in out.stdout, (t, v, out.stdout, out.stderr)
    out = run(raw, "i16")
    assert out.returncode == 1 and "u8, u16, f32 or f64" in out.stdout


# ---------------------------------------------------------------- preconditions of the GPU cases, on the oracle
@pytest.mark.parametrize("t", R.NARROW)
@pytest.mark.parametrize("kind", R.KINDS)
def test_case_frames_keep_keypoints_on_their_levels(orc, kind, t):
    """every case frame, after quantisation, still yields keypoints on every pyramid level it has: the one level of the shapes below
    83 x 83 (a second level of scale 1.2 would be under the 69 px the extraction accepts), both levels of 100 x 700"""
    for shape in R.SHAPES:
        q, w, orb, ref = R.case(orc, kind, t, shape)
        assert q.dtype == R.DTYPES[t] and (w == q).all()
        octs = set(ref["kps"]["octave"].tolist())
        assert octs == set(range(shape[2])), (kind, t, shape, octs)
        assert len(ref["levels"]) == shape[2]
    assert R.SHAPES[-1][2] == 2


@pytest.mark.parametrize("t", R.NARROW + ("f64",))
def test_hot_pixels_erase_mask_pixels_in_every_type(orc, t):
    mp = X.mask_params(orc, **R.MASK)
    for N, M, _, _ in R.SHAPES:
        q = R.frame("flat_with_hot", t, N, M)
        cold = q.copy()
        for i, j in R.hot_pixels(N, M): cold[i, j] = q[0, 0]
        erased = int((orc.mask(R.widen(q), mp) != orc.mask(R.widen(cold), mp)).sum())
        assert erased == 2 * (2 * R.MASK["r"]) ** 2, (t, N, M, erased)


def test_f32_frames_make_the_summation_order_observable(orc):
    """the fixed tree's mean of a widened f32 frame is not the row-major running sum's: a form that adds in another order shows"""
    for kind in R.KINDS:
        for N, M, _, _ in R.SHAPES:
            w = R.widen(R.frame(kind, "f32", N, M))
            m = orc.lib().orc_mean(orc.dp(w), N, M)
            assert R.bits(m) != R.bits(R.sequential_mean(w)), (kind, N, M)


@pytest.mark.parametrize("t", R.INTEGER)
def test_integer_frames_have_an_order_free_mean(orc, t):
    for kind in R.KINDS:
        for N, M, _, _ in R.SHAPES:
            q = R.frame(kind, t, N, M); w = R.widen(q)
            assert R.bits(orc.lib().orc_mean(orc.dp(w), N, M)) == R.bits(R.exact_mean(q)), (kind, t, N, M)
    for q in (np.full((69, 2000), 65535, np.uint16), np.full((69, 2000), 255, np.uint8)):
        w = R.widen(q)
        assert R.bits(orc.lib().orc_mean(orc.dp(w), 69, 2000)) == R.bits(float(q[0, 0])) == R.bits(R.exact_mean(q))

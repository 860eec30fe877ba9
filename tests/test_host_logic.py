"""CPU tests of the product's host-side logic and of the C-ABI surface (no GPU needed):
- libdsss.so loads and exports every symbol include/dsss.h declares;
- the host quadtree (DistributeOctTree) agrees with the oracle on seeded candidate sets;
- without a device the library fails loudly (no CPU fallback)."""
import ctypes as C
import os
import re
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    hdr = open(os.path.join(ROOT, "include", "dsss.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(dsss_[a-z0-9_]+)\s*\(", hdr)))


def test_cabi_exports_every_declared_symbol():
    from diasss_amd import capi
    L = capi.lib()
    syms = _declared_symbols()
    assert len(syms) >= 40
    missing = [s for s in syms if not hasattr(L, s)]
    assert not missing, missing


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    from diasss_amd import capi
    with pytest.raises(capi.DsssError):
        capi.Context(max_frames=2)
    assert b"no HIP device" in capi.lib().dsss_strerror(-1)


@pytest.mark.parametrize("seed,n,w,h,quota", [(1, 3000, 603, 903, 300), (2, 20000, 990, 1960, 501), (3, 50, 400, 300, 100),
                                              (4, 5000, 1200, 300, 242), (5, 1, 100, 100, 10), (6, 800, 170, 370, 201)])
def test_host_quadtree_matches_oracle(orc, seed, n, w, h, quota):
    from diasss_amd import capi
    rng = np.random.default_rng(seed)
    pts = set()
    while len(pts) < n:
        pts.add((int(rng.integers(3, w - 3)), int(rng.integers(3, h - 3))))
    pts = sorted(pts, key=lambda p: (p[1] // 30, p[0] // 30, p[1], p[0]))     # cell-major like the FAST output
    xs = np.array([p[0] for p in pts], np.float32); ys = np.array([p[1] for p in pts], np.float32)
    resp = rng.integers(7, 120, n).astype(np.float32)                      # many ties on purpose
    k_o = np.zeros(n, np.int32)
    no = orc.lib().orc_quadtree(orc.fp(xs), orc.fp(ys), orc.fp(resp), n, 16, 16 + w, 16, 16 + h, quota, orc.ip(k_o))
    k_p = np.zeros(n, np.int32); npk = C.c_int(0)
    rc = capi.lib().dsss_host_quadtree(xs.ctypes.data_as(C.c_void_p), ys.ctypes.data_as(C.c_void_p), resp.ctypes.data_as(C.c_void_p), n,
                                       16, 16 + w, 16, 16 + h, quota, k_p.ctypes.data_as(C.c_void_p), C.byref(npk))
    assert rc == 0 and npk.value == no
    assert (k_p[:no] == k_o[:no]).all()


def test_load_input_data_reference_layout(tmp_path):
    """Util::LoadInputData (util.cpp:45-213): five folders, FileStorage XML and YAML matrices + text
    columns, files in name order, exact f64 round trip -- host code only, built with g++"""
    import subprocess
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import export_survey as E
    host = os.path.join(ROOT, "diasss_amd", "host")
    subprocess.check_call(["make", "-C", host, "-s", "load_check"])
    rng = np.random.default_rng(5)
    for yaml in (False, True):
        frames = []
        for f in range(3):
            N, M = 40 + 7 * f, 32 + 2 * f
            raw = rng.rayleigh(1.0, (N, M)) * 10 ** rng.uniform(-3, 3)
            raw[0, 0] = 1.0 / 3.0; raw[-1, -1] = 123456789.123456789e-7
            pose = rng.standard_normal((N, 6)); alt = 9 + rng.standard_normal(N); gr = 0.05 * np.arange(M // 2)
            anno = rng.integers(0, 1000, (5 + f, 7)).astype(np.int32)
            frames.append((raw, pose, alt, gr, anno))
        d = E.export_reference_layout(str(tmp_path / ("yaml" if yaml else "xml")), frames, yaml=yaml)
        out = subprocess.check_output([os.path.join(host, "load_check"), d["image"], d["pose"], d["altitude"], d["groundrange"], d["annotation"]], text=True)
        got = {}
        for ln in out.splitlines():
            t = ln.split()
            if t[0] in ("@img", "@pose", "@alt", "@gr"):
                got[(t[0][1:], int(t[1]))] = (int(t[2]), int(t[3]), float.fromhex(t[4]), float.fromhex(t[5]), float.fromhex(t[6]))
            elif t[0] == "@anno":
                got[("anno", int(t[1]))] = (int(t[2]), int(t[3]), int(t[4]), int(t[6]))
        for f, (raw, pose, alt, gr, anno) in enumerate(frames):
            for kind, a in (("img", raw), ("pose", pose), ("alt", alt), ("gr", gr)):
                r, c, s_, first, last = got[(kind, f)]
                assert (r, c) == ((a.shape + (1,))[:2])
                assert first == a.reshape(-1)[0] and last == a.reshape(-1)[-1]          # exact round trip of the text form
                assert abs(s_ - float(np.sum(a.astype(np.longdouble)))) <= 1e-9 * max(1.0, abs(s_))
            assert got[("anno", f)] == (anno.shape[0], anno.shape[1], int(anno.sum()), 4)   # CV_32S


def test_drop_in_driver_compiles_and_links_against_the_library(tmp_path):
    """north_star: "Host code stays C++ with the existing Frame/constraint API surface so test_demo links unchanged".  The
    driver loop of the reference (diasss_amd/host/test_demo.cpp: Util::LoadInputData, Frame, FEAmatcher, Optimizer) is compiled
    with -Wall -Werror against the host mirror in diasss_amd/host/, linked with the drop-in classes + libdsss.so outside the tree,
    and the resulting binary must start without a device and print its usage for both input forms."""
    import subprocess
    host = os.path.join(ROOT, "diasss_amd", "host")
    flags = ["-std=c++17", "-Wall", "-Wno-unused-parameter", "-Werror", "-I" + host]
    srcs = [os.path.join(host, s) for s in ("test_demo.cpp", "frame.cpp", "FEAmatcher.cpp", "optimizer.cpp", "util.cpp", "filestorage.cpp")]
    subprocess.check_call(["g++", "-fsyntax-only"] + flags + [srcs[0]])
    exe = str(tmp_path / "test_demo_dropin")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-O1"] + flags + ["-o", exe] + srcs
                          + ["-L" + os.path.join(ROOT, "diasss_amd"), "-ldsss", "-L" + rocm + "/lib", "-lamdhip64",
                             "-Wl,-rpath," + os.path.join(ROOT, "diasss_amd"), "-Wl,-rpath," + rocm + "/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "--image" in out.stdout and "--groundrange" in out.stdout and "frame_%03d.bin" in out.stdout

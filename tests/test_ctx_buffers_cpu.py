"""CPU: the failure path of the context's buffer ownership (diasss_amd/csrc/dsss_internal.h: dsss_buf, dsss_family_alloc) and of
dsss_ensure_store, on a machine WITHOUT a device, where every hipMalloc / hipHostMalloc fails with hipErrorNoDevice -- a free,
deterministic run of the path that no GPU test may provoke.  The checks live in a stand-alone program
(diasss_amd/host/ctx_buffers_check.cpp, own main) built with -fsanitize=address,undefined on the host side; nothing is preloaded
and nothing is loaded into Python.  What it holds:
  - reserve: DSSS_E_HIP, dsss_last_error's text set, p == nullptr and cap == 0 -- also when the buffer held a block before;
    reserve_keep leaves the buffer as it was;
  - the family helper: a family whose first member was set ends with every member null and capacity 0;
  - release() twice, move construction / assignment, a moved frame, destruction of moved-from objects: clean under ASan;
  - dsss_ensure_store fails twice in a row and leaves no store.  (It used to test `kps` alone: a failure at a later one of its
    seven allocations left kps set -- hipMalloc leaves its output as it was -- and the next call returned DSSS_OK over null
    pointers.  Without a device the FIRST allocation fails, so these two calls hold the return codes and the empty store only;
    the half-built state itself is what the family check starts from.)"""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_buffer_ownership_failure_path_under_host_sanitizers():
    from diasss_amd import capi
    ndev = ctypes.c_int(0)
    if capi._load_hip_runtime().hipGetDeviceCount(ctypes.byref(ndev)) == 0 and ndev.value > 0:
        pytest.skip("a HIP device is present: allocations succeed, the failure path cannot be exercised here")
    host = os.path.join(ROOT, "diasss_amd", "host")
    subprocess.check_call(["make", "-C", host, "-s", "ctx_buffers_check"])
    out = subprocess.run([os.path.join(host, "ctx_buffers_check")], capture_output=True, text=True, timeout=120)
    print(out.stdout, out.stderr)
    if out.returncode == 77:
        pytest.skip("the program found a HIP device")
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ctx_buffers_check: ok" in out.stdout
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error:" not in out.stderr

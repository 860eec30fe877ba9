"""CPU: the LM decisions shared by lc_kernel, tri_kernel and the pose-graph LM (diasss_amd/csrc/dsss_lm.h) against a hand-written truth
table of GTSAM's rule as oracle/orc_lc.c states it: the trial verdict on both sides of every comparison (linChange negative, zero, at and
above eps * oldLin; fidelity at, below and above minFid; |costChange| around relTol * err; err == 0; NaN and infinite errors), the lambda
schedule up to lamMax exactly, and the outer condition at maxIter - 1 / maxIter and with a non-finite cur.  The rows are in
diasss_amd/host/lm_rule_table.h; a stand-alone program walks them (diasss_amd/host/lm_rule_check.cpp, own main) built with
-fsanitize=address,undefined on the host side; nothing is preloaded and nothing is loaded into Python.  The device walks the same rows in
tests/test_gpu_dev_probe.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lm_rule_truth_table_under_host_sanitizers():
    host = os.path.join(ROOT, "diasss_amd", "host")
    subprocess.check_call(["make", "-C", host, "-s", "lm_rule_check"])
    out = subprocess.run([os.path.join(host, "lm_rule_check")], capture_output=True, text=True, timeout=120)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "lm_rule_check: ok" in out.stdout
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error:" not in out.stderr

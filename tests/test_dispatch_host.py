"""The pure host half of the render path (small-pathtracer_amd/csrc/spt_dispatch.cpp: build_geo,
the kernel choice, the launch sizing) under AddressSanitizer and UBSan, as a stand-alone program
(tests/probe/spt_dispatch_check.cpp). CPU only: the program has no HIP in it and is never loaded
into Python.

It runs build_geo / spt_select_kernel on scenes at the sizes where the 64-entry arrays could
overrun (1 and exactly 64 primitives, 64 rectangles of one kind, 11 boxes behind a room) and asserts
plan_launch on four shapes whose expected sizes were derived by hand.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "probe")
HOSTCXX = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(HOSTCXX), reason="needs the ROCm host clang")
def test_dispatch_host_under_sanitizers():
    r = subprocess.run(["make", "-s", "-C", PROBE, "spt_dispatch_check"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    r = subprocess.run([os.path.join(PROBE, "spt_dispatch_check")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "spt_dispatch_check ok" in r.stdout

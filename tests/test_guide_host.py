"""The guide's CPU resolve (small-pathtracer_amd/csrc/spt_guide_host.cpp: the statement every GPU
guide test compares the device resolve against) under AddressSanitizer and UBSan, as a stand-alone
program (tests/probe/spt_guide_check.cpp). CPU only: the program has no HIP in it and is never
loaded into Python.

It calls spt_guide_resolve_host on the edge records of the header's rule (hits 0, 0 < hits < n,
negative normal sums, albedo sums at and above the clamp, the largest depth and spp), full, partial
and with no sample, with planes left NULL, on a zero-pixel guide, and on the refused arguments, and
asserts results derived by hand.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "probe")
HOSTCXX = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(HOSTCXX), reason="needs the ROCm host clang")
def test_guide_host_under_sanitizers():
    r = subprocess.run(["make", "-s", "-C", PROBE, "-f", "guide_check.mk", "spt_guide_check"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    r = subprocess.run([os.path.join(PROBE, "spt_guide_check")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "spt_guide_check ok" in r.stdout
    assert "Sanitizer" not in r.stdout + r.stderr and "runtime error" not in r.stderr

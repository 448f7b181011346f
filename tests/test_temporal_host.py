"""Temporal accumulation's CPU statement (small-pathtracer_amd/csrc/spt_temporal_host.cpp: what every GPU
temporal test compares the kernel against) under AddressSanitizer and UBSan, as a stand-alone program
(tests/probe/spt_temporal_check.cpp). CPU only: the program has no HIP in it and is never loaded into
Python.

It calls spt_temporal_accumulate_host at 1x1, 3x2, 5x1, 1x5, 17x13 and 40x56 as a first frame, with the
same camera again, with a moved camera, with a previous camera that the points lie behind and with one so
far to the side that every tap falls outside; with both flag values, with n_out and hist given and left
NULL, on inputs and a previous state that are not finite, and on every refused argument. Every plane is
a vector of exactly its size, so a tap address formed before its range check would be reported.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "probe")
HOSTCXX = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(HOSTCXX), reason="needs the ROCm host clang")
def test_temporal_host_under_sanitizers():
    r = subprocess.run(["make", "-s", "-C", PROBE, "-f", "temporal_check.mk", "spt_temporal_check"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    r = subprocess.run([os.path.join(PROBE, "spt_temporal_check")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "spt_temporal_check ok" in r.stdout
    assert "Sanitizer" not in r.stdout + r.stderr and "runtime error" not in r.stderr

"""The filter bank's CPU statement and its summary (small-pathtracer_amd/csrc/spt_denoise_host.cpp: what
every GPU bank test compares the device kernels against) under AddressSanitizer and UBSan, as a
stand-alone program (tests/probe/spt_denoise_bank_check.cpp). CPU only: the program has no HIP in it and
is never loaded into Python.

It calls spt_denoise_bank_host at 1x1, 3x2, 5x1, 1x5 and 17x13 with 1, 2 and 4 candidates (iterations 6,
3, 0 and 1), error_iterations 0..3 and both pair_flags, with mse and choice given and left NULL, with one
candidate against spt_denoise_pair_host, on swapped halves, on inputs that are not finite, and on every
refused argument; and spt_denoise_bank_summary_host on the planes it gave. Every plane is a vector of
exactly its size, so the small images at step 32 are where a tap address that was not clipped would be
reported.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "probe")
HOSTCXX = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(HOSTCXX), reason="needs the ROCm host clang")
def test_denoise_bank_host_under_sanitizers():
    r = subprocess.run(["make", "-s", "-C", PROBE, "-f", "denoise_bank_check.mk", "spt_denoise_bank_check"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    r = subprocess.run([os.path.join(PROBE, "spt_denoise_bank_check")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "spt_denoise_bank_check ok" in r.stdout
    assert "Sanitizer" not in r.stdout + r.stderr and "runtime error" not in r.stderr

"""The light guide's CPU statements (small-pathtracer_amd/csrc/spt_guide_light_host.cpp: the resolve
and the shade every GPU light-guide test compares the device kernels against) under AddressSanitizer
and UBSan, as a stand-alone program (tests/probe/spt_guide_light_check.cpp). CPU only: the program has
no HIP in it and is never loaded into Python.

It calls spt_light_guide_resolve_host on the edge records of the header's rule (tested 0, lit == tested,
0 < lit < tested, weight sums at and above one sample's clamp, the largest spp), full, partial and with
no sample, with planes left NULL, on a zero-pixel light guide and on the refused arguments, and
spt_light_shade_host at both ends of its floor's range, in place and refused, and asserts results
derived by hand.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "probe")
HOSTCXX = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(HOSTCXX), reason="needs the ROCm host clang")
def test_guide_light_host_under_sanitizers():
    r = subprocess.run(["make", "-s", "-C", PROBE, "-f", "guide_light_check.mk", "spt_guide_light_check"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    r = subprocess.run([os.path.join(PROBE, "spt_guide_light_check")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "spt_guide_light_check ok" in r.stdout
    assert "Sanitizer" not in r.stdout + r.stderr and "runtime error" not in r.stderr

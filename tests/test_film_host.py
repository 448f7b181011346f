"""The film's CPU statements (small-pathtracer_amd/csrc/spt_film_host.cpp: the resolve, the error
map, the summary and the selection that every GPU film test compares against) under AddressSanitizer
and UBSan, as a stand-alone program (tests/probe/spt_film_check.cpp). CPU only: the program has no
HIP in it and is never loaded into Python.

It calls the seven statements at the smallest shapes where they can go wrong (1x1, 5x3, rows = 0;
the two-row and the 4097-row table; counts 0, 1, 2, b_max with and without the retired bit, and
b_max + 1 refused; batch sums at the bound batch * 2^31 and a B * M2 above 64 bits), asserts results
derived by hand, and that with every count equal the adaptive statements return the uniform ones bit
for bit.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "probe")
HOSTCXX = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(HOSTCXX), reason="needs the ROCm host clang")
def test_film_host_under_sanitizers():
    r = subprocess.run(["make", "-s", "-C", PROBE, "spt_film_check"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    r = subprocess.run([os.path.join(PROBE, "spt_film_check")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "spt_film_check ok" in r.stdout
    assert "Sanitizer" not in r.stdout + r.stderr and "runtime error" not in r.stderr

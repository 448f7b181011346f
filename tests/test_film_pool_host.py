"""The pooled error's CPU statements (spt_film_noise_pool_map_host and
spt_film_adaptive_select_pooled_host in small-pathtracer_amd/csrc/spt_film_host.cpp, what
tests/test_gpu_film_pool.py compares the device with) under AddressSanitizer and UBSan, as a
stand-alone program (tests/probe/spt_film_pool_check.cpp, built by tests/probe/pool_check.mk with the
compiler and flags of the spt_film_check rule). CPU only: the program has no HIP in it and is never
loaded into Python.

It runs the two statements where a window can leave the film: every border pixel of 5x3 and 9x7 at
R = 1 and 2, R = 16 above the film's size, bands of 3, 3 and 1 rows (and of 1 row, and above the
rows), the 1x1 film with the centre excluded (n == 0: the own rule), a count of 1, rows = 0 and the
refused arguments; its buffers have exactly the statement's sizes.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "probe")
HOSTCXX = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(HOSTCXX), reason="needs the ROCm host clang")
def test_film_pool_host_under_sanitizers():
    r = subprocess.run(["make", "-s", "-C", PROBE, "-f", "pool_check.mk", "spt_film_pool_check"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    r = subprocess.run([os.path.join(PROBE, "spt_film_pool_check")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "spt_film_pool_check ok" in r.stdout
    assert "Sanitizer" not in r.stdout + r.stderr and "runtime error" not in r.stderr

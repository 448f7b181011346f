"""What a film and a guide share (small-pathtracer_amd/csrc/spt_window_shape.h: the create-time
checks, the four checks of a sample window, the film-against-guide comparison) under
AddressSanitizer and UBSan, as a stand-alone program (tests/probe/spt_window_check.cpp). CPU only:
the program has no HIP in it and is never loaded into Python.

It asserts the accepted edges (1x1 @ 1, a shard without rows, tile_rows 0 read as 8, both pixel caps
exactly) and, for both nouns, the exact text of every rejection from the smallest change that trips
it, and that a call tripping two checks gets the earlier message.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "probe")
HOSTCXX = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(HOSTCXX), reason="needs the ROCm host clang")
def test_window_shape_host_under_sanitizers():
    r = subprocess.run(["make", "-s", "-C", PROBE, "-f", "window_check.mk", "spt_window_check"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    r = subprocess.run([os.path.join(PROBE, "spt_window_check")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "spt_window_check ok" in r.stdout
    assert "Sanitizer" not in r.stdout + r.stderr and "runtime error" not in r.stderr

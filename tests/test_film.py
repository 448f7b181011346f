"""The film's host side (no GPU): spt_film_resolve_host against its numpy statement, the film file
round trip, and the ABI markers (version still 6, SPT_HAS_FILM defined).

The resolve is exact arithmetic on float32: (float)sum is the correctly rounded uint64 -> float32
conversion (numpy's astype), * 2^-31 is exact, the preview factor r = float32(float64(spp_total) /
samples_done) is rounded once and applied as a second, separate multiply; then min(., 1). So every
comparison here is bitwise."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# hand-made sums: zero, one ulp of 1.31, values whose float32 conversion must round (2^24 + 1,
# 2^31 - 1), exactly 1.0 (2^31), just above, far above, and the top of uint64
HAND = np.array([0, 1, 3, (1 << 24) + 1, 123456789, (1 << 30) + 12345, (1 << 31) - 129, (1 << 31) - 1,
                 1 << 31, (1 << 31) + 1, (1 << 31) + 257, 3 << 31, 1 << 40, (1 << 63) + (1 << 39),
                 (1 << 64) - 1], dtype=np.uint64)


def _sums(w, rows):
    n = 3 * w * rows
    return np.resize(HAND, n).reshape(rows, w, 3)


def numpy_resolve(sums, spp_total, samples_done):
    """The statement of spt.h's spt_film_resolve, independent of the library."""
    f = sums.astype(np.float32) * np.float32(2.0 ** -31)
    if samples_done == 0:
        return np.zeros(sums.shape, np.float32)
    if samples_done != spp_total:
        f = f * np.float32(np.float64(spp_total) / np.float64(samples_done))
    return np.minimum(f, np.float32(1.0)).astype(np.float32)


def test_resolve_host_full_film(spt):
    s = _sums(5, 3)
    got = spt.film_resolve_host(s, 5, 3, 16, 16)
    assert got.dtype == np.float32 and got.shape == (3, 5, 3)
    assert np.array_equal(got, np.minimum(s.astype(np.float32) * np.float32(2.0 ** -31), np.float32(1)))
    flat, src = got.ravel(), s.ravel()
    assert np.all(flat[src > (1 << 31)] == 1.0)  # a sum above 2^31 clamps to 1
    assert flat[list(src).index(1 << 31)] == 1.0
    assert 0.0 < flat[list(src).index((1 << 31) - 129)] < 1.0
    assert flat[0] == 0.0


@pytest.mark.parametrize("spp,done", [(16, 5), (16, 1), (16, 15), (7, 3), (512, 200), (1000, 999)])
def test_resolve_host_preview_equals_numpy(spt, spp, done):
    s = _sums(7, 2)
    got = spt.film_resolve_host(s, 7, 2, spp, done)
    assert np.array_equal(got, numpy_resolve(s, spp, done))


def test_resolve_host_empty_film_is_zero(spt):
    s = _sums(4, 4)
    got = spt.film_resolve_host(s, 4, 4, 16, 0)
    assert np.array_equal(got, np.zeros((4, 4, 3), np.float32))


@pytest.mark.parametrize("w,rows,spp,done", [(0, 2, 16, 4), (-3, 2, 16, 4), (4, -1, 16, 4), (4, 2, 0, 0),
                                             (4, 2, 16, -1), (4, 2, 16, 17)])
def test_resolve_host_bad_info_is_invalid_arg(spt, w, rows, spp, done):
    import ctypes
    lib = spt.load_library()
    info = spt.spt_film_info(w, rows, spp, done)
    sums = np.zeros(64, np.uint64)
    out = np.full(64, 7.0, np.float32)
    assert lib.spt_film_resolve_host(sums.ctypes.data, ctypes.byref(info), out.ctypes.data) == 1
    assert np.all(out == 7.0)  # rejected: nothing written
    assert lib.spt_film_resolve_host(None, None, None) == 1
    good = spt.spt_film_info(2, 2, 16, 16)
    assert lib.spt_film_resolve_host(None, ctypes.byref(good), out.ctypes.data) == 1
    assert lib.spt_film_resolve_host(sums.ctypes.data, ctypes.byref(good), None) == 1


def test_film_file_round_trip(spt, tmp_path):
    s = _sums(6, 5)
    path = str(tmp_path / "f.bin")
    spt.write_film_file(path, s, 6, 5, 64, 23)
    data = open(path, "rb").read()
    assert data[:8] == b"SPTFILM1" and len(data) == 32 + 8 * s.size
    assert np.array_equal(np.frombuffer(data, "<i4", 4, 8), [6, 5, 64, 0])
    assert int(np.frombuffer(data, "<i8", 1, 24)[0]) == 23
    assert np.array_equal(np.frombuffer(data, "<u8", offset=32), s.ravel())
    back, info = spt.read_film_file(path)
    assert info == {"width": 6, "rows": 5, "spp_total": 64, "samples_done": 23}
    assert back.dtype == np.uint64 and np.array_equal(back, s)
    for bad in (data[:-8], data + b"\0" * 8, b"XPTFILM1" + data[8:], data[:20]):
        open(path, "wb").write(bad)
        with pytest.raises(spt.SptError):
            spt.read_film_file(path)
    with pytest.raises(spt.SptError):
        spt.write_film_file(path, s, 6, 4, 64, 23)


def test_sample_windows_cover_the_samples_once(spt):
    for spp, k in [(16, 3), (16, 16), (5, 8), (512, 7), (1, 1)]:
        w = spt.sample_windows(spp, k)
        assert all(c >= 1 for _, c in w) and len(w) == min(spp, k)
        assert [b for b, _ in w] == [0] + list(np.cumsum([c for _, c in w])[:-1])
        assert sum(c for _, c in w) == spp
        assert max(c for _, c in w) - min(c for _, c in w) <= 1


def test_abi_version_stays_and_film_is_announced(spt):
    assert spt.load_library().spt_abi_version() == 6
    hdr = open(os.path.join(ROOT, "include", "spt.h")).read()
    assert re.search(r"^#define SPT_ABI_VERSION 6\b", hdr, re.M)
    assert re.search(r"^#define SPT_HAS_FILM 1\b", hdr, re.M)
    for name in ("spt_film_create", "spt_film_destroy", "spt_film_info_get", "spt_film_clear",
                 "spt_film_render_async", "spt_film_resolve", "spt_film_merge", "spt_film_download",
                 "spt_film_upload", "spt_film_resolve_host"):
        assert name in spt.EXPORTS and getattr(spt.load_library(), name) is not None


def test_film_needs_the_gpu(spt):
    """No CPU fallback: without a device a film cannot be created."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(spt.SptError) as e:
        spt.Film(spt.default_params(width=8, height=8, spp=4))
    assert e.value.status in (2, 3)

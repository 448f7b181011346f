"""The noise film's host side (no GPU): the error map and the image figures as pure host functions
against a statement in Python integers, the SPTFILM2 file, and the ABI markers.

Statement (include/spt.h): D = B * M2 - S^2 in exact integers, d = (double)hi * 2^64 + (double)lo,
se = (float)(sqrt(d) * k), k = spp_total / (batch * 2^31 * B * sqrt(B - 1)); se = 0 where the resolved
value is the clamp 1.0f. Tolerances: a float within relative 2^-21 (4 ulp: the two double roundings
of sqrt and the product, then one float rounding); a summary figure within relative 1e-9 (n * 2^-53
for n < 10^6 terms); clamped channels and D = 0 exactly 0."""
import ctypes
import math
import os
import re
import struct

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, ROWS, SPP, BATCH = 9, 7, 64, 8
REL_F32 = 2.0 ** -21
REL_SUM = 1e-9


def numpy_resolve(sums, spp_total, samples_done):
    f = sums.astype(np.float32) * np.float32(2.0 ** -31)
    if samples_done != spp_total:
        f = f * np.float32(np.float64(spp_total) / np.float64(samples_done))
    return np.minimum(f, np.float32(1.0)).astype(np.float32)


def synthetic(B, seed=5):
    """B batch sums P per element -> (S, M2 as (lo, hi) pairs, the Python-int lists). Element 0..2:
    equal batches (D = 0); 3..5: a pixel far above the clamp, batches near the bound batch * 2^31
    (M2's hi word in use); 6: one batch holds everything, resolved just below the clamp (with all
    eight batches D's hi word is in use); 7: all zero; the rest: dim values with a spread."""
    rng = np.random.default_rng(seed)
    n = 3 * W * ROWS
    top = BATCH << 31
    P = [[int(v) for v in rng.integers(0, top // 160, size=B)] for _ in range(n)]
    for e in range(3):
        P[e] = [123456789 + e] * B
    for e in range(3, 6):
        P[e] = [int(v) for v in rng.integers(top // 2, top, size=B)]
    P[6] = [(2 ** 31 - 4096) * B * BATCH // SPP] + [0] * (B - 1)
    P[7] = [0] * B
    S = [sum(p) for p in P]
    M = [sum(v * v for v in p) for p in P]
    sums = np.array(S, dtype=np.uint64).reshape(ROWS, W, 3)
    m2 = np.array([[m & (2 ** 64 - 1), m >> 64] for m in M], dtype=np.uint64).reshape(ROWS, W, 3, 2)
    return sums, m2, S, M


def statement(S, M, B, samples_done):
    """-> (se list as Python floats, d * k^2 list, clamped flags) from Python integers."""
    k = SPP / (BATCH * 2.0 ** 31 * B * math.sqrt(B - 1))
    res = numpy_resolve(np.array(S, dtype=np.uint64), SPP, samples_done)
    se, dk2, cl = [], [], []
    for s, m, r in zip(S, M, res):
        D = B * m - s * s
        assert D >= 0
        clamp = bool(r == np.float32(1.0))
        se.append(0.0 if clamp else math.sqrt(D) * k)
        dk2.append(0.0 if clamp else float(D) * k * k)
        cl.append(clamp)
    return se, dk2, cl


@pytest.mark.parametrize("B", [8, 5, 2], ids=["full", "preview", "two_batches"])
def test_map_host_against_python_integers(spt, B):
    sums, m2, S, M = synthetic(B)
    done = B * BATCH
    got = spt.film_noise_map_host(sums, m2, W, ROWS, SPP, done, BATCH, B)
    assert got.dtype == np.float32 and got.shape == (ROWS, W, 3)
    want, _, cl = statement(S, M, B, done)
    g = got.reshape(-1)
    assert cl[3] and cl[4] and cl[5] and not cl[0] and sum(cl) >= 3
    for e in range(len(S)):
        if cl[e] or want[e] == 0.0:
            assert g[e] == 0.0, e  # the clamp, and D = 0 (equal batches, all-zero batches): exact
        else:
            assert abs(float(g[e]) - want[e]) <= REL_F32 * want[e], (e, g[e], want[e])
    assert g[0] == 0.0 and g[7] == 0.0 and g[6] > 0.0 and not cl[6]
    assert B < 8 or (B * M[6] - S[6] * S[6]) >> 64 > 0


@pytest.mark.parametrize("B", [8, 5], ids=["full", "preview"])
def test_summary_host_against_python_integers(spt, B):
    sums, m2, S, M = synthetic(B)
    done = B * BATCH
    got = spt.film_noise_summary_host(sums, m2, W, ROWS, SPP, done, BATCH, B)
    se, dk2, cl = statement(S, M, B, done)
    npix = W * ROWS
    for c in range(3):
        want = math.sqrt(math.fsum(dk2[c::3]) / npix)
        assert abs(got["rmse"][c] - want) <= REL_SUM * want, (c, got["rmse"][c], want)
    want = math.sqrt(math.fsum(dk2) / (3 * npix))
    assert abs(got["rmse_all"] - want) <= REL_SUM * want
    assert abs(got["se_max"] - max(se)) <= REL_F32 * max(se)
    assert got["clamped"] == sum(cl) and got["batches_done"] == B
    # the map's own maximum, bit for bit
    assert got["se_max"] == float(spt.film_noise_map_host(sums, m2, W, ROWS, SPP, done, BATCH, B).max())


def test_all_clamped_or_constant_is_exactly_zero(spt):
    B, n = 4, 3 * W * ROWS
    P = [(BATCH << 31) if e % 2 else 1000 + e for e in range(n)]  # the bound (clamped), or constant
    sums = np.array([B * p for p in P], dtype=np.uint64)
    M = [B * p * p for p in P]
    m2 = np.array([[m & (2 ** 64 - 1), m >> 64] for m in M], dtype=np.uint64)
    got = spt.film_noise_map_host(sums, m2, W, ROWS, SPP, B * BATCH, BATCH, B)
    assert not got.any()
    s = spt.film_noise_summary_host(sums, m2, W, ROWS, SPP, B * BATCH, BATCH, B)
    assert s["rmse"] == [0.0, 0.0, 0.0] and s["rmse_all"] == 0.0 and s["se_max"] == 0.0
    assert s["clamped"] == n // 2


def test_fewer_than_two_batches_and_null_arguments_are_rejected(spt):
    sums, m2, _, _ = synthetic(4)
    for B in (0, 1):
        with pytest.raises(spt.SptError) as e:
            spt.film_noise_map_host(sums, m2, W, ROWS, SPP, B * BATCH, BATCH, B)
        assert e.value.status == 1
        with pytest.raises(spt.SptError) as e:
            spt.film_noise_summary_host(sums, m2, W, ROWS, SPP, B * BATCH, BATCH, B)
        assert e.value.status == 1
    lib = spt.load_library()
    info = spt.spt_film_info(W, ROWS, SPP, 32)
    noise = spt.spt_film_noise_info(1, BATCH, 4)
    plain = spt.spt_film_noise_info(0, 0, 0)
    out = np.zeros(3 * W * ROWS, np.float32)
    summ = spt.spt_noise_summary()
    a, m = np.ascontiguousarray(sums), np.ascontiguousarray(m2)
    I, N = ctypes.byref(info), ctypes.byref(noise)
    assert lib.spt_film_noise_map_host(a.ctypes.data, m.ctypes.data, I, N, out.ctypes.data) == 0
    assert lib.spt_film_noise_map_host(None, m.ctypes.data, I, N, out.ctypes.data) == 1
    assert lib.spt_film_noise_map_host(a.ctypes.data, None, I, N, out.ctypes.data) == 1
    assert lib.spt_film_noise_map_host(a.ctypes.data, m.ctypes.data, I, N, None) == 1
    assert lib.spt_film_noise_map_host(a.ctypes.data, m.ctypes.data, None, N, out.ctypes.data) == 1
    assert lib.spt_film_noise_map_host(a.ctypes.data, m.ctypes.data, I, None, out.ctypes.data) == 1
    assert lib.spt_film_noise_map_host(a.ctypes.data, m.ctypes.data, I, ctypes.byref(plain),
                                       out.ctypes.data) == 1
    assert lib.spt_film_noise_summary_host(a.ctypes.data, m.ctypes.data, I, N, ctypes.byref(summ)) == 0
    assert lib.spt_film_noise_summary_host(None, m.ctypes.data, I, N, ctypes.byref(summ)) == 1
    assert lib.spt_film_noise_summary_host(a.ctypes.data, None, I, N, ctypes.byref(summ)) == 1
    assert lib.spt_film_noise_summary_host(a.ctypes.data, m.ctypes.data, I, N, None) == 1


def test_noise_film_file_round_trip(spt, tmp_path):
    sums, m2, _, _ = synthetic(5)
    path = str(tmp_path / "n.film")
    spt.write_film_file(path, sums, W, ROWS, SPP, 40, m2, BATCH, 5)
    data = open(path, "rb").read()
    assert data[:8] == b"SPTFILM2" and len(data) == 48 + 24 * W * ROWS + 48 * W * ROWS
    assert struct.unpack("<iiiiqiiq", data[8:48]) == (W, ROWS, SPP, 0, 40, BATCH, 0, 5)
    assert data[48:48 + 24 * W * ROWS] == sums.astype("<u8").tobytes()
    assert data[48 + 24 * W * ROWS:] == m2.astype("<u8").tobytes()
    s, m, info = spt.read_film_file(path, with_noise=True)
    assert np.array_equal(s, sums) and np.array_equal(m, m2) and m.shape == (ROWS, W, 3, 2)
    assert info == {"width": W, "rows": ROWS, "spp_total": SPP, "samples_done": 40, "batch": BATCH,
                    "batches_done": 5}
    with pytest.raises(spt.SptError):  # a reader that would drop the moments
        spt.read_film_file(path)


def test_plain_film_file_is_version_1_byte_for_byte(spt, tmp_path):
    sums, _, _, _ = synthetic(3)
    path = str(tmp_path / "p.film")
    spt.write_film_file(path, sums, W, ROWS, SPP, 23)
    want = struct.pack("<8siiiiq", b"SPTFILM1", W, ROWS, SPP, 0, 23) + sums.astype("<u8").tobytes()
    assert open(path, "rb").read() == want
    s, info = spt.read_film_file(path)
    assert np.array_equal(s, sums)
    assert info == {"width": W, "rows": ROWS, "spp_total": SPP, "samples_done": 23}
    s, m, info2 = spt.read_film_file(path, with_noise=True)
    assert m is None and info2 == info and np.array_equal(s, sums)


def test_truncated_and_mismatched_noise_files_are_refused(spt, tmp_path):
    sums, m2, _, _ = synthetic(5)
    path = str(tmp_path / "n.film")
    spt.write_film_file(path, sums, W, ROWS, SPP, 40, m2, BATCH, 5)
    good = open(path, "rb").read()

    def refused(data):
        bad = str(tmp_path / "bad.film")
        open(bad, "wb").write(data)
        with pytest.raises(spt.SptError):
            spt.read_film_file(bad, with_noise=True)

    refused(good[:-8])                                   # truncated moments
    refused(good[:40])                                   # truncated header
    refused(good + b"\0" * 8)                            # oversized
    refused(b"SPTFILM1" + good[8:])                      # a v1 magic over a v2 body
    refused(b"SPTFILM2" + good[8:32] + good[48:])        # a v2 magic over a v1 layout
    hdr = lambda **kw: struct.pack("<8siiiiqiiq", b"SPTFILM2", W, ROWS, SPP, 0, kw.get("done", 40),  # noqa: E731
                                   kw.get("batch", BATCH), 0, kw.get("bdone", 5))
    refused(hdr(batch=7) + good[48:])                    # a batch that does not divide spp
    refused(hdr(batch=SPP) + good[48:])                  # fewer than two batches
    refused(hdr(bdone=9) + good[48:])                    # more batches than spp holds
    refused(hdr(done=41) + good[48:])                    # samples that are no whole batches
    with pytest.raises(spt.SptError):                    # moments of the wrong size
        spt.write_film_file(path, sums, W, ROWS, SPP, 40, m2.reshape(-1)[:-2], BATCH, 5)
    s, m, _ = spt.read_film_file(str(tmp_path / "n.film"), with_noise=True)  # the good file still reads
    assert np.array_equal(m, m2)


def test_abi_version_stays_and_noise_is_announced(spt):
    assert spt.load_library().spt_abi_version() == 6
    hdr = open(os.path.join(ROOT, "include", "spt.h")).read()
    assert re.search(r"^#define SPT_ABI_VERSION 6\b", hdr, re.M)
    assert re.search(r"^#define SPT_HAS_FILM_NOISE 1\b", hdr, re.M)
    for name in ("spt_film_noise_enable", "spt_film_noise_info_get", "spt_film_noise_download",
                 "spt_film_noise_upload", "spt_film_noise_map", "spt_film_noise_summary",
                 "spt_film_noise_map_host", "spt_film_noise_summary_host"):
        assert name in spt.EXPORTS and hasattr(spt.load_library(), name)
    assert ctypes.sizeof(spt.spt_film_noise_info) == 16 and ctypes.sizeof(spt.spt_noise_summary) == 56

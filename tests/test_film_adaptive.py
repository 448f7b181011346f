"""The adaptive film's host side (no GPU): the four host statements against a statement in Python
integers on synthetic sums, moments and counts, and the ABI markers.

Statement (include/spt.h): pixel p holds B = counts[p] & 0x7FFFFFFF batches. Resolve:
min((float)S * 2^-31 [* r(B)], 1), r(B) = (float)(spp / (B * batch)), no factor iff B * batch == spp.
Error: D = B * M2 - S^2 in exact integers, d = (double)hi * 2^64 + (double)lo, se = (float)(sqrt(d) *
k(B)), k(B) = spp / (batch * 2^31 * B * sqrt(B - 1)); 0 where the resolved value is the clamp. The
selection keeps an active pixel iff keep allows it and (threshold < 0 or some channel has
d * k(B)^2 > threshold^2): the same IEEE double operations in C and in Python, so it is exact.
Tolerances (those of tests/test_film_noise.py for the same quantities): a float within relative 2^-21,
a summary figure within relative 1e-9; clamped channels and D = 0 exactly 0."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, ROWS, SPP, BATCH = 9, 7, 64, 8
B_MAX = SPP // BATCH
NPIX = W * ROWS
REL_F32 = 2.0 ** -21
REL_SUM = 1e-9
RETIRED, MASK = 0x80000000, 0x7FFFFFFF


def synthetic(seed=7):
    """Per pixel a count B (pixel 0..3 at B = 2, 4..7 at B_max, the rest from 2..B_max), and per
    element B batch sums P -> S, M2. Pixel 0 and 4: equal batches (D = 0); pixel 1 and 5: far above
    the clamp, batches near the bound batch * 2^31; pixel 2: all zero; the rest: dim values with a
    spread. The active pixels share the front B_max; every pixel below it is retired, and so are a
    few at B_max."""
    rng = np.random.default_rng(seed)
    top = BATCH << 31
    B = [int(v) for v in rng.integers(2, B_MAX + 1, size=NPIX)]
    B[0:4] = [2] * 4
    B[4:8] = [B_MAX] * 4
    B[8::2] = [B_MAX] * len(B[8::2])  # half of the rest at the front
    S, M = [], []
    for p in range(NPIX):
        for c in range(3):
            if p in (0, 4):
                P = [123456789 + c] * B[p]
            elif p in (1, 5):
                P = [int(v) for v in rng.integers(top // 2, top, size=B[p])]
            elif p == 2:
                P = [0] * B[p]
            else:
                P = [int(v) for v in rng.integers(0, top // 160, size=B[p])]
            S.append(sum(P))
            M.append(sum(v * v for v in P))
    counts = np.array(B, dtype=np.uint32)
    retired = np.array([b < B_MAX for b in B]) | (rng.random(NPIX) < 0.2)
    retired[4] = False
    retired[5] = False
    counts[retired] |= np.uint32(RETIRED)
    sums = np.array(S, dtype=np.uint64).reshape(ROWS, W, 3)
    m2 = np.array([[m & (2 ** 64 - 1), m >> 64] for m in M], dtype=np.uint64).reshape(ROWS, W, 3, 2)
    return sums, m2, counts.reshape(ROWS, W), S, M, B


def k_of(B):
    return SPP / (BATCH * 2.0 ** 31 * B * math.sqrt(B - 1)) if B >= 2 else 0.0


def resolve1(S, B):
    f = np.float32(S) * np.float32(2.0 ** -31)
    if B * BATCH != SPP:
        f = f * (np.float32(np.float64(SPP) / np.float64(B * BATCH)) if B else np.float32(0.0))
    return min(f, np.float32(1.0))


def statement(S, M, B):
    """-> per element: se (Python float), d * k2 exactly as the C computes it, clamped flag."""
    se, dk2, cl = [], [], []
    for e, (s, m) in enumerate(zip(S, M)):
        b = B[e // 3]
        D = b * m - s * s
        assert D >= 0
        clamp = bool(resolve1(s, b) == np.float32(1.0))
        k = k_of(b)
        d = 0.0 if clamp else float(D >> 64) * 2.0 ** 64 + float(D & (2 ** 64 - 1))
        se.append(0.0 if clamp else math.sqrt(D) * k)
        dk2.append(d * (k * k))
        cl.append(clamp)
    return se, dk2, cl


def test_resolve_host_is_the_numpy_restatement_bit_for_bit(spt):
    sums, m2, counts, S, M, B = synthetic()
    got = spt.film_adaptive_resolve_host(sums, counts, W, ROWS, SPP, BATCH)
    assert got.dtype == np.float32 and got.shape == (ROWS, W, 3)
    want = np.array([resolve1(s, B[e // 3]) for e, s in enumerate(S)], dtype=np.float32)
    assert np.array_equal(got.reshape(-1), want)
    assert (got.reshape(-1, 3)[1] == 1.0).all() and (got.reshape(-1, 3)[5] == 1.0).all()
    # a pixel at B_max takes no factor: the full film's resolve; one at B = 2 takes spp / (2 batch)
    full = spt.film_resolve_host(sums, W, ROWS, SPP, SPP).reshape(-1, 3)
    part = spt.film_resolve_host(sums, W, ROWS, SPP, 2 * BATCH).reshape(-1, 3)
    assert np.array_equal(got.reshape(-1, 3)[4:8], full[4:8])
    assert np.array_equal(got.reshape(-1, 3)[0:4], part[0:4])
    # a pixel without batches resolves to 0
    z = counts.copy()
    z.reshape(-1)[3] = 0
    assert not spt.film_adaptive_resolve_host(sums, z, W, ROWS, SPP, BATCH).reshape(-1, 3)[3].any()


def test_map_host_against_python_integers(spt):
    sums, m2, counts, S, M, B = synthetic()
    got = spt.film_adaptive_noise_map_host(sums, m2, counts, W, ROWS, SPP, BATCH).reshape(-1)
    want, _, cl = statement(S, M, B)
    assert all(cl[3:6]) and all(cl[15:18]) and not any(cl[0:3])
    for e in range(len(S)):
        if cl[e] or want[e] == 0.0:
            assert got[e] == 0.0, e
        else:
            assert abs(float(got[e]) - want[e]) <= REL_F32 * want[e], (e, got[e], want[e])
    assert not got[0:3].any() and not got[6:9].any() and not got[12:15].any()  # D = 0, zeros
    assert got[9:12].all()
    # pixels at B = 2 and at B_max agree with the uniform noise film's map at that depth
    u2 = spt.film_noise_map_host(sums, m2, W, ROWS, SPP, 2 * BATCH, BATCH, 2).reshape(-1)
    u8 = spt.film_noise_map_host(sums, m2, W, ROWS, SPP, SPP, BATCH, B_MAX).reshape(-1)
    assert np.array_equal(got[0:12], u2[0:12]) and np.array_equal(got[12:24], u8[12:24])


def test_summary_host_against_python_integers(spt):
    sums, m2, counts, S, M, B = synthetic()
    got = spt.film_adaptive_noise_summary_host(sums, m2, counts, W, ROWS, SPP, BATCH, B_MAX)
    se, dk2, cl = statement(S, M, B)
    for c in range(3):
        want = math.sqrt(math.fsum(dk2[c::3]) / NPIX)  # the mean over ALL pixels
        assert abs(got["rmse"][c] - want) <= REL_SUM * want, (c, got["rmse"][c], want)
    want = math.sqrt(math.fsum(dk2) / (3 * NPIX))
    assert abs(got["rmse_all"] - want) <= REL_SUM * want
    assert abs(got["se_max"] - max(se)) <= REL_F32 * max(se)
    assert got["clamped"] == sum(cl) and got["batches_done"] == B_MAX
    m = spt.film_adaptive_noise_map_host(sums, m2, counts, W, ROWS, SPP, BATCH)
    assert got["se_max"] == float(m.max())


def test_equal_counts_give_the_uniform_statements_bit_for_bit(spt):
    """With every count equal to B >= 2 each adaptive statement is the uniform one for batches_done =
    B, samples_done = B * batch: the resolve, the map and every field of the summary."""
    sums, m2, _, _, _, _ = synthetic()
    for B in (2, 5, B_MAX):
        counts = np.full((ROWS, W), B, dtype=np.uint32)
        counts.reshape(-1)[::3] |= np.uint32(RETIRED)  # the retired bit changes nothing
        done = B * BATCH
        assert spt.film_adaptive_resolve_host(sums, counts, W, ROWS, SPP, BATCH).tobytes() == \
            spt.film_resolve_host(sums, W, ROWS, SPP, done).tobytes()
        assert spt.film_adaptive_noise_map_host(sums, m2, counts, W, ROWS, SPP, BATCH).tobytes() == \
            spt.film_noise_map_host(sums, m2, W, ROWS, SPP, done, BATCH, B).tobytes()
        a = spt.film_adaptive_noise_summary_host(sums, m2, counts, W, ROWS, SPP, BATCH, B)
        u = spt.film_noise_summary_host(sums, m2, W, ROWS, SPP, done, BATCH, B)
        assert a == u and a["batches_done"] == B
        assert [x.hex() for x in a["rmse"] + [a["rmse_all"], a["se_max"]]] == \
            [x.hex() for x in u["rmse"] + [u["rmse_all"], u["se_max"]]]


def py_select(S, M, B, counts, threshold, keep):
    _, dk2, _ = statement(S, M, B)
    thr2 = threshold * threshold
    out, lst = counts.reshape(-1).copy(), []
    for p in range(NPIX):
        if out[p] & RETIRED:
            continue
        stay = keep is None or keep[p] != 0
        if stay and not threshold < 0:
            stay = any(dk2[3 * p + c] > thr2 for c in range(3))
        if stay:
            lst.append(p)
        else:
            out[p] |= np.uint32(RETIRED)
    return out, np.array(lst, dtype=np.uint32)


def test_select_host_is_exact(spt):
    sums, m2, counts, S, M, B = synthetic()
    se, _, _ = statement(S, M, B)
    active = [p for p in range(NPIX) if not counts.reshape(-1)[p] & RETIRED]
    assert len(active) > 8 and 4 in active and 5 in active
    act_se = sorted(max(se[3 * p:3 * p + 3]) for p in active)
    keep = (np.random.default_rng(3).random(NPIX) < 0.6).astype(np.uint8)
    cases = [(-1.0, None), (-1.0, keep), (act_se[len(act_se) // 2], None), (act_se[len(act_se) // 2], keep),
             (0.0, None), (act_se[-1] * 2.0, None)]
    for thr, kp in cases:
        got_c, got_l = spt.film_adaptive_select_host(sums, m2, counts, W, ROWS, SPP, BATCH, B_MAX, thr, kp)
        want_c, want_l = py_select(S, M, B, counts, thr, kp)
        assert np.array_equal(got_c.reshape(-1), want_c), (thr, kp is None)
        assert np.array_equal(got_l, want_l) and got_l.dtype == np.uint32
        assert np.all(np.diff(got_l.astype(np.int64)) > 0)
        # retired pixels stay retired, the batches never change
        assert np.array_equal(got_c.reshape(-1) & MASK, counts.reshape(-1) & MASK)
        assert np.all((got_c.reshape(-1) & RETIRED) >= (counts.reshape(-1) & RETIRED))
    all_c, all_l = spt.film_adaptive_select_host(sums, m2, counts, W, ROWS, SPP, BATCH, B_MAX, -1.0)
    assert np.array_equal(all_c, counts) and list(all_l) == active
    # threshold 0 retires exactly the pixels with d = 0 in all channels (D = 0, or clamped): 4 and 5
    _, zero_l = spt.film_adaptive_select_host(sums, m2, counts, W, ROWS, SPP, BATCH, B_MAX, 0.0)
    assert sorted(set(active) - set(int(v) for v in zero_l)) == [4, 5]
    _, none_l = spt.film_adaptive_select_host(sums, m2, counts, W, ROWS, SPP, BATCH, B_MAX,
                                              act_se[-1] * 2.0)
    assert none_l.size == 0


def test_host_statements_reject_bad_arguments(spt):
    sums, m2, counts, _, _, _ = synthetic()
    with pytest.raises(spt.SptError) as e:  # NaN threshold
        spt.film_adaptive_select_host(sums, m2, counts, W, ROWS, SPP, BATCH, B_MAX, float("nan"))
    assert e.value.status == 1
    with pytest.raises(spt.SptError) as e:  # a selection before two batches
        spt.film_adaptive_select_host(sums, m2, counts, W, ROWS, SPP, BATCH, 1, 0.5)
    assert e.value.status == 1
    bad = counts.copy()
    bad.reshape(-1)[9] = B_MAX + 1
    with pytest.raises(spt.SptError) as e:  # a count the film cannot hold
        spt.film_adaptive_resolve_host(sums, bad, W, ROWS, SPP, BATCH)
    assert e.value.status == 1
    with pytest.raises(spt.SptError) as e:  # more than 4096 batches
        spt.film_adaptive_resolve_host(sums, counts, W, ROWS, 8192, 1)
    assert e.value.status == 1
    with pytest.raises(spt.SptError) as e:  # a batch that does not divide spp
        spt.film_adaptive_noise_map_host(sums, m2, counts, W, ROWS, SPP, 7)
    assert e.value.status == 1
    lib = spt.load_library()
    info, noise = spt.spt_film_info(W, ROWS, SPP, SPP), spt.spt_film_noise_info(1, BATCH, B_MAX)
    out = np.zeros(3 * NPIX, np.float32)
    a, c = np.ascontiguousarray(sums), np.ascontiguousarray(counts)
    I, N = ctypes.byref(info), ctypes.byref(noise)
    assert lib.spt_film_adaptive_resolve_host(a.ctypes.data, c.ctypes.data, I, N, out.ctypes.data) == 0
    assert lib.spt_film_adaptive_resolve_host(None, c.ctypes.data, I, N, out.ctypes.data) == 1
    assert lib.spt_film_adaptive_resolve_host(a.ctypes.data, None, I, N, out.ctypes.data) == 1
    assert lib.spt_film_adaptive_resolve_host(a.ctypes.data, c.ctypes.data, I, N, None) == 1
    assert lib.spt_film_adaptive_resolve_host(a.ctypes.data, c.ctypes.data, None, N, out.ctypes.data) == 1
    plain = spt.spt_film_noise_info(0, 0, 0)
    assert lib.spt_film_adaptive_resolve_host(a.ctypes.data, c.ctypes.data, I, ctypes.byref(plain),
                                              out.ctypes.data) == 1


def test_abi_version_stays_and_adaptive_is_announced(spt):
    lib = spt.load_library()
    assert lib.spt_abi_version() == 6
    hdr = open(os.path.join(ROOT, "include", "spt.h")).read()
    assert re.search(r"^#define SPT_ABI_VERSION 6\b", hdr, re.M)
    assert re.search(r"^#define SPT_HAS_FILM_ADAPTIVE 1\b", hdr, re.M)
    sig = {"spt_film_adaptive_enable": 1, "spt_film_adaptive_info_get": 2, "spt_film_adaptive_select": 5,
           "spt_film_adaptive_download": 3, "spt_film_adaptive_upload": 3,
           "spt_film_adaptive_resolve_host": 5, "spt_film_adaptive_noise_map_host": 6,
           "spt_film_adaptive_noise_summary_host": 6, "spt_film_adaptive_select_host": 10}
    for name, n_args in sig.items():
        assert name in spt.EXPORTS and hasattr(lib, name)
        fn = getattr(lib, name)
        assert len(fn.argtypes) == n_args and fn.restype is ctypes.c_int32, name
        decl = re.search(r"spt_status\s+%s\(([^;]*)\);" % name, hdr)
        assert decl and decl.group(1).count(",") + 1 == n_args, name
    assert lib.spt_film_adaptive_select.argtypes[1] is ctypes.c_double
    assert lib.spt_film_adaptive_select_host.argtypes[5] is ctypes.c_double
    assert ctypes.sizeof(spt.spt_film_adaptive_info) == 32
    assert [f for f, _ in spt.spt_film_adaptive_info._fields_] == ["enabled", "reserved", "front",
                                                                   "n_active", "samples_total"]
    assert spt.COUNT_RETIRED == 1 << 31 and spt.COUNT_MASK == (1 << 31) - 1
    # the existing structs and markers are untouched
    assert re.search(r"^#define SPT_HAS_FILM_NOISE 1\b", hdr, re.M)
    assert ctypes.sizeof(spt.spt_film_noise_info) == 16 and ctypes.sizeof(spt.spt_noise_summary) == 56

"""The pooled error's host side (no GPU): spt_film_noise_pool_map_host and
spt_film_adaptive_select_pooled_host against a statement in plain Python floats, and the ABI markers.

Statement (include/spt.h, SPT_HAS_FILM_POOL). Pixel q holds B_q = counts[q] & 0x7FFFFFFF batches;
u(q,c) = (d * k2(B_q)) * B_q with d and k2 of the error map (d = 0 for a clamped channel), 0 and not
counted where B_q < 2. The window of (y, x) with radius R: columns max(0, x-R) .. min(w-1, x+R), rows
y-R .. y+R clipped to the film and to the pixel's band of band_rows rows. h = 0.0 + u over the columns
ascending, g = 0.0 + h over the rows ascending, n = the window's counted pixels; with
SPT_POOL_EXCLUDE_CENTER g = g - u(y,x,c) and n = n - 1 if B_p >= 2. Map: (float)sqrt(g / (n * B_p)), 0
where n == 0 or B_p < 2. Selection: an active pixel stays iff keep allows it and (threshold < 0 or some
channel has g > (thr2 * n) * B_p); where n == 0 its own rule d * k2 > thr2 decides.

Python floats are IEEE doubles, never contracted, and the statement adds in the stated order, so the
selection is compared exactly; the map within relative 2^-21 (one float rounding and the square root,
the tolerance of tests/test_film_noise.py for the same kind of quantity), exactly 0 where the
statement says 0."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, ROWS, SPP, BATCH = 9, 7, 64, 8
B_MAX = SPP // BATCH
REL_F32 = 2.0 ** -21
RETIRED, MASK = 0x80000000, 0x7FFFFFFF
EXCLUDE = 1


def synthetic(w=W, rows=ROWS, seed=10, special=True, uniform=None):
    """Planes of tests/test_film_adaptive.py's kind. Per pixel a count B and per element B batch sums
    P -> S, M2 (Python integers). The active pixels share the front B_MAX; every pixel below it is
    retired, and so are a few at B_MAX. With `special` (needs >= 12 pixels): pixel 0 and 4 have equal
    batches (D = 0), 1 and 5 lie far above the clamp, 2 is all zero, and pixel 3 is retired with an
    uploaded count of 1 (it holds no error estimate and is not counted in any n). uniform = b: every
    pixel holds b batches and none is retired (a uniform noise film after b batches).
    The seed: with R = 16 and bands a window is a whole band, the active pixels of a band share one
    pooled se, and the median rule splits the film by whole bands; seed 10 is one whose bands
    fall so that the Python statement alone retires 20-80 % in every case where it can."""
    rng = np.random.default_rng(seed)
    npix = w * rows
    top = BATCH << 31
    B = [int(v) for v in rng.integers(2, B_MAX + 1, size=npix)]
    if special:
        B[0:4] = [2, 2, 2, 1]
        B[4:8] = [B_MAX] * 4
    B[8::2] = [B_MAX] * len(B[8::2])  # half of the rest at the front
    if uniform is not None:
        B = [uniform] * npix
    S, M = [], []
    for p in range(npix):
        for c in range(3):
            if special and p in (0, 4):
                P = [123456789 + c] * B[p]
            elif special and p in (1, 5):
                P = [int(v) for v in rng.integers(top // 2, top, size=B[p])]
            elif special and p == 2:
                P = [0] * B[p]
            else:
                P = [int(v) for v in rng.integers(0, top // 160, size=B[p])]
            S.append(sum(P))
            M.append(sum(v * v for v in P))
    counts = np.array(B, dtype=np.uint32)
    retired = np.array([b < B_MAX for b in B]) | (rng.random(npix) < 0.2)
    if special:
        retired[4] = retired[5] = False
    if uniform is not None:
        retired[:] = False
    counts[retired] |= np.uint32(RETIRED)
    sums = np.array(S, dtype=np.uint64).reshape(rows, w, 3)
    m2 = np.array([[m & (2 ** 64 - 1), m >> 64] for m in M], dtype=np.uint64).reshape(rows, w, 3, 2)
    return sums, m2, counts.reshape(rows, w), S, M, B


def k_of(B):
    return SPP / (BATCH * 2.0 ** 31 * B * math.sqrt(B - 1)) if B >= 2 else 0.0


def resolve1(S, B, done=None):
    """The resolve's value of a pixel at B batches (done: a uniform film's samples_done)."""
    done = B * BATCH if done is None else done
    f = np.float32(S) * np.float32(2.0 ** -31)
    if done != SPP:
        f = f * (np.float32(np.float64(SPP) / np.float64(done)) if done else np.float32(0.0))
    return min(f, np.float32(1.0))


def d_of(s, m, b):
    """The error map's d: the exact integer D = B * M2 - S^2 as hi * 2^64 + lo in double; 0 clamped."""
    if resolve1(s, b) == np.float32(1.0):
        return 0.0
    D = b * m - s * s
    assert D >= 0
    return float(D >> 64) * 2.0 ** 64 + float(D & (2 ** 64 - 1))


def u_of(S, M, B):
    """-> u per element, counted per pixel."""
    u = []
    for e, (s, m) in enumerate(zip(S, M)):
        b = B[e // 3]
        k = k_of(b)
        u.append((d_of(s, m, b) * (k * k)) * float(b) if b >= 2 else 0.0)
    return u, [1 if b >= 2 else 0 for b in B]


def window(u, counted, B, w, rows, band_rows, R, flags, y, x):
    """-> g[3], n of pixel (y, x): the stated sums in the stated order."""
    x0, x1 = max(0, x - R), min(w - 1, x + R)
    b0, b1 = 0, rows
    if band_rows > 0:
        b0 = y - y % band_rows
        b1 = min(rows, b0 + band_rows)
    y0, y1 = max(b0, y - R), min(b1 - 1, y + R)
    g, n = [0.0, 0.0, 0.0], 0
    for yy in range(y0, y1 + 1):
        h = [0.0, 0.0, 0.0]
        for xx in range(x0, x1 + 1):
            q = yy * w + xx
            for c in range(3):
                h[c] = h[c] + u[3 * q + c]
            n += counted[q]
        for c in range(3):
            g[c] = g[c] + h[c]
    p = y * w + x
    if flags & EXCLUDE:
        for c in range(3):
            g[c] = g[c] - u[3 * p + c]
        if B[p] >= 2:
            n -= 1
    return g, n


def py_map(S, M, B, w, rows, band_rows, R, flags):
    u, counted = u_of(S, M, B)
    out = []
    for p in range(w * rows):
        g, n = window(u, counted, B, w, rows, band_rows, R, flags, p // w, p % w)
        for c in range(3):
            out.append(0.0 if n == 0 or B[p] < 2 else math.sqrt(g[c] / (float(n) * float(B[p]))))
    return out


def py_select(S, M, B, counts, w, rows, band_rows, R, flags, threshold, keep):
    u, counted = u_of(S, M, B)
    thr2 = threshold * threshold
    out, lst = counts.reshape(-1).copy(), []
    for p in range(w * rows):
        if out[p] & RETIRED:
            continue
        stay = keep is None or keep[p] != 0
        if stay and not threshold < 0:
            g, n = window(u, counted, B, w, rows, band_rows, R, flags, p // w, p % w)
            if n:
                t = (thr2 * float(n)) * float(B[p])
                stay = any(g[c] > t for c in range(3))
            else:  # nothing to pool: the pixel's own rule
                k = k_of(B[p])
                stay = any(d_of(S[3 * p + c], M[3 * p + c], B[p]) * (k * k) > thr2 for c in range(3))
        if stay:
            lst.append(p)
        else:
            out[p] |= np.uint32(RETIRED)
    return out, np.array(lst, dtype=np.uint32)


def check_map(got, want):
    got = got.reshape(-1)
    assert got.dtype == np.float32 and got.size == len(want)
    for e, v in enumerate(want):
        if v == 0.0:
            assert got[e] == 0.0, e
        else:
            assert abs(float(got[e]) - v) <= REL_F32 * v, (e, got[e], v)


@pytest.fixture(scope="module")
def planes():
    return synthetic()


CASES = [(R, band, flags) for R in (1, 2, 16) for band in (0, 3) for flags in (0, EXCLUDE)]


@pytest.mark.parametrize("R,band,flags", CASES)
def test_map_host_against_python_floats(spt, planes, R, band, flags):
    sums, m2, counts, S, M, B = planes
    got = spt.film_noise_pool_map_host(sums, m2, counts, W, ROWS, SPP, BATCH, B_MAX, R, bool(flags), band)
    assert got.shape == (ROWS, W, 3)
    want = py_map(S, M, B, W, ROWS, band, R, flags)
    check_map(got, want)
    assert not got.reshape(-1, 3)[3].any()  # the pixel at count 1 has no error of its own to scale
    assert sum(v > 0 for v in want) > len(want) // 2
    if R == 16 and band == 0 and not flags:  # the window is the whole film: one g, n for every pixel
        u, counted = u_of(S, M, B)
        _, n = window(u, counted, B, W, ROWS, 0, 16, 0, 3, 4)
        assert n == W * ROWS - 1  # pixel 3 is not counted


@pytest.mark.parametrize("R,band,flags", [(1, 0, 0), (2, 3, EXCLUDE), (16, 0, EXCLUDE)])
def test_map_host_on_a_uniform_film(spt, R, band, flags):
    """counts = NULL: every pixel holds batches_done batches, the clamp rule takes samples_done =
    batches_done * batch; with every count equal the adaptive statement returns the same bits."""
    for b in (2, 5, B_MAX):
        sums, m2, counts, S, M, B = synthetic(uniform=b)
        assert B == [b] * (W * ROWS)
        got = spt.film_noise_pool_map_host(sums, m2, None, W, ROWS, SPP, BATCH, b, R, bool(flags), band)
        check_map(got, py_map(S, M, B, W, ROWS, band, R, flags))
        same = spt.film_noise_pool_map_host(sums, m2, counts, W, ROWS, SPP, BATCH, b, R, bool(flags), band)
        assert same.tobytes() == got.tobytes()


def median_threshold(S, M, B, counts, w, rows, band, R, flags):
    """The median over the active pixels of the statement's pooled se (largest channel)."""
    se = py_map(S, M, B, w, rows, band, R, flags)
    act = [p for p in range(w * rows) if not counts.reshape(-1)[p] & RETIRED]
    return sorted(max(se[3 * p:3 * p + 3]) for p in act)[len(act) // 2], act


@pytest.mark.parametrize("R,band,flags", CASES)
def test_select_host_is_exact(spt, planes, R, band, flags):
    sums, m2, counts, S, M, B = planes
    thr, act = median_threshold(S, M, B, counts, W, ROWS, band, R, flags)
    assert thr > 0 and len(act) > 8
    keep = (np.random.default_rng(3).random(W * ROWS) < 0.6).astype(np.uint8)
    for t, kp in [(thr, None), (thr, keep), (-1.0, None), (-1.0, keep), (0.0, None)]:
        want_c, want_l = py_select(S, M, B, counts, W, ROWS, band, R, flags, t, kp)
        if t == thr and kp is None:  # not vacuous: the statement alone retires 20-80 % of the active
            gone = len(act) - want_l.size
            if R == 16 and band == 0 and not flags:
                # one window, the whole film, for every pixel: the active ones (one count, the front)
                # share one pooled se, the median is that value and no threshold can split them
                assert gone in (0, len(act))
            else:
                assert 0.2 * len(act) <= gone <= 0.8 * len(act), (len(act), gone)
        got_c, got_l = spt.film_adaptive_select_pooled_host(sums, m2, counts, W, ROWS, SPP, BATCH, B_MAX, t,
                                                            R, bool(flags), kp, band)
        assert np.array_equal(got_c.reshape(-1), want_c), (t, kp is None)
        assert np.array_equal(got_l, want_l) and got_l.dtype == np.uint32
        assert np.array_equal(got_c.reshape(-1) & MASK, counts.reshape(-1) & MASK)
        assert np.all((got_c.reshape(-1) & RETIRED) >= (counts.reshape(-1) & RETIRED))
    # threshold < 0 looks at no error: the unpooled statement's answer
    c0, l0 = spt.film_adaptive_select_host(sums, m2, counts, W, ROWS, SPP, BATCH, B_MAX, -1.0, keep)
    c1, l1 = spt.film_adaptive_select_pooled_host(sums, m2, counts, W, ROWS, SPP, BATCH, B_MAX, -1.0, R,
                                                  bool(flags), keep, band)
    assert np.array_equal(c0, c1) and np.array_equal(l0, l1)


def test_one_pixel_film_falls_back_to_its_own_rule(spt):
    """1x1 with the centre excluded: n == 0, the map reads 0 and the pixel's own rule decides."""
    top = BATCH << 31
    P = [[top // 300, top // 200, top // 250, top // 220, top // 260, top // 210, top // 240, top // 230],
         [top // 310] * 8, [top // 400, top // 100] * 4]
    S = [sum(p) for p in P]
    M = [sum(v * v for v in p) for p in P]
    B = [B_MAX]
    sums = np.array(S, dtype=np.uint64).reshape(1, 1, 3)
    m2 = np.array([[m & (2 ** 64 - 1), m >> 64] for m in M], dtype=np.uint64).reshape(1, 1, 3, 2)
    counts = np.array([[B_MAX]], dtype=np.uint32)
    assert not spt.film_noise_pool_map_host(sums, m2, counts, 1, 1, SPP, BATCH, B_MAX, 1, True).any()
    inc = spt.film_noise_pool_map_host(sums, m2, counts, 1, 1, SPP, BATCH, B_MAX, 1, False)
    own = spt.film_adaptive_noise_map_host(sums, m2, counts, 1, 1, SPP, BATCH)
    check_map(inc, py_map(S, M, B, 1, 1, 0, 1, 0))
    assert np.all(np.abs(inc.astype(np.float64) - own) <= 4 * REL_F32 * own)  # a window of one pixel
    se = float(own.max())
    assert se > 0
    for t in (0.5 * se, 2.0 * se):
        for flags in (0, EXCLUDE):
            want_c, want_l = py_select(S, M, B, counts, 1, 1, 0, 1, flags, t, None)
            assert want_l.size == (1 if t < se else 0)
            got_c, got_l = spt.film_adaptive_select_pooled_host(sums, m2, counts, 1, 1, SPP, BATCH, B_MAX, t,
                                                                1, bool(flags))
            assert np.array_equal(got_c.reshape(-1), want_c) and np.array_equal(got_l, want_l)


def test_a_count_of_one_is_not_counted(spt, planes):
    sums, m2, counts, S, M, B = planes
    assert B[3] == 1 and counts.reshape(-1)[3] == (1 | RETIRED)
    u, counted = u_of(S, M, B)
    assert counted[3] == 0 and u[9:12] == [0.0, 0.0, 0.0]
    _, n = window(u, counted, B, W, ROWS, 0, 1, 0, 0, 3)
    assert n == 5  # a 2x3 border window around (0, 3) without the pixel itself
    _, n = window(u, counted, B, W, ROWS, 0, 1, EXCLUDE, 0, 3)
    assert n == 5  # ... and the excluded centre was never in n
    # at count 2 it would be counted: the neighbours' pooled error changes
    two = counts.copy()
    two.reshape(-1)[3] = 2 | RETIRED
    a = spt.film_noise_pool_map_host(sums, m2, counts, W, ROWS, SPP, BATCH, B_MAX, 1)
    b = spt.film_noise_pool_map_host(sums, m2, two, W, ROWS, SPP, BATCH, B_MAX, 1)
    assert a[0, 4, 2] != b[0, 4, 2] and np.array_equal(a[3:], b[3:])


def test_rejections(spt, planes):
    sums, m2, counts, _, _, _ = planes

    def refused(call):
        with pytest.raises(spt.SptError) as e:
            call()
        assert e.value.status == 1

    sel, mp = spt.film_adaptive_select_pooled_host, spt.film_noise_pool_map_host
    for R in (0, -1, 17):
        refused(lambda: sel(sums, m2, counts, W, ROWS, SPP, BATCH, B_MAX, 0.5, R))
        refused(lambda: mp(sums, m2, counts, W, ROWS, SPP, BATCH, B_MAX, R))
    refused(lambda: sel(sums, m2, counts, W, ROWS, SPP, BATCH, B_MAX, float("nan"), 2))
    refused(lambda: sel(sums, m2, counts, W, ROWS, SPP, BATCH, 1, 0.5, 2))       # front < 2
    refused(lambda: mp(sums, m2, None, W, ROWS, SPP, BATCH, 1, 2))               # one batch
    refused(lambda: sel(sums, m2, counts, W, ROWS, SPP, BATCH, B_MAX, 0.5, 2, band_rows=-1))
    refused(lambda: mp(sums, m2, counts, W, ROWS, SPP, BATCH, B_MAX, 2, band_rows=-1))
    bad = counts.copy()
    bad.reshape(-1)[9] = B_MAX + 1
    refused(lambda: mp(sums, m2, bad, W, ROWS, SPP, BATCH, B_MAX, 2))
    refused(lambda: sel(sums, m2, bad, W, ROWS, SPP, BATCH, B_MAX, 0.5, 2))
    lib = spt.load_library()
    info, noise = spt.spt_film_info(W, ROWS, SPP, SPP), spt.spt_film_noise_info(1, BATCH, B_MAX)
    I, N = ctypes.byref(info), ctypes.byref(noise)
    a, m, c = np.ascontiguousarray(sums), np.ascontiguousarray(m2), np.ascontiguousarray(counts)
    out = np.zeros(3 * W * ROWS, np.float32)
    co, lo, n = np.zeros(W * ROWS, np.uint32), np.zeros(W * ROWS, np.uint32), ctypes.c_int64(-5)
    A, Mp, C = a.ctypes.data, m.ctypes.data, c.ctypes.data
    assert lib.spt_film_noise_pool_map_host(A, Mp, C, I, N, 0, 2, 0, out.ctypes.data) == 0
    assert lib.spt_film_noise_pool_map_host(A, Mp, C, I, N, 0, 2, 2, out.ctypes.data) == 1  # a flag bit
    assert lib.spt_film_noise_pool_map_host(A, Mp, C, I, N, 0, 2, 0x80000001, out.ctypes.data) == 1
    assert lib.spt_film_noise_pool_map_host(None, Mp, C, I, N, 0, 2, 0, out.ctypes.data) == 1
    assert lib.spt_film_noise_pool_map_host(A, Mp, C, I, N, 0, 2, 0, None) == 1
    args = (A, Mp, C, I, N, 0, 0.5, 2)
    tail = (None, co.ctypes.data, lo.ctypes.data, ctypes.byref(n))
    assert lib.spt_film_adaptive_select_pooled_host(*args, 0, *tail) == 0 and n.value >= 0
    n.value = -5
    assert lib.spt_film_adaptive_select_pooled_host(*args, 2, *tail) == 1 and n.value == -5
    assert lib.spt_film_adaptive_select_pooled_host(*args, 1, None, None, lo.ctypes.data, ctypes.byref(n)) == 1
    assert lib.spt_film_adaptive_select_pooled_host(*args, 1, None, co.ctypes.data, lo.ctypes.data, None) == 1
    # a film without rows: nothing to do
    e_info = spt.spt_film_info(W, 0, SPP, SPP)
    assert lib.spt_film_adaptive_select_pooled_host(None, None, None, ctypes.byref(e_info), N, 0, 0.5, 2, 0,
                                                    None, None, None, ctypes.byref(n)) == 0
    assert n.value == 0


def test_abi_version_stays_and_the_pool_is_announced(spt):
    lib = spt.load_library()
    assert lib.spt_abi_version() == 6
    hdr = open(os.path.join(ROOT, "include", "spt.h")).read()
    assert re.search(r"^#define SPT_ABI_VERSION 6\b", hdr, re.M)
    assert re.search(r"^#define SPT_HAS_FILM_POOL 1\b", hdr, re.M)
    assert re.search(r"^#define SPT_POOL_MAX_RADIUS 16\b", hdr, re.M)
    assert re.search(r"^#define SPT_POOL_EXCLUDE_CENTER 1u\b", hdr, re.M)
    assert "SPT_HAS_FILM_POOL" in hdr[:hdr.index("#define SPT_HAS_FILM 1")]  # the version comment
    sig = {"spt_film_noise_pool_map": 5, "spt_film_adaptive_select_pooled": 7,
           "spt_film_noise_pool_map_host": 9, "spt_film_adaptive_select_pooled_host": 13}
    for name, n_args in sig.items():
        assert name in spt.EXPORTS and hasattr(lib, name)
        fn = getattr(lib, name)
        assert len(fn.argtypes) == n_args and fn.restype is ctypes.c_int32, name
        decl = re.search(r"spt_status\s+%s\(([^;]*)\);" % name, hdr)
        assert decl and decl.group(1).count(",") + 1 == n_args, name
    assert lib.spt_film_adaptive_select_pooled.argtypes[1] is ctypes.c_double
    assert lib.spt_film_adaptive_select_pooled_host.argtypes[6] is ctypes.c_double
    assert spt.POOL_MAX_RADIUS == 16 and spt.POOL_EXCLUDE_CENTER == 1
    # the earlier markers and structs are untouched
    for marker in ("SPT_HAS_FILM", "SPT_HAS_FILM_NOISE", "SPT_HAS_FILM_ADAPTIVE"):
        assert re.search(r"^#define %s 1\b" % marker, hdr, re.M)
    assert ctypes.sizeof(spt.spt_film_adaptive_info) == 32 and ctypes.sizeof(spt.spt_noise_summary) == 56

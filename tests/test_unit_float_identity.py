"""A random word's unit-interval float as one funnel shift (spt_device.h, funnel_float): the shift and
the or, (K << 23) | (v >> 9), are the low 32 bits of the 64-bit word {K, v} shifted right by 9, which
is what v_alignbit_b32(K, v, 9) returns. K = 0x7F gives u01's float 1 + m 2^-23, K = 0x96 the light
lattice's 2^23 + m, m = v >> 9: the two constants are pinned here, on the CPU."""
import numpy as np
import pytest

KS = {0x7F: "one", 0x96: "two_pow_23"}


def words():
    edge = [0, 1, 0x1FF, 0x200, 0xFFFFFFFF] + [1 << b for b in range(32)]
    rnd = np.random.default_rng(30).integers(0, 1 << 32, size=1 << 16, dtype=np.uint64)
    return np.concatenate([np.array(edge, dtype=np.uint64), rnd])


@pytest.mark.parametrize("k", list(KS))
def test_funnel_shift_is_the_shift_and_the_or(k):
    v = words()
    assert v.size == 5 + 32 + (1 << 16)
    pair = (np.uint64(k) << np.uint64(23)) | (v >> np.uint64(9))
    funnel = (((np.uint64(k) << np.uint64(32)) | v) >> np.uint64(9)) & np.uint64(0xFFFFFFFF)
    assert np.array_equal(pair, funnel)
    assert int(pair.max()) < 1 << 32


@pytest.mark.parametrize("k", list(KS))
def test_the_floats(k):
    v = words()
    bits = ((np.uint64(k) << np.uint64(23)) | (v >> np.uint64(9))).astype(np.uint32)
    f = bits.view(np.float32).astype(np.float64)
    m = (v >> np.uint64(9)).astype(np.float64)
    want = 1.0 + m * 2.0 ** -23 if k == 0x7F else 2.0 ** 23 + m
    assert np.array_equal(f, want)
    if k == 0x7F:  # u01 itself: [0, 1), the subtraction exact
        u = (bits.view(np.float32) - np.float32(1.0)).astype(np.float64)
        assert np.array_equal(u, m * 2.0 ** -23) and u.min() == 0.0 and u.max() < 1.0


def test_the_constants_are_the_kernels():
    assert 0x7F << 23 == 0x3F800000 and 0x96 << 23 == 0x4B000000
    assert np.array([0x3F800000, 0x4B000000], dtype=np.uint32).view(np.float32).tolist() == [1.0, 2.0 ** 23]

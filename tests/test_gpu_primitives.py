"""The device building blocks of spt_device.h, run directly on the GPU through the probe library
(tests/probe/spt_probe.hip, built by __graft_entry__.build() with the render kernel's HIPFLAGS) and
compared word for word with the oracle's spt_oracle_map.

tests/test_contract_math.py holds that C to the fp64 truth; bitwise equality here carries its bounds
over to the device. Every non-NaN result must have the oracle's bits and NaN must meet NaN. A NaN's
sign and payload are not part of the contract (x86 makes 0xFFC00000 where the device may make
0x7FC00000): the intersection may only rely on it being a NaN (tests/test_gpu_rays.py).
"""
import ctypes
import os

import numpy as np
import pytest

import contract_truth as ct
import test_contract_math as tcm
import test_oracle as to

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PROBE = os.path.join(HERE, "probe", "libspt_probe.so")
NAMES = ["rcp_nr", "rsq_nr", "rsq_nr1", "rsq_nr2", "u01", "u16i", "u16", "jitter_f", "disk_dir",
         "cosine_axis", "cosine_general", "fix31", "philox4x32", "philox_px", "normalize3",
         "normalize3_free"]


@pytest.fixture(scope="module")
def probe(spt):
    """run(name, words (n, wi) uint32, wo) -> (n, wo) uint32: one launch of the probe's kernel."""
    import torch  # the package loaded torch's HIP runtime first; the probe binds to the same one

    assert os.path.exists(PROBE), f"{PROBE} not built: run __graft_entry__.build()"
    lib = ctypes.CDLL(PROBE)
    for name in NAMES:
        fn = getattr(lib, "spt_probe_" + name)  # a missing launcher is an error
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]
        fn.restype = ctypes.c_int

    def run(name, words, wo):
        a = np.ascontiguousarray(words, dtype=np.uint32)
        a = a.reshape(len(a), -1)
        n = len(a)
        src = torch.from_numpy(a.view(np.int32)).to("cuda:0")
        dst = torch.zeros((n, wo), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream().cuda_stream
        rc = getattr(lib, "spt_probe_" + name)(src.data_ptr(), dst.data_ptr(), n, stream)
        assert rc == 0, f"spt_probe_{name}: hip error {rc}"
        return dst.cpu().numpy().view(np.uint32)

    return run


def _is_nan(words):
    return np.isnan(words.view(np.float32))


def _assert_same_floats(got, want, what):
    """Bitwise equal wherever the oracle's result is not a NaN; NaN exactly where it is."""
    gn, wn = _is_nan(got), _is_nan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN at other inputs, first {np.argwhere(gn != wn)[:5].tolist()}"
    bad = np.argwhere((got != want) & ~wn)
    assert bad.size == 0, (f"{what}: {len(bad)} words differ, first {bad[:5].tolist()}: "
                           f"{[(hex(int(got[tuple(b)])), hex(int(want[tuple(b)]))) for b in bad[:5]]}")


def _f32_inputs():
    """The sweeps of test_contract_math: [1, 4) exhaustively, both signs, the log-uniform samples
    and the specials."""
    sw = ct.binade_sweep()
    return np.concatenate([sw, -sw[::257], ct.log_uniform(10 ** 6, -125, 128, seed=12),
                           -ct.log_uniform(10 ** 5, -125, 125, seed=11), ct.SPECIALS,
                           ct.log_uniform(10 ** 4, -149, -125, seed=14)])


@pytest.mark.parametrize("name", ["rcp_nr", "rsq_nr", "rsq_nr1", "rsq_nr2"])
def test_reciprocals_bit_exact(probe, oracle, name):
    x = _f32_inputs().view(np.uint32)
    if name == "rcp_nr":
        x = np.concatenate([x, (-ct.binade_sweep()).view(np.uint32)])
    _assert_same_floats(probe(name, x, 1), oracle.map_words(name, x), name)


def test_rcp_nr_of_zero_is_a_nan_on_the_device(probe, oracle):
    """The one thing the intersection needs of rcp_nr(+-0). The bit patterns are printed for
    DESIGN.md section 3; the host's is 0xFFC00000 (x86's default NaN) for both zeros."""
    z = np.array([0.0, -0.0], dtype=np.float32).view(np.uint32)
    dev, host = probe("rcp_nr", z, 1)[:, 0], oracle.map_words("rcp_nr", z)[:, 0]
    print(f"rcp_nr(+0), rcp_nr(-0): device {hex(int(dev[0]))} {hex(int(dev[1]))}, "
          f"host {hex(int(host[0]))} {hex(int(host[1]))}")
    assert _is_nan(dev).all() and _is_nan(host).all()


def test_u01_u16_jitter_bit_exact(probe, oracle):
    rng = np.random.default_rng(31)
    v = np.concatenate([rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32),
                        np.array([0, 1, 0x1FF, 0x200, 0xFFFFFFFF, 0xFFFFFE00, 0xFF, 0xFF00],
                                 dtype=np.uint32)])
    assert np.array_equal(probe("u01", v, 1), oracle.map_words("u01", v))
    pair = np.stack([v, v[::-1]], axis=1)
    assert np.array_equal(probe("u16i", pair, 1), oracle.map_words("u16i", pair))
    assert np.array_equal(probe("u16", pair, 1), oracle.map_words("u16", pair))
    assert np.array_equal(probe("jitter_f", pair, 1), oracle.map_words("jitter", pair))
    # every 16-bit draw once, in the bytes the permute picks, whatever the other bytes hold
    j = np.arange(1 << 16, dtype=np.uint32)
    pair = np.stack([(j & np.uint32(0xFF)) | np.uint32(0xABCDEF00), (j >> np.uint32(8)) | np.uint32(0x12345600)],
                    axis=1)
    assert np.array_equal(probe("u16i", pair, 1)[:, 0], j)


def test_disk_dir_every_angle_bit_exact(probe, oracle):
    ra = ct.disk_words()
    got = probe("disk_dir", ra, 2)
    assert np.array_equal(got, oracle.map_words("disk_dir", ra))
    assert int((got.view(np.float32) == 0).sum()) == 8
    lo = ra[::4099] | np.uint32(0xFF)  # the low byte is not read
    assert np.array_equal(probe("disk_dir", lo, 2), oracle.map_words("disk_dir", lo))


@pytest.mark.parametrize("unit", [True, False], ids=["unit", "free"])
@pytest.mark.parametrize("uniform", [False, True], ids=["cosine", "uniform"])
def test_cosine_vec_bit_exact(probe, oracle, uniform, unit):
    """cosine_vec<true> (axis normals), cosine_vec<false> (its per-lane test on axis normals, and
    the general frame), each followed by the kernel's normalize, against c_cosine."""
    ra, rb = ct.cosine_words(10 ** 5, seed=21)
    mode = int(uniform) | (int(unit) << 1)

    def words(nl):
        w = np.empty((len(ra), 6), dtype=np.uint32)
        w[:, :3] = np.asarray(nl, dtype=np.float32).view(np.uint32)
        w[:, 3], w[:, 4], w[:, 5] = ra, rb, mode
        return w

    for nl in ct.AXIS_NORMALS:
        want = oracle.map_words("cosine", words(nl))
        _assert_same_floats(probe("cosine_axis", words(nl), 3), want, f"cosine_vec<true> {nl}")
        _assert_same_floats(probe("cosine_general", words(nl), 3), want, f"cosine_vec<false> {nl}")
    for nl in ct.GENERAL_NORMALS:
        _assert_same_floats(probe("cosine_general", words(nl), 3), oracle.map_words("cosine", words(nl)),
                            f"cosine_vec<false> {nl}")


def test_normalize_bit_exact(probe, oracle):
    rng = np.random.default_rng(41)
    v = (rng.standard_normal((1 << 18, 3)) * np.exp2(rng.uniform(-20, 20, (1 << 18, 1)))).astype(np.float32)
    v[:64, 0] = 0.0   # zero components, exactly axis-aligned vectors, the zero vector
    v[:32, 1] = 0.0
    v[:4] = 0.0
    v[64:67] = np.eye(3, dtype=np.float32)
    w = v.view(np.uint32)
    _assert_same_floats(probe("normalize3", w, 3), oracle.map_words("normalize", w), "normalize3")
    _assert_same_floats(probe("normalize3_free", w, 3), oracle.map_words("normalize_free", w),
                        "normalize3_free")
    assert np.all(probe("normalize3", w[:4], 3).view(np.float32) == 0)  # 0 * rsq(0) = 0, not NaN


def test_fix31_bit_exact(probe, oracle):
    L, inv = ct.fix_pairs()
    rng = np.random.default_rng(43)
    L = np.concatenate([L, (rng.random(1 << 16) * 40).astype(np.float32)])
    inv = np.concatenate([inv, np.full(1 << 16, 1.0 / 24.0, dtype=np.float32)])
    w = np.stack([L.view(np.uint32), inv.view(np.uint32)], axis=1)
    got = probe("fix31", w, 1)[:, 0]
    assert np.array_equal(got, oracle.fix_batch(L, inv))
    n = len(ct.fix_pairs()[0])
    assert np.array_equal(got[:n], ct.fix_truth(L[:n], inv[:n]))


def test_philox_bit_exact(probe, oracle, spt):
    """philox_px(philox_pixel_key(p, s), c1, c2) == philox4x32(p, c1, c2, s) on the device, both the
    oracle's c_philox, and at the edge counters the Python big-integer Philox."""
    edge = tcm.philox_counters()
    rng = np.random.default_rng(47)
    ctrs = np.concatenate([edge, rng.integers(0, 1 << 32, (1 << 18, 4), dtype=np.uint64).astype(np.uint32)])
    full, px = probe("philox4x32", ctrs, 4), probe("philox_px", ctrs, 4)
    assert np.array_equal(full, px)
    assert np.array_equal(full, oracle.map_words("philox", ctrs))
    key = (0x53505430, spt.PHILOX_KEY1)
    for c, g in zip(edge.tolist(), full[:len(edge)].tolist()):
        assert g == to._philox_py(c, key, 7), c

"""The contract's arithmetic against fp64, point by point (CPU: the oracle's C through
spt_oracle_map; tests/test_gpu_primitives.py holds the device functions to the same C bit for bit).

The error figures asserted here are the ones spt_device.h states. The reference is numpy float64 /
Python integers (tests/contract_truth.py), never the oracle's own code.
"""
import os

import numpy as np
import pytest

import contract_truth as ct
import test_oracle as to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sweep():
    return ct.binade_sweep()


def test_rcp_nr_relative_error(oracle, sweep):
    y = oracle.map_f32("rcp_nr", sweep)
    e = np.abs(ct.rel_err_rcp(sweep, y)).max()
    print(f"rcp_nr [1,4) exhaustive: max relative error {e:.4e}")
    assert e <= ct.RCP_NR_REL
    # odd in x, bit for bit
    assert np.array_equal(oracle.map_f32("rcp_nr", -sweep).view(np.uint32),
                          (-y).view(np.uint32))
    # x and 1/x both normal, with one binade to spare at either end
    x = ct.log_uniform(10 ** 6, -125, 125, seed=11)
    x[::2] *= np.float32(-1)
    e = np.abs(ct.rel_err_rcp(x, oracle.map_f32("rcp_nr", x))).max()
    print(f"rcp_nr log-uniform: max relative error {e:.4e}")
    assert e <= ct.RCP_NR_REL


@pytest.mark.parametrize("name,bound", [("rsq_nr", ct.RSQ_NR_REL), ("rsq_nr2", ct.RSQ_NR2_REL),
                                        ("rsq_nr1", ct.RSQ_NR1_REL)])
def test_rsq_relative_error(oracle, sweep, name, bound):
    for what, x in (("[1,4) exhaustive", sweep),
                    ("log-uniform", ct.log_uniform(10 ** 6, -125, 128, seed=12))):
        e = ct.rel_err_rsq(x, oracle.map_f32(name, x))
        print(f"{name} {what}: relative error in [{e.min():.4e}, {e.max():.4e}]")
        assert np.abs(e).max() <= bound


def test_rsq_nr1_stays_below_the_root_up_to_rounding(oracle, sweep):
    """The free-scale argument wants |d| <= 1 after normalize3_free. One Newton step lands at
    -1.5 e^2 below the root for a seed error e, but its own three roundings can lift it above where
    e is small: measured at most 1.2421e-7 above (RSQ_NR1_ABOVE), never 'always below' as the
    comment once said."""
    for x in (sweep, ct.log_uniform(10 ** 6, -125, 128, seed=13)):
        e = ct.rel_err_rsq(x, oracle.map_f32("rsq_nr1", x))
        print(f"rsq_nr1: at most {e.max():.4e} above the root, {np.mean(e > 0):.3%} of x above it")
        assert e.max() <= ct.RSQ_NR1_ABOVE


# The contract's own bits over the exhaustive [1, 4) sweep: the sum of the results' bit patterns and
# the extreme relative errors (fp64). The fp64 bounds above cannot see a seed constant changed in its
# low bits (three Newton steps converge from any nearby seed); these pins can: the one-step
# function's worst error moves by 3 e0 de0 ~ 1e-8 per unit of the seed's last place. They change
# only when the contract does, together with the golden images.
SWEEP_PINS = {
    "rcp_nr": (17716920895131146, -5.964646732081746e-08, 5.956047743893578e-08),
    "rsq_nr": (17791218913404701, -1.3140239030207113e-07, 1.3241591223511762e-07),
    "rsq_nr1": (17791033215334117, -0.0017512762058086162, 1.2420617578889903e-07),
    "rsq_nr2": (17791218555770793, -4.720364688681755e-06, 1.291390767654832e-07),
}


@pytest.mark.parametrize("name", sorted(SWEEP_PINS))
def test_sweep_pins(oracle, sweep, name):
    y = oracle.map_f32(name, sweep)
    e = ct.rel_err_rcp(sweep, y) if name == "rcp_nr" else ct.rel_err_rsq(sweep, y)
    bits, lo, hi = SWEEP_PINS[name]
    assert abs(e.min() - lo) <= 1e-12 and abs(e.max() - hi) <= 1e-12, (e.min(), e.max())
    assert int(y.view(np.uint32).astype(np.uint64).sum()) == bits


def _cls(v):
    v = np.asarray(v, dtype=np.float32)
    return ["nan" if np.isnan(a) else "inf" if np.isinf(a) else "zero" if a == 0 else "finite" for a in v]


def test_specials_classes(oracle):
    """What the contract's reciprocal / rsqrt return outside the normal range: nothing in the
    renderer may assume more than this. SPECIALS = +-0, +-denormals, 2^-126, +-FLT_MAX, +-inf, NaN."""
    x = ct.SPECIALS
    assert _cls(x) == ["zero", "zero", "finite", "finite", "finite", "finite", "finite", "finite",
                       "inf", "inf", "nan"]
    # rcp_nr: the seed of a zero or denormal x is a huge float whose first step overflows to
    # inf - inf: NaN, not the inf of 1/0. Of FLT_MAX and inf: the seed's subtraction wraps to a
    # negative float and the steps diverge to -+inf.
    assert _cls(oracle.map_f32("rcp_nr", x)) == ["nan", "nan", "nan", "nan", "nan", "finite", "inf",
                                                  "inf", "inf", "inf", "nan"]
    # rsq_nr*: finite (not inf) at zeros and denormals -- x * rsq(x) is then an exact 0 -- finite
    # at FLT_MAX, -inf for every negative input but -0 and denormals, NaN only for NaN
    for name in ("rsq_nr", "rsq_nr1", "rsq_nr2"):
        got = _cls(oracle.map_f32(name, x))
        assert got[:7] == ["finite"] * 7, (name, got)
        assert got[7] == "inf" and got[9] == "inf" and got[10] == "nan", (name, got)
        assert got[8] == "inf", (name, got)  # rsq(+inf): an infinity, of either sign
    # the smallest normal: 1/x = 2^126 is representable and rcp_nr is within its bound there
    assert abs(ct.rel_err_rcp(x[5], oracle.map_f32("rcp_nr", x[5:6])[0])) <= ct.RCP_NR_REL


def test_x_times_rsq_is_an_exact_zero_at_zero(oracle):
    """The sphere root det * rsq_nr2(det) and the cosine sample's R = xi2 * rsq(xi2 (1 - xi2)) rely on
    0 * rsq(0) = 0: rsq of +-0 must be finite."""
    z = np.array([0.0, -0.0], dtype=np.float32)
    for name in ("rsq_nr", "rsq_nr1", "rsq_nr2"):
        r = oracle.map_f32(name, z)
        assert np.all(np.isfinite(r)), (name, r)
        assert np.all(z * r == 0.0) and not np.any(np.isnan(z * r))
    assert np.signbit(z * oracle.map_f32("rsq_nr2", z)).tolist() == [False, True]


def test_disk_dir_every_angle(oracle):
    """All 2^24 values of the bits disk_dir reads, against cos / sin of the angle they name."""
    ra = ct.disk_words()
    c, s = oracle.disk_dir_batch(ra)
    tc, ts = ct.disk_truth(ra)
    c64, s64 = c.astype(np.float64), s.astype(np.float64)
    err = max(np.abs(c64 - tc).max(), np.abs(s64 - ts).max())
    unit = np.abs(c64 * c64 + s64 * s64 - 1.0).max()
    print(f"disk_dir: max abs error {err:.4e}, max |c^2+s^2-1| {unit:.4e}")
    assert err <= 3e-7 and unit <= 3e-7
    # the low byte is not read
    assert np.array_equal(oracle.map_words("disk_dir", ra[::4097] | np.uint32(0xFF)),
                          oracle.map_words("disk_dir", ra[::4097]))
    # exact zeros: the sine of theta = 0 (u = 0) in each octant, nowhere else
    zero = (c == 0) | (s == 0)
    u = (ra >> np.uint32(8)) & np.uint32(0x1FFFFF)
    assert int(zero.sum()) == 8
    assert np.all(u[zero] == 0) and int((u == 0).sum()) == 8
    assert not np.any((c == 0) & (s == 0))


FRAMES = [("axis", n) for n in ct.AXIS_NORMALS] + [("general", n) for n in ct.GENERAL_NORMALS]


@pytest.mark.parametrize("unit", [True, False], ids=["unit", "free"])
@pytest.mark.parametrize("uniform", [False, True], ids=["cosine", "uniform"])
@pytest.mark.parametrize("frame,nl", FRAMES, ids=[f"{f}{i}" for i, (f, _) in enumerate(FRAMES)])
def test_cosine_sample_against_fp64(oracle, frame, nl, uniform, unit):
    ra, rb = ct.cosine_words(10 ** 5, seed=21)
    d = oracle.cosine_batch(nl, ra, rb, uniform, unit).astype(np.float64)
    n = np.sqrt((d * d).sum(axis=1))
    print(f"|d| - 1 in [{(n - 1).min():.3e}, {(n - 1).max():.3e}]")
    assert np.abs(n - 1).max() <= (3e-7 if unit else ct.RSQ_NR1_REL)
    truth = ct.cosine_truth(nl, ra, rb, uniform)
    err = np.abs(d / n[:, None] - truth).max()
    print(f"max component error after normalising {err:.4e}")
    assert err <= (1e-6 if unit else ct.COSINE_FREE_ABS)
    # exact zero components only from an exact zero of disk_dir or of xi2 (the axis frame passes
    # them on; the general frame's sums may or may not cancel)
    c, s = oracle.disk_dir_batch(ra)
    may = (c == 0) | (s == 0) | (oracle.map_words("u01", rb).view(np.float32)[:, 0] == 0)
    zero = (d == 0).any(axis=1)
    assert not np.any(zero & ~may)
    if frame == "axis":
        assert np.all(zero[may])  # and the axis frame always does pass them on
        assert int(zero.sum()) == 16


def test_u01_u16_jitter_are_exact(oracle):
    rng = np.random.default_rng(31)
    v = np.concatenate([rng.integers(0, 1 << 32, 10 ** 5, dtype=np.uint64).astype(np.uint32),
                        np.array([0, 1, 0x1FF, 0x200, 0xFFFFFFFF, 0xFFFFFE00], dtype=np.uint32)])
    u = oracle.map_words("u01", v).view(np.float32)[:, 0]
    assert np.array_equal(u.astype(np.float64), ct.u01_truth(v))
    assert u.max() == np.float32(1 - 2.0 ** -23) and u.min() == 0
    lo, hi = v, v[::-1].copy()
    pair = np.stack([lo, hi], axis=1)
    j = (lo & np.uint32(0xFF)) | ((hi & np.uint32(0xFF)) << np.uint32(8))
    assert np.array_equal(oracle.map_words("u16i", pair)[:, 0], j)
    assert np.array_equal(oracle.map_words("u16", pair).view(np.float32)[:, 0].astype(np.float64),
                          j.astype(np.float64) * 2.0 ** -16)
    assert np.array_equal(oracle.map_words("jitter", pair).view(np.float32)[:, 0].astype(np.float64),
                          2.0 ** 23 + j.astype(np.float64))


def test_fix_integer_formula(oracle):
    L, inv = ct.fix_pairs()
    got = oracle.fix_batch(L, inv)
    want = ct.fix_truth(L, inv)
    assert np.array_equal(got, want), [(float(a), float(b), int(g), int(w))
                                       for a, b, g, w in zip(L, inv, got, want) if g != w]
    assert got.max() == 1 << 31 and got.min() == 0


def test_philox_batch_is_the_contracts_generator(oracle, spt):
    """spt_oracle_map's Philox: 7 rounds, the fixed key, counter (pixel, sample, vertex | stream,
    seed) -- against the Python big-integer Philox."""
    ctrs = philox_counters()
    got = oracle.map_words("philox", ctrs)
    key = (0x53505430, spt.PHILOX_KEY1)
    for c, g in zip(ctrs.tolist(), got.tolist()):
        assert g == to._philox_py(c, key, 7), c


def philox_counters() -> np.ndarray:
    """(pixel, sample, vertex | stream << 31, seed) at the edges of every word."""
    rows = [(p, s, c2, sd)
            for p in (0, 1, (1 << 24) - 1, (1 << 24) + 1, (1 << 32) - 1)
            for s in (0, 1, 511, (1 << 31) - 1, 1 << 31)
            for c2 in (1, 2, 1 | (1 << 31), 17 | (1 << 24), 40 | (3 << 24) | (1 << 31))
            for sd in (0, 1, (1 << 32) - 1)]
    return np.array(rows, dtype=np.uint32)


def test_probe_is_built_with_the_kernels_flags():
    """tests/probe/Makefile compiles the device primitives with the render kernel's HIPFLAGS, to the
    letter: -ffp-contract=off and the correctly rounded division are what the probe is there for."""
    a = ct.makefile_hipflags(os.path.join(ROOT, "small-pathtracer_amd", "csrc", "Makefile"))
    b = ct.makefile_hipflags(os.path.join(ROOT, "tests", "probe", "Makefile"))
    assert a == b
    assert "-ffp-contract=off" in a.split() and "-fhip-fp32-correctly-rounded-divide-sqrt" in a.split()

"""The two-half a-trous filter (include/spt.h SPT_HAS_DENOISE_PAIR) on the CPU: the host statement
spt_denoise_pair_host against tests/denoise_pair_truth.py (the header's text restated in numpy float32),
bit for bit, the properties the header's rules imply, and the calibration of diff^2 where it can be
derived.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import denoise_pair_truth as dpt
import denoise_truth as dt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (3, 2), (17, 13), (40, 56)]
ITERATIONS = (0, 1, 2, 3, 6)
REL_SUM = 1e-9  # tests/test_gpu_film_noise.py's tolerance for a sum taken in another order
_halves = {}


def halves(w, h):
    """-> the seven planes (read-only) of the synthetic pair of this size."""
    if (w, h) not in _halves:
        planes, _clean = dpt.synthetic_halves(w, h)
        for a in planes:
            a.setflags(write=False)
        _halves[(w, h)] = planes
    return _halves[(w, h)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want, label):
    assert np.array_equal(bits(got), bits(want)), label


# ---- 1. host equals the numpy truth ---------------------------------------------------------------
@pytest.mark.parametrize("pair_flags", [0, 1])
@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_host_statement_equals_the_truth(spt, w, h, flags, pair_flags):
    P = halves(w, h)
    for it in ITERATIONS:
        p = spt.default_denoise_params(iterations=it, flags=flags)
        out, se_out, diff = spt.denoise_pair_host(*P, p, pair_flags)
        want, want_se, want_diff = dpt.denoise_pair_truth(*P, iterations=it, flags=flags, pair_flags=pair_flags)
        label = (w, h, it, flags, pair_flags)
        same(out, want, ("out",) + label)
        same(se_out, want_se, ("se_out",) + label)
        same(diff, want_diff, ("diff",) + label)
        # the optional planes left NULL change nothing in out
        only, none_se, none_diff = spt.denoise_pair_host(*P, p, pair_flags, return_se=False, return_diff=False)
        assert none_se is None and none_diff is None
        same(only, want, ("out alone",) + label)
        _, _, d2 = spt.denoise_pair_host(*P, p, pair_flags, return_se=False)
        same(d2, want_diff, ("diff without se_out",) + label)


def test_host_statement_equals_the_truth_with_other_parameters(spt):
    P = halves(17, 13)
    kw = dict(iterations=3, sigma_color=2.5, sigma_depth=0.5, sigma_albedo=0.3, normal_squarings=0,
              albedo_floor=0.3)
    for pf in (0, 1):
        got = spt.denoise_pair_host(*P, spt.default_denoise_params(**kw), pf)
        want = dpt.denoise_pair_truth(*P, pair_flags=pf, **kw)
        for g, w_, name in zip(got, want, ("out", "se_out", "diff")):
            same(g, w_, (name, pf))


# ---- 2. equal halves ------------------------------------------------------------------------------
@pytest.mark.parametrize("pair_flags", [0, 1])
def test_equal_halves_give_the_single_filter(spt, pair_flags):
    """Both halves the same planes: g * w_c is the single filter's product, so each half's result is
    spt_denoise_host's; out = 0.5 * (o + o) = o, diff = +0, se_out = (0.5 * sqrtf(v + v)) * a with v the
    single run's (the truth's v plane, tied to the single run by sqrtf(v) * a == its se_out)."""
    s = dt.synthetic(40, 56)
    F = np.float32
    both = (s["rgb"], s["se"], s["rgb"], s["se"], s["albedo"], s["normal"], s["depth"])
    for flags in (0, 1):
        a = np.ones_like(s["albedo"]) if flags else np.fmax(s["albedo"], F(0.01))
        for it in (0, 1, 5):
            p = spt.default_denoise_params(iterations=it, flags=flags)
            out, se_out, diff = spt.denoise_pair_host(*both, p, pair_flags)
            single, single_se = spt.denoise_host(*dt.planes_of(s), p, return_se=True)
            same(out, single, ("out", it, flags))
            if it == 0:
                same(se_out, F(0.5) * np.sqrt(s["se"] * s["se"] + s["se"] * s["se"]), ("se_out", it))
            else:
                v, vb = dpt.denoise_pair_truth(*both, iterations=it, flags=flags, pair_flags=pair_flags,
                                               return_v=True)[3:]
                same(v, vb, "both halves carry one v")
                same(np.sqrt(v)[..., None] * a, single_se, "v is the single run's v")
                same(se_out, (F(0.5) * np.sqrt(v + v))[..., None] * a, ("se_out", it, flags))
            assert not bits(diff).any(), "diff is +0 everywhere"


# ---- 3. symmetry ----------------------------------------------------------------------------------
@pytest.mark.parametrize("pair_flags", [0, 1])
def test_swapping_the_halves(spt, pair_flags):
    ra, sa, rb, sb, al, no, de = halves(40, 56)
    for it in (0, 2, 5):
        p = spt.default_denoise_params(iterations=it)
        out, se_out, diff = spt.denoise_pair_host(ra, sa, rb, sb, al, no, de, p, pair_flags)
        out2, se_out2, diff2 = spt.denoise_pair_host(rb, sb, ra, sa, al, no, de, p, pair_flags)
        same(out, out2, ("out", it))
        same(se_out, se_out2, ("se_out", it))
        # 0.5f * (a - b) and 0.5f * (b - a) are each other's negation bit for bit, except where a == b:
        # IEEE a - a is +0 in either order (the clamped pixels of the synthetic planes)
        zero = diff == 0
        same(diff[~zero], -diff2[~zero], ("diff negated", it))
        assert not bits(diff[zero]).any() and not bits(diff2[zero]).any() and (~zero).any()


def test_cross_and_own_weights_differ(spt):
    P = halves(40, 56)
    cross = spt.denoise_pair_host(*P, None, 0)
    own = spt.denoise_pair_host(*P, None, spt.DENOISE_PAIR_OWN_WEIGHTS)
    assert (bits(cross[0]) != bits(own[0])).any() and (bits(cross[2]) != bits(own[2])).any()


# ---- 4. calibration -------------------------------------------------------------------------------
N_REAL = 32


def _ratio_and_se(spt, params, pair_flags, sigma=0.05):
    """r = mean(diff^2) / mean(sample variance of out across realisations) over N_REAL realisations of
    two iid halves on dt.synthetic(64, 48, seed=1, sigma), and its leave-one-realisation-out jackknife
    standard error."""
    outs, d2 = [], []
    for k in range(N_REAL):
        P, _clean = dpt.synthetic_halves(64, 48, seed=1, sigma=sigma, realisation=k)
        out, _, diff = spt.denoise_pair_host(*P, params, pair_flags, return_se=False)
        outs.append(out.astype(np.float64))
        d2.append(float(np.mean(diff.astype(np.float64) ** 2)))
    outs, d2 = np.stack(outs), np.array(d2)

    def ratio(keep):
        return d2[keep].mean() / outs[keep].var(axis=0, ddof=1).mean()

    every = np.arange(N_REAL)
    r = ratio(every)
    jack = np.array([ratio(every[every != k]) for k in range(N_REAL)])
    se = np.sqrt((N_REAL - 1) / N_REAL * np.sum((jack - jack.mean()) ** 2))
    return float(r), float(se)


def test_diff_squared_is_calibrated_with_own_weights(spt):
    """Own weights: the two results are functions of independent samples, so E[diff^2] = Var(out) and
    E[r] = 1. Asserted: |r - 1| <= 5 standard errors (jackknife over the realisations)."""
    r, se = _ratio_and_se(spt, spt.default_denoise_params(), spt.DENOISE_PAIR_OWN_WEIGHTS)
    print(f"own weights: r = {r:.4f}, s.e. {se:.4f}")
    assert abs(r - 1.0) <= 5 * se, (r, se)


def test_diff_squared_is_calibrated_when_the_colours_do_not_weigh(spt):
    """Cross weights with sigma_color = 1e6: the colour weights are 1 whatever the colours, the halves
    are independent again, E[r] = 1."""
    r, se = _ratio_and_se(spt, spt.default_denoise_params(sigma_color=1e6), 0)
    print(f"cross weights, sigma_color 1e6: r = {r:.4f}, s.e. {se:.4f}")
    assert abs(r - 1.0) <= 5 * se, (r, se)


def test_diff_squared_reads_low_with_cross_weights(spt):
    """Cross weights at the default sigma_color: A's weights are B's data, the results correlate
    positively and diff^2 under-reads. Only r < 1 + 5 s.e. is asserted; the figure is printed."""
    r, se = _ratio_and_se(spt, spt.default_denoise_params(), 0)
    print(f"cross weights: r = {r:.4f}, s.e. {se:.4f}")
    assert r < 1.0 + 5 * se, (r, se)


# ---- 5. the summary -------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_summary_host_equals_float64_numpy(spt, w, h):
    _, _, diff = spt.denoise_pair_host(*halves(w, h), spt.default_denoise_params(iterations=2), 0)
    got, want = spt.pair_summary_host(diff), dpt.pair_summary_truth(diff)
    for k in range(3):
        assert abs(got["rmse"][k] - want["rmse"][k]) <= REL_SUM * want["rmse"][k], (k, got, want)
    assert abs(got["rmse_all"] - want["rmse_all"]) <= REL_SUM * want["rmse_all"]
    assert got["diff_max"] == want["diff_max"]


# ---- 6. rejections, layout, symbols ---------------------------------------------------------------
def test_rejected_calls_leave_every_output_untouched(spt):
    lib = spt.load_library()
    P = [a.copy() for a in halves(17, 13)]
    w, h = 17, 13
    fill = np.float32(-7.25)
    ok = spt.default_denoise_params
    nan, inf = float("nan"), float("inf")

    def call(planes, w_, h_, p, pf, out, se_out, diff):
        ptr = [a.ctypes.data if a is not None else None for a in planes]
        return lib.spt_denoise_pair_host(*ptr, w_, h_, ctypes.byref(p) if p is not None else None, pf,
                                         *[o.ctypes.data if o is not None else None for o in (out, se_out, diff)])

    cases = [(f"null plane {k}", P[:k] + [None] + P[k + 1:], w, h, ok(), 0) for k in range(7)]
    cases += [("iterations -1", P, w, h, ok(iterations=-1), 0), ("iterations 7", P, w, h, ok(iterations=7), 0),
              ("squarings 9", P, w, h, ok(normal_squarings=9), 0), ("flags 2", P, w, h, ok(flags=2), 0),
              ("reserved", P, w, h, ok(reserved=1), 0), ("null params", P, w, h, None, 0),
              ("pair_flags 2", P, w, h, ok(), 2), ("pair_flags 3", P, w, h, ok(), 3),
              ("pair_flags high", P, w, h, ok(), 0x80000001),
              ("width 0", P, 0, h, ok(), 0), ("height 0", P, w, 0, ok(), 0), ("width < 0", P, -w, h, ok(), 0),
              ("too many pixels", P, 65536, 32768, ok(), 0)]
    for field in ("sigma_color", "sigma_depth", "sigma_albedo", "albedo_floor"):
        cases += [(f"{field} {v}", P, w, h, ok(**{field: v}), 0) for v in (0.0, -1.0, nan, inf)]
    for label, planes, w_, h_, p, pf in cases:
        outs = [np.full((h, w, 3), fill) for _ in range(3)]
        assert call(planes, w_, h_, p, pf, *outs) == 1, label
        assert all((o == fill).all() for o in outs), label
        assert lib.spt_last_error(), label
    outs = [np.full((h, w, 3), fill) for _ in range(3)]
    assert call(P, w, h, ok(), 0, None, outs[1], outs[2]) == 1  # a null out
    before = [a.copy() for a in P]
    for k in range(6):  # an output that is an input (the depth plane is too short to try as one)
        for slot in range(3):
            o = list(outs)
            o[slot] = P[k]
            assert call(P, w, h, ok(), 0, *o) == 1, (k, slot)
    for i, j in ((0, 1), (0, 2), (1, 2)):  # two outputs that are one plane
        o = list(outs)
        o[j] = o[i]
        assert call(P, w, h, ok(), 0, *o) == 1, (i, j)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(P, before))
    assert all((o == fill).all() for o in outs)
    # ... and the same arguments in range are accepted, with and without the optional planes
    assert call(P, w, h, ok(), 1, outs[0], None, None) == 0 and (outs[0] != fill).all()
    assert (outs[1] == fill).all() and (outs[2] == fill).all()
    assert call(P, w, h, ok(), 0, *outs) == 0 and all((o != fill).any() for o in outs)
    s = spt.spt_pair_summary()
    d = outs[2]
    assert lib.spt_denoise_pair_summary_host(None, w, h, ctypes.byref(s)) == 1
    assert lib.spt_denoise_pair_summary_host(d.ctypes.data, w, h, None) == 1
    assert lib.spt_denoise_pair_summary_host(d.ctypes.data, 0, h, ctypes.byref(s)) == 1
    assert lib.spt_denoise_pair_summary_host(d.ctypes.data, w, -1, ctypes.byref(s)) == 1
    assert lib.spt_denoise_pair_summary_host(d.ctypes.data, w, h, ctypes.byref(s)) == 0


def test_abi_markers(spt):
    hdr = open(os.path.join(ROOT, "include", "spt.h")).read()
    assert re.search(r"^#define SPT_HAS_DENOISE_PAIR 1\b", hdr, re.M)
    assert re.search(r"^#define SPT_DENOISE_PAIR_OWN_WEIGHTS 1u\b", hdr, re.M)
    assert re.search(r"^#define SPT_ABI_VERSION 6\b", hdr, re.M)
    assert spt.SPT_HAS_DENOISE_PAIR == 1 and spt.DENOISE_PAIR_OWN_WEIGHTS == 1
    assert ctypes.sizeof(spt.spt_pair_summary) == 40
    assert ctypes.sizeof(spt.spt_denoise_params) == 32
    lib = spt.load_library()
    for name in ("spt_denoise_pair_async", "spt_denoise_pair_host", "spt_denoise_pair_summary",
                 "spt_denoise_pair_summary_host", "spt_film_pair_denoise"):
        assert name in spt.EXPORTS and hasattr(lib, name)

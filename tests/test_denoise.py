"""The a-trous filter (include/spt.h SPT_HAS_DENOISE) on the CPU: the host statement
spt_denoise_host against tests/denoise_truth.py (the header's text restated in numpy float32), bit for
bit, and the properties the header's rules imply.
"""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import denoise_truth as dt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (3, 2), (5, 1), (1, 5), (17, 13), (40, 56)]
_synth = {}


def synth(w, h):
    if (w, h) not in _synth:
        s = dt.synthetic(w, h)
        for a in s.values():
            a.setflags(write=False)
        _synth[(w, h)] = s
    return _synth[(w, h)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ulps(a, b):
    """Distance in units of the last place between float32 arrays of equal sign (or zeros)."""
    return np.abs(bits(a).astype(np.int64) - bits(b).astype(np.int64))


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_host_statement_equals_the_truth(spt, w, h, flags):
    s = synth(w, h)
    for it in range(7):
        out, se_out = spt.denoise_host(*dt.planes_of(s), spt.default_denoise_params(iterations=it, flags=flags),
                                       return_se=True)
        want, want_se = dt.denoise_truth(*dt.planes_of(s), iterations=it, flags=flags)
        assert np.array_equal(bits(out), bits(want)), (w, h, it, flags)
        assert np.array_equal(bits(se_out), bits(want_se)), (w, h, it, flags)


def test_host_statement_equals_the_truth_with_other_parameters(spt):
    s = synth(17, 13)
    kw = dict(iterations=3, sigma_color=2.5, sigma_depth=0.5, sigma_albedo=0.3, normal_squarings=0,
              albedo_floor=0.3)
    out, se_out = spt.denoise_host(*dt.planes_of(s), spt.default_denoise_params(**kw), return_se=True)
    want, want_se = dt.denoise_truth(*dt.planes_of(s), **kw)
    assert np.array_equal(bits(out), bits(want)) and np.array_equal(bits(se_out), bits(want_se))


def test_default_params(spt):
    p = spt.default_denoise_params()
    assert (p.iterations, p.normal_squarings, p.flags, p.reserved) == (5, 7, 0, 0)
    assert (p.sigma_color, p.sigma_depth) == (4.0, 1.0)
    assert p.sigma_albedo == np.float32(0.1) and p.albedo_floor == np.float32(0.01)
    assert ctypes.sizeof(spt.spt_denoise_params) == 32


def test_zero_iterations_copy_bits(spt):
    s = synth(17, 13)
    rgb = s["rgb"].copy()
    rgb[0, 0] = [np.float32("nan"), -0.0, 7.5]  # a copy keeps what a divide and multiply would not
    out, se_out = spt.denoise_host(rgb, s["se"], s["albedo"], s["normal"], s["depth"],
                                   spt.default_denoise_params(iterations=0), return_se=True)
    assert np.array_equal(bits(out), bits(rgb)) and np.array_equal(bits(se_out), bits(s["se"]))


def test_without_variance_only_the_centre_tap_survives(spt):
    """se = 0 everywhere and distinct colours: every colour weight is phi of a huge number, 0, so
    c' = (w c) / w with w = 9/64, then a multiply by the divisor the colour was divided by: four
    roundings, within 4 ulp."""
    s = synth(17, 13)
    rng = np.random.default_rng(7)
    rgb = (0.05 + 0.9 * rng.random((13, 17, 3))).astype(np.float32)
    out, se_out = spt.denoise_host(rgb, np.zeros_like(rgb), s["albedo"], s["normal"], s["depth"],
                                   return_se=True)
    assert ulps(out, rgb).max() <= 4
    assert not se_out.any()


def test_no_weight_crosses_an_edge(spt):
    """The two regions of the synthetic image differ in normal (orthogonal) and albedo (far apart):
    every tap from one into the other has weight exactly 0. The taps of a pixel next to the edge
    reach two pixels into the other region, so new colours there must leave this region's bits alone.
    The variance prefilter vt is a plain 3x3 filter, not edge-stopped (spt.h), so the other region's
    se is changed everywhere except in the one column that the 3x3 windows of this region touch, and
    the comparison is after one iteration: later iterations read the v' of that column, which the new
    colours have changed."""
    s = synth(40, 56)
    left = s["region"] == 0
    p = spt.default_denoise_params(iterations=1)
    base = spt.denoise_host(*dt.planes_of(s), p)
    rgb, se = s["rgb"].copy(), s["se"].copy()
    right = np.zeros_like(left)
    right[:, 20:] = True
    rgb[right] = (rgb[right] * np.float32(0.5) + np.float32(0.3))
    far = right.copy()
    far[:, 20] = False
    se[far] = se[far] * np.float32(3)
    other = spt.denoise_host(rgb, se, s["albedo"], s["normal"], s["depth"], p)
    assert np.array_equal(bits(base[left]), bits(other[left]))
    changed = (bits(base) != bits(other)).any(axis=2)
    assert changed[:, 20:][s["region"][:, 20:] == 1].all()  # ... and the other region did change


def test_a_miss_pixel_comes_back(spt):
    """All features zero: the normal weight of every tap but the centre's is 0."""
    s = synth(40, 56)
    miss = s["region"] == 2
    assert miss.sum() >= 2
    out = spt.denoise_host(*dt.planes_of(s))
    assert ulps(out[miss], np.minimum(s["rgb"][miss], np.float32(1))).max() <= 1
    nd = spt.denoise_host(*dt.planes_of(s), spt.default_denoise_params(flags=spt.DENOISE_NO_DEMODULATE))
    assert ulps(nd[miss], np.minimum(s["rgb"][miss], np.float32(1))).max() <= 1


def _rejections(spt, s):
    """(label, planes, width, height, params) of every call spt_denoise_host must refuse."""
    P = dt.planes_of(s)
    h, w = s["depth"].shape
    ok = spt.default_denoise_params
    nan, inf = float("nan"), float("inf")
    cases = [(f"null plane {k}", P[:k] + [None] + P[k + 1:], w, h, ok()) for k in range(5)]
    cases += [("iterations -1", P, w, h, ok(iterations=-1)), ("iterations 7", P, w, h, ok(iterations=7)),
              ("squarings -1", P, w, h, ok(normal_squarings=-1)), ("squarings 9", P, w, h, ok(normal_squarings=9)),
              ("flags 2", P, w, h, ok(flags=2)), ("flags high", P, w, h, ok(flags=0x80000001)),
              ("reserved", P, w, h, ok(reserved=1)),
              ("width 0", P, 0, h, ok()), ("height 0", P, w, 0, ok()), ("width < 0", P, -w, h, ok()),
              ("too many pixels", P, 65536, 32768, ok())]
    for field in ("sigma_color", "sigma_depth", "sigma_albedo", "albedo_floor"):
        cases += [(f"{field} {v}", P, w, h, ok(**{field: v})) for v in (0.0, -1.0, nan, inf)]
    return cases


def test_rejected_calls_leave_out_untouched(spt):
    s = synth(17, 13)
    lib = spt.load_library()
    fill = np.float32(-7.25)

    def call(planes, w, h, p, out, se_out):
        ptr = [a.ctypes.data if a is not None else None for a in planes]
        return lib.spt_denoise_host(*ptr, w, h, ctypes.byref(p) if p is not None else None,
                                    out.ctypes.data if out is not None else None,
                                    se_out.ctypes.data if se_out is not None else None)

    cases = _rejections(spt, s) + [("null params", dt.planes_of(s), 17, 13, None)]
    for label, planes, w, h, p in cases:
        out, se_out = np.full((13, 17, 3), fill), np.full((13, 17, 3), fill)
        assert call(planes, w, h, p, out, se_out) == 1, label
        assert (out == fill).all() and (se_out == fill).all(), label
        assert lib.spt_last_error(), label
    P = [a.copy() for a in dt.planes_of(s)]
    ok = spt.default_denoise_params()
    assert call(P, 17, 13, ok, None, None) == 1  # a null out
    for k in range(4):  # an output that is an input (the depth plane is too short to try as one)
        before = [a.copy() for a in P]
        se_out = np.full((13, 17, 3), fill)
        assert call(P, 17, 13, ok, P[k], se_out) == 1 and call(P, 17, 13, ok, se_out, P[k]) == 1
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(P, before)) and (se_out == fill).all()
    out = np.full((13, 17, 3), fill)
    assert call(P, 17, 13, ok, out, out) == 1 and (out == fill).all()
    # ... and the same arguments in range are accepted, with and without se_out
    assert call(P, 17, 13, ok, out, None) == 0 and (out != fill).all()


def test_noise_reduction_on_the_two_plane_image(spt):
    """40x56, sigma = 0.05. The ideal 5x5 B3 filter leaves sqrt(sum h^4) = 70/256 = 0.27 of flat
    Gaussian noise after one iteration; edges, the image border and the unfiltered miss pixels cost
    the rest of the bound of 0.6, and five iterations must reach 0.25."""
    s = synth(40, 56)
    noisy = rmse(np.minimum(s["rgb"], 1), s["clean"])
    assert 0.045 < noisy < 0.055
    one = rmse(spt.denoise_host(*dt.planes_of(s), spt.default_denoise_params(iterations=1)), s["clean"])
    five = rmse(spt.denoise_host(*dt.planes_of(s), spt.default_denoise_params(iterations=5)), s["clean"])
    print(f"rmse ratio to noisy: 1 iteration {one / noisy:.3f}, 5 iterations {five / noisy:.3f}")
    assert one <= 0.6 * noisy
    assert five <= 0.25 * noisy


def test_se_out_tracks_the_weights(spt):
    """Without demodulation (a = 1, so the three channels share v) se_out after one iteration is the
    input's se times sqrt(sum w^2) / sum w of the weights that survive: never above the input's, and
    near 70/256 of it where all 25 taps survive."""
    s = synth(40, 56)
    _, se_out = spt.denoise_host(*dt.planes_of(s), spt.default_denoise_params(iterations=1, flags=1),
                                 return_se=True)
    plain = s["region"] <= 1
    assert (se_out[plain] <= s["se"][plain] * np.float32(1.0001)).all()
    assert np.median(se_out[plain] / s["se"][plain]) < 0.5


def test_abi_markers(spt):
    hdr = open(os.path.join(ROOT, "include", "spt.h")).read()
    assert re.search(r"^#define SPT_HAS_DENOISE 1\b", hdr, re.M)
    assert re.search(r"^#define SPT_ABI_VERSION 6\b", hdr, re.M)
    assert spt.SPT_HAS_DENOISE == 1 and spt.load_library().spt_abi_version() == 6
    lib = spt.load_library()
    for name in ("spt_denoise_default_params", "spt_denoiser_create", "spt_denoiser_destroy",
                 "spt_denoise_async", "spt_denoise_host", "spt_film_denoise"):
        assert name in spt.EXPORTS and hasattr(lib, name)
    for rel in ("csrc/spt_denoise.hip", "csrc/spt_denoise_host.cpp", "csrc/spt_denoise.h"):
        assert rel in spt.KERNEL_SOURCES
    assert math.isclose(70 / 256, math.sqrt(sum((a * b) ** 2 for a in (1, 4, 6, 4, 1) for b in (1, 4, 6, 4, 1))) / 256)

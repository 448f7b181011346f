"""The filter bank (include/spt.h SPT_HAS_DENOISE_BANK) on the CPU: the host statement
spt_denoise_bank_host against tests/denoise_bank_truth.py (the header's text restated in numpy float32),
bit for bit; the properties the header's rules imply; the calibration of the cross-validated error where
it can be derived; and that the bank beats its best candidate where the candidates fail in different
places.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import denoise_bank_truth as dbt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (3, 2), (17, 13), (40, 56)]
# the candidates of the n-candidate cases: sigma_color and iterations differ, one has no iteration at all
CANDS = [dict(sigma_color=2.0, iterations=5), dict(sigma_color=8.0, iterations=3),
         dict(sigma_color=4.0, iterations=0), dict(sigma_color=1.0, iterations=1, flags=1)]
REL_SUM = 1e-9  # tests/test_gpu_film_noise.py's tolerance for a sum taken in another order
_halves = {}


def halves(w, h):
    """-> the seven planes (read-only) of the synthetic pair of this size."""
    if (w, h) not in _halves:
        planes = dbt.bank_halves(w, h)
        for a in planes:
            a.setflags(write=False)
        _halves[(w, h)] = planes
    return _halves[(w, h)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want, label):
    assert np.array_equal(bits(got), bits(want)), label


def params_of(spt, cands):
    return [spt.default_denoise_params(**c) for c in cands]


# ---- 1. host equals the numpy truth ---------------------------------------------------------------
@pytest.mark.parametrize("pair_flags", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 4])
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_host_statement_equals_the_truth(spt, w, h, n, pair_flags):
    P = halves(w, h)
    for ei in (0, 1, 2, 3):
        out, mse, choice = spt.denoise_bank_host(*P, params_of(spt, CANDS[:n]), None, pair_flags, ei)
        want, want_mse, want_choice = dbt.denoise_bank_truth(*P, CANDS[:n], ei, pair_flags)
        label = (w, h, n, ei, pair_flags)
        same(out, want, ("out",) + label)
        same(mse, want_mse, ("mse",) + label)
        assert np.array_equal(choice, want_choice), ("choice",) + label
        assert choice.max() < n
    # the optional planes left NULL change nothing in out
    only, none_mse, none_choice = spt.denoise_bank_host(*P, params_of(spt, CANDS[:n]), None, pair_flags, 3,
                                                        return_mse=False, return_choice=False)
    assert none_mse is None and none_choice is None
    same(only, want, "out alone")
    _, m2, _ = spt.denoise_bank_host(*P, params_of(spt, CANDS[:n]), None, pair_flags, 3, return_choice=False)
    same(m2, want_mse, "mse without choice")


def test_the_smoothing_takes_its_geometry_from_the_first_candidate(spt):
    """Other sigma_depth / sigma_albedo / normal_squarings in cands[0] than in cands[1]: the truth, which
    reads cands[0]'s, is met bit for bit, and the two orders of the candidates differ."""
    P = halves(17, 13)
    a = dict(sigma_color=2.0, sigma_depth=0.5, sigma_albedo=0.3, normal_squarings=0, albedo_floor=0.3)
    b = dict(sigma_color=8.0, iterations=2)
    got = []
    for order in ((a, b), (b, a)):
        out, mse, choice = spt.denoise_bank_host(*P, params_of(spt, order))
        want = dbt.denoise_bank_truth(*P, list(order))
        same(out, want[0], "out")
        same(mse, want[1], "mse")
        assert np.array_equal(choice, want[2])
        got.append(np.sort(mse.ravel()))
    assert (bits(got[0]) != bits(got[1])).any()


# ---- 2. exact properties --------------------------------------------------------------------------
@pytest.mark.parametrize("pair_flags", [0, 1])
def test_one_candidate_is_the_pair_filter(spt, pair_flags):
    P = halves(40, 56)
    for it in (0, 2, 5):
        p = spt.default_denoise_params(iterations=it)
        pair_out, _, _ = spt.denoise_pair_host(*P, p, pair_flags, return_se=False, return_diff=False)
        assert not (bits(pair_out) == 0x80000000).any()  # no -0: the header's one exception does not arise
        for ei in (0, 2):
            out, mse, choice = spt.denoise_bank_host(*P, [p], None, pair_flags, ei)
            same(out, pair_out, ("out", it, ei))
            assert not choice.any()


@pytest.mark.parametrize("pair_flags", [0, 1])
def test_two_identical_candidates(spt, pair_flags):
    P = halves(40, 56)
    p = spt.default_denoise_params(sigma_color=3.0)
    pair_out, _, _ = spt.denoise_pair_host(*P, p, pair_flags, return_se=False, return_diff=False)
    out, mse, choice = spt.denoise_bank_host(*P, [p, p], None, pair_flags)
    one = spt.denoise_bank_host(*P, [p], None, pair_flags)
    assert not choice.any(), "`<` with k ascending: a tie goes to the first"
    same(out, pair_out, "out")
    same(mse, one[1], "mse")


@pytest.mark.parametrize("pair_flags", [0, 1])
def test_swapping_the_halves(spt, pair_flags):
    ra, sa, rb, sb, al, no, de = halves(40, 56)
    assert (bits(sa) != bits(sb)).any(), "the halves' error planes differ, so the swap swaps something"
    for n in (1, 2, 4):
        got = spt.denoise_bank_host(ra, sa, rb, sb, al, no, de, params_of(spt, CANDS[:n]), None, pair_flags)
        swapped = spt.denoise_bank_host(rb, sb, ra, sa, al, no, de, params_of(spt, CANDS[:n]), None, pair_flags)
        same(got[0], swapped[0], ("out", n))
        same(got[1], swapped[1], ("mse", n))
        assert np.array_equal(got[2], swapped[2]), ("choice", n)


def test_the_candidates_are_told_apart(spt):
    P = halves(40, 56)
    out, mse, choice = spt.denoise_bank_host(*P, params_of(spt, CANDS[:2]))
    assert 0 < choice.mean() < 1, "both candidates are chosen somewhere"
    alone = [spt.denoise_bank_host(*P, params_of(spt, [c]))[0] for c in CANDS[:2]]
    assert (bits(out) != bits(alone[0])).any() and (bits(out) != bits(alone[1])).any()


# ---- 3. calibration -------------------------------------------------------------------------------
N_REAL = 32
FLAT = np.s_[:, :dbt.DETAIL_X0]
DETAIL = np.s_[:, dbt.DETAIL_X0:]
_runs = {}


def runs(spt, sigma_colors):
    """Per realisation of dbt.calibration_halves, own weights, the default error_iterations: the mean of
    mse, the mean true squared error of out against the clean image (whole image, flat region, detail
    region), the mean diff^2 of the pair filter (one candidate only) and the choice's share of candidate 1
    in the flat and of candidate 0 in the detail region. Computed once per candidate set."""
    key = tuple(sigma_colors)
    if key not in _runs:
        rows = []
        for k in range(N_REAL):
            P, clean = dbt.calibration_halves(realisation=k)
            cands = [spt.default_denoise_params(sigma_color=s) for s in sigma_colors]
            out, mse, choice = spt.denoise_bank_host(*P, cands)
            err = ((out.astype(np.float64) - clean) ** 2).mean(axis=2)
            d2 = np.nan
            if len(cands) == 1:
                _, _, diff = spt.denoise_pair_host(*P, cands[0], spt.DENOISE_PAIR_OWN_WEIGHTS, return_se=False)
                d2 = (diff.astype(np.float64) ** 2).mean()
            rows.append((mse.astype(np.float64).mean(), err.mean(), err[FLAT].mean(), err[DETAIL].mean(), d2,
                         (choice[FLAT] == 1).mean(), (choice[DETAIL] == 0).mean()))
        _runs[key] = np.array(rows)
        _runs[key].setflags(write=False)
    return _runs[key]


def jackknife(stat, n=N_REAL):
    """stat(keep) over all realisations and its leave-one-out jackknife standard error, as
    tests/test_denoise_pair.py takes it."""
    every = np.arange(n)
    jack = np.array([stat(every[every != k]) for k in range(n)])
    return float(stat(every)), float(np.sqrt((n - 1) / n * np.sum((jack - jack.mean()) ** 2)))


@pytest.mark.parametrize("sigma_color", [2.0, 8.0])
def test_mse_is_calibrated_with_own_weights(spt, sigma_color):
    """One candidate, own weights, iid halves, se the exact standard deviation: E[mse] = MSE(out), bias
    included (include/spt.h), so r = mean mse / mean true squared error has E[r] = 1 at a narrow and at a
    wide sigma_color. Asserted: |r - 1| <= 5 standard errors."""
    t = runs(spt, [sigma_color])
    r, se = jackknife(lambda keep: t[keep, 0].mean() / t[keep, 1].mean())
    print(f"sigma_color {sigma_color}: mse r = {r:.4f}, s.e. {se:.4f}")
    assert abs(r - 1.0) <= 5 * se, (r, se)


def test_mse_sees_the_bias_that_diff_squared_cannot(spt):
    """At the wide sigma_color the detail is blurred away in both halves alike: the error of out is nearly
    all bias, which cancels in diff. The ratio taken with diff^2 lies below 1 - 5 s.e."""
    t = runs(spt, [8.0])
    r, se = jackknife(lambda keep: t[keep, 4].mean() / t[keep, 1].mean())
    print(f"sigma_color 8: diff^2 r = {r:.4f}, s.e. {se:.4f}")
    assert r < 1.0 - 5 * se, (r, se)


def test_the_bank_beats_its_best_candidate(spt):
    narrow, wide, bank = runs(spt, [2.0]), runs(spt, [8.0]), runs(spt, [2.0, 8.0])
    # the precondition: each candidate's regional error is at least twice the other's in its bad region
    flat_n, flat_w = narrow[:, 2].mean(), wide[:, 2].mean()
    det_n, det_w = narrow[:, 3].mean(), wide[:, 3].mean()
    print(f"flat: narrow {flat_n:.3e} wide {flat_w:.3e}; detail: narrow {det_n:.3e} wide {det_w:.3e}")
    assert flat_n >= 2 * flat_w and det_w >= 2 * det_n
    best = narrow if narrow[:, 1].mean() <= wide[:, 1].mean() else wide
    gain, se = jackknife(lambda keep: best[keep, 1].mean() - bank[keep, 1].mean())
    print(f"true MSE: narrow {narrow[:, 1].mean():.3e} wide {wide[:, 1].mean():.3e} bank {bank[:, 1].mean():.3e}; "
          f"gain over the better {gain:.3e}, s.e. {se:.3e}")
    assert gain > 5 * se, (gain, se)
    share_wide_flat, share_narrow_detail = bank[:, 5].mean(), bank[:, 6].mean()
    print(f"choice: wide holds {share_wide_flat:.3f} of the flat region, narrow {share_narrow_detail:.3f} of the detail")
    assert share_wide_flat > 0.5 and share_narrow_detail > 0.5


def test_selection_reads_low_at_most(spt):
    """Two candidates: the least of two noisy estimates reads low by selection. Only r < 1 + 5 s.e. is
    asserted; the figure is printed."""
    t = runs(spt, [2.0, 8.0])
    r, se = jackknife(lambda keep: t[keep, 0].mean() / t[keep, 1].mean())
    print(f"two candidates: mse r = {r:.4f}, s.e. {se:.4f}")
    assert r < 1.0 + 5 * se, (r, se)


# ---- 4. the summary -------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_summary_host_equals_float64_numpy(spt, w, h):
    _, mse, choice = spt.denoise_bank_host(*halves(w, h), params_of(spt, CANDS))
    got, want = spt.bank_summary_host(mse, choice), dbt.bank_summary_truth(mse, choice)
    assert abs(got["mse_mean"] - want["mse_mean"]) <= REL_SUM * abs(want["mse_mean"]), (got, want)
    assert abs(got["rmse_est"] - want["rmse_est"]) <= REL_SUM * want["rmse_est"]
    assert got["share"] == want["share"] and abs(sum(got["share"]) - 1) < 1e-12
    assert got["mse_min"] == want["mse_min"] and got["mse_max"] == want["mse_max"]


def test_summary_of_a_negative_mean(spt):
    s = spt.bank_summary_host(np.full((2, 3), -0.5, np.float32), np.zeros((2, 3), np.uint8))
    assert s["mse_mean"] == -0.5 and s["rmse_est"] == 0.0 and s["share"] == [1.0, 0.0, 0.0, 0.0]


# ---- 5. rejections, layout, symbols ---------------------------------------------------------------
def test_rejected_calls_leave_every_output_untouched(spt):
    lib = spt.load_library()
    P = [a.copy() for a in halves(17, 13)]
    w, h = 17, 13
    ok = spt.default_denoise_params
    nan, inf = float("nan"), float("inf")

    def outputs():
        return [np.full((h, w, 3), -7.25, np.float32), np.full((h, w), -7.25, np.float32),
                np.full((h, w), 0xA5, np.uint8)]

    def untouched(o):
        return (o[0] == -7.25).all() and (o[1] == -7.25).all() and (o[2] == 0xA5).all()

    def call(planes, w_, h_, cands, n, bank, out, mse, choice):
        ptr = [a.ctypes.data if a is not None else None for a in planes]
        arr = None
        if cands is not None:
            arr = (spt.spt_denoise_params * 4)()
            for k, c in enumerate(cands):
                ctypes.memmove(ctypes.byref(arr, 32 * k), ctypes.byref(c), 32)
        return lib.spt_denoise_bank_host(*ptr, w_, h_, arr, n, ctypes.byref(bank) if bank is not None else None,
                                         *[o.ctypes.data if o is not None else None for o in (out, mse, choice)])

    def bank(**kw):
        b = spt.default_bank_params()
        for k, v in kw.items():
            if k == "reserved":
                b.reserved[v] = 1
            else:
                setattr(b, k, v)
        return b

    good = [ok(), ok(sigma_color=8.0)]
    cases = [(f"null plane {k}", P[:k] + [None] + P[k + 1:], w, h, good, 2, bank()) for k in range(7)]
    cases += [("null cands", P, w, h, None, 2, bank()), ("null bank", P, w, h, good, 2, None),
              ("n_cands 0", P, w, h, good, 0, bank()), ("n_cands -1", P, w, h, good, -1, bank()),
              ("n_cands 5", P, w, h, good + good, 5, bank()),
              ("error_iterations -1", P, w, h, good, 2, bank(error_iterations=-1)),
              ("error_iterations 4", P, w, h, good, 2, bank(error_iterations=4)),
              ("pair_flags 2", P, w, h, good, 2, bank(pair_flags=2)),
              ("pair_flags high", P, w, h, good, 2, bank(pair_flags=0x80000001)),
              ("reserved 0", P, w, h, good, 2, bank(reserved=0)), ("reserved 1", P, w, h, good, 2, bank(reserved=1)),
              ("width 0", P, 0, h, good, 2, bank()), ("height 0", P, w, 0, good, 2, bank()),
              ("width < 0", P, -w, h, good, 2, bank()), ("too many pixels", P, 65536, 32768, good, 2, bank())]
    bad = [ok(iterations=-1), ok(iterations=7), ok(normal_squarings=9), ok(flags=2), ok(reserved=1)]
    for field in ("sigma_color", "sigma_depth", "sigma_albedo", "albedo_floor"):
        bad += [ok(**{field: v}) for v in (0.0, -1.0, nan, inf)]
    for k, b in enumerate(bad):  # a bad candidate, in every place of the list in turn
        cands = [ok(), ok(), ok(), ok()]
        cands[k % 4] = b
        cases.append((f"bad candidate {k}", P, w, h, cands, 4, bank()))
    for label, planes, w_, h_, cands, n, b in cases:
        o = outputs()
        assert call(planes, w_, h_, cands, n, b, *o) == 1, label
        assert untouched(o), label
        assert lib.spt_last_error(), label
    o = outputs()
    assert call(P, w, h, good, 2, bank(), None, o[1], o[2]) == 1  # a null out
    before = [a.copy() for a in P]
    for k in range(6):  # an output that is an input (the depth plane is too short to try as out)
        for slot in range(3):
            oo = list(o)
            oo[slot] = P[k]
            assert call(P, w, h, good, 2, bank(), *oo) == 1, (k, slot)
    for i, j in ((0, 1), (0, 2), (1, 2)):  # two outputs that are one plane
        oo = list(o)
        oo[j] = oo[i]
        assert call(P, w, h, good, 2, bank(), *oo) == 1, (i, j)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(P, before))
    assert untouched(o)
    # ... and the same arguments in range are accepted, with and without the optional planes
    assert call(P, w, h, good, 2, bank(), o[0], None, None) == 0 and (o[0] != -7.25).all()
    assert (o[1] == -7.25).all() and (o[2] == 0xA5).all()
    assert call(P, w, h, good, 2, bank(), *o) == 0 and (o[1] != -7.25).all() and (o[2] < 2).all()
    s = spt.spt_bank_summary()
    m, c = o[1], o[2]
    assert lib.spt_denoise_bank_summary_host(None, c.ctypes.data, w, h, ctypes.byref(s)) == 1
    assert lib.spt_denoise_bank_summary_host(m.ctypes.data, None, w, h, ctypes.byref(s)) == 1
    assert lib.spt_denoise_bank_summary_host(m.ctypes.data, c.ctypes.data, w, h, None) == 1
    assert lib.spt_denoise_bank_summary_host(m.ctypes.data, c.ctypes.data, 0, h, ctypes.byref(s)) == 1
    assert lib.spt_denoise_bank_summary_host(m.ctypes.data, c.ctypes.data, w, -1, ctypes.byref(s)) == 1
    assert lib.spt_denoise_bank_summary_host(m.ctypes.data, c.ctypes.data, w, h, ctypes.byref(s)) == 0


def test_abi_markers(spt):
    hdr = open(os.path.join(ROOT, "include", "spt.h")).read()
    assert re.search(r"^#define SPT_HAS_DENOISE_BANK 1\b", hdr, re.M)
    assert re.search(r"^#define SPT_BANK_MAX_CANDIDATES 4\b", hdr, re.M)
    assert re.search(r"^#define SPT_ABI_VERSION 6\b", hdr, re.M)
    assert spt.SPT_HAS_DENOISE_BANK == 1 and spt.BANK_MAX_CANDIDATES == 4
    assert ctypes.sizeof(spt.spt_bank_params) == 16 and ctypes.sizeof(spt.spt_bank_summary) == 56
    assert ctypes.sizeof(spt.spt_denoise_params) == 32
    b = spt.default_bank_params()
    assert (b.error_iterations, b.pair_flags, list(b.reserved)) == (2, spt.DENOISE_PAIR_OWN_WEIGHTS, [0, 0])
    lib = spt.load_library()
    for name in ("spt_denoise_bank_default_params", "spt_denoise_bank_async", "spt_denoise_bank_host",
                 "spt_denoise_bank_summary", "spt_denoise_bank_summary_host", "spt_film_pair_denoise_bank"):
        assert name in spt.EXPORTS and hasattr(lib, name)

"""The filter bank on the GPU (include/spt.h SPT_HAS_DENOISE_BANK; spt_denoise.hip): every comparison of
the device kernels is bit for bit against the host statement spt_denoise_bank_host, which
tests/test_denoise_bank.py pins to the header's text.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import denoise_bank_truth as dbt

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, BATCH, GUIDE_SPP = 64, 48, 64, 8, 16
FILL = -7.25
REL_SUM = 1e-9  # tests/test_gpu_film_noise.py's tolerance for the noise summary
# as tests/test_denoise_bank.py: sigma_color and iterations differ, one candidate has no iteration at all
CANDS = [dict(sigma_color=2.0, iterations=5), dict(sigma_color=8.0, iterations=3),
         dict(sigma_color=4.0, iterations=0), dict(sigma_color=1.0, iterations=1, flags=1)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want, label):
    diff = np.argwhere(bits(got) != bits(want))
    assert diff.size == 0, f"{label}: {len(diff)} values differ, first at {diff[:3].tolist()}: " \
                           f"{[(float(got[tuple(i)]), float(want[tuple(i)])) for i in diff[:3]]}"


def _aspect(w, h):
    return float(np.float32(w) / np.float32(h))


def _upload(torch, planes):
    return [torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1)).cuda() for a in planes]


def _guarded(torch, w, h):
    """out, mse and choice on the device, each one element longer than needed: NaN, NaN and 0xA5."""
    n = w * h
    return [torch.full((3 * n + 1,), float("nan"), dtype=torch.float32, device="cuda"),
            torch.full((n + 1,), float("nan"), dtype=torch.float32, device="cuda"),
            torch.full((n + 1,), 0xA5, dtype=torch.uint8, device="cuda")]


def _params(spt, cands):
    return [spt.default_denoise_params(**c) for c in cands]


def _close(a, b, rel):
    return abs(a - b) <= rel * max(abs(a), abs(b))


# ---- 1. device equals host on synthetic halves ----------------------------------------------------
SYNTH_SIZES = [(1, 1), (33, 9), (70, 50), (300, 4), (4, 300)]


@pytest.mark.parametrize("w,h", SYNTH_SIZES, ids=[f"{w}x{h}" for w, h in SYNTH_SIZES])
def test_device_equals_host_on_synthetic_halves(spt, w, h):
    import torch
    planes = dbt.bank_halves(w, h)
    dev = _upload(torch, planes)
    ptr = [t.data_ptr() for t in dev]
    n = w * h
    dn = spt.Denoiser(w, h, 0)
    try:
        for pf in (0, spt.DENOISE_PAIR_OWN_WEIGHTS):
            for nc in (1, 2, 4):
                for ei in (0, 1, 3):
                    arr, cnt, bank = spt._bank_args(_params(spt, CANDS[:nc]), None, pf, ei)
                    bufs = _guarded(torch, w, h)
                    dn.denoise_bank_async(*ptr, arr, cnt, bank, *[b.data_ptr() for b in bufs])
                    torch.cuda.synchronize()
                    got = [b.cpu().numpy() for b in bufs]
                    assert np.isnan(got[0][3 * n]) and np.isnan(got[1][n]) and got[2][n] == 0xA5, \
                        "a write past a plane"
                    want = spt.denoise_bank_host(*planes, _params(spt, CANDS[:nc]), None, pf, ei)
                    label = f"{w}x{h} n_cands={nc} error_iterations={ei} pair_flags={pf}"
                    same(got[0][:3 * n].reshape(h, w, 3), want[0], f"out {label}")
                    same(got[1][:n].reshape(h, w), want[1], f"mse {label}")
                    assert np.array_equal(got[2][:n].reshape(h, w), want[2]), f"choice {label}"
                    only = _guarded(torch, w, h)  # mse and choice left out
                    dn.denoise_bank_async(*ptr, arr, cnt, bank, only[0].data_ptr(), 0, 0)
                    torch.cuda.synchronize()
                    only = only[0].cpu().numpy()
                    assert np.isnan(only[3 * n])
                    same(only[:3 * n].reshape(h, w, 3), want[0], f"out alone {label}")
    finally:
        dn.close()


def test_one_candidate_is_the_pair_filter_on_the_device(spt):
    planes = dbt.bank_halves(70, 50)
    dn = spt.Denoiser(70, 50, 0)
    try:
        for own in (False, True):
            p = spt.default_denoise_params(iterations=2)
            pair_out = dn.denoise_pair(*planes, p, own)[0]
            out, _mse, choice = dn.denoise_bank(*planes, [p], None, own)
            same(out, pair_out, f"own={own}")
            assert not choice.any()
    finally:
        dn.close()


# ---- 2. the summary -------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (17, 13), (70, 50), (640, 103)], ids=lambda v: str(v))
def test_summary_device_equals_host_and_repeats(spt, w, h):
    rng = np.random.default_rng(w * 1000 + h)
    mse = (rng.normal(1e-4, 5e-4, (h, w)) * rng.random((h, w))).astype(np.float32)
    choice = rng.integers(0, 4, (h, w)).astype(np.uint8)
    dn = spt.Denoiser(w, h, 0)
    try:
        one, two = dn.bank_summary(mse, choice), dn.bank_summary(mse, choice)
    finally:
        dn.close()
    host = spt.bank_summary_host(mse, choice)
    assert one == two, "two device runs differ"
    assert _close(one["mse_mean"], host["mse_mean"], REL_SUM), (one, host)
    assert _close(one["rmse_est"], host["rmse_est"], REL_SUM)
    assert one["share"] == host["share"] == [float((choice == k).sum() / (w * h)) for k in range(4)]
    assert one["mse_min"] == host["mse_min"] == float(mse.min())
    assert one["mse_max"] == host["mse_max"] == float(mse.max())


# ---- 3. the film path -----------------------------------------------------------------------------
def _pair_session(spt, prims, seed=5):
    """-> (renderer, film A, film B, guide, params, cam): 64x48, 64 spp in batches of 8, even batches in A
    and odd ones in B (four each), a guide of GUIDE_SPP samples."""
    p = spt.default_params(width=W, height=H, spp=SPP, seed=seed)
    cam = spt.Camera(aspect=_aspect(W, H))
    r, fa, fb, guide = spt.Renderer(0), spt.Film(p, 0), spt.Film(p, 0), spt.Guide(p, 0)
    for f in (fa, fb):
        f.enable_noise(BATCH)
    for k in range(SPP // BATCH):
        (fb if k & 1 else fa).render(r, prims, cam, p, k * BATCH, BATCH)
        r.stats()
    guide.render(r, prims, cam, p, 0, GUIDE_SPP)
    return r, fa, fb, guide, p, cam


def test_film_bank_equals_the_separate_calls_and_the_host(spt):
    prims = spt.cornell_scene()
    r, fa, fb, guide, p, cam = _pair_session(spt, prims)
    dn = spt.Denoiser(W, H, 0)
    try:
        state = [fa.to_numpy(), fa.noise_to_numpy(), fb.to_numpy(), fb.noise_to_numpy(), guide.to_numpy()]
        g = guide.resolve()
        planes = [fa.resolve(), fa.noise_map(), fb.resolve(), fb.noise_map(), g["albedo"], g["normal"], g["depth"]]
        cands = spt.bank_candidates((2.0, 4.0, 8.0))
        for own in (True, False):
            fused = dn.denoise_film_bank(fa, fb, guide, cands, None, own, return_summary=True)
            apart = dn.denoise_bank(*planes, cands, None, own)
            want = spt.denoise_bank_host(*planes, cands, None, own)
            for k, name in enumerate(("out", "mse", "choice")):
                same(fused[k].astype(np.float32), apart[k].astype(np.float32), f"{name}: film vs planes, own={own}")
                same(fused[k].astype(np.float32), want[k].astype(np.float32), f"{name}: film vs host, own={own}")
            assert len(np.unique(fused[2])) > 1, "more than one candidate is chosen on a render"
            host_summary = spt.bank_summary_host(want[1], want[2])
            assert fused[3]["share"] == host_summary["share"]
            assert _close(fused[3]["mse_mean"], host_summary["mse_mean"], REL_SUM)
        after = [fa.to_numpy(), fa.noise_to_numpy(), fb.to_numpy(), fb.noise_to_numpy(), guide.to_numpy()]
        assert all(np.array_equal(a, b) for a, b in zip(state, after)), "the bank only reads the films"
    finally:
        for o in (dn, guide, fa, fb, r):
            o.close()


def test_the_single_and_pair_filters_do_not_notice_the_bank(spt):
    """spt_film_denoise and spt_film_pair_denoise give the same bits before and after the first bank call
    on one denoiser; create, bank and destroy twice."""
    prims = spt.cornell_scene()
    r, fa, fb, guide, p, cam = _pair_session(spt, prims)
    try:
        banks = []
        for _round in range(2):
            dn = spt.Denoiser(W, H, 0)
            try:
                single = dn.denoise_film(fa, guide, return_se=True)
                pair = dn.denoise_film_pair(fa, fb, guide)
                banks.append(dn.denoise_film_bank(fa, fb, guide, spt.bank_candidates((2.0, 8.0))))
                single2 = dn.denoise_film(fa, guide, return_se=True)
                pair2 = dn.denoise_film_pair(fa, fb, guide)
                for a, b in zip(single + pair, single2 + pair2):
                    same(a, b, "around the first bank call")
                again = dn.denoise_film_bank(fa, fb, guide, spt.bank_candidates((2.0, 8.0)))
                for a, b in zip(banks[-1], again):
                    same(a.astype(np.float32), b.astype(np.float32), "the bank twice on one denoiser")
            finally:
                dn.close()
        for a, b in zip(*banks):
            same(a.astype(np.float32), b.astype(np.float32), "the bank on two denoisers")
    finally:
        for o in (guide, fa, fb, r):
            o.close()


# ---- 4. rejected calls ----------------------------------------------------------------------------
def test_rejected_calls_queue_nothing_and_leave_the_outputs_untouched(spt):
    import torch
    lib = spt.load_library()
    prims = spt.cornell_scene()
    r, fa, fb, guide, p, cam = _pair_session(spt, prims)
    planes = dbt.bank_halves(W, H)
    dev = _upload(torch, planes)
    ptr = [t.data_ptr() for t in dev]
    n = W * H
    outs = [torch.full((3 * n,), FILL, dtype=torch.float32, device="cuda"),
            torch.full((n,), FILL, dtype=torch.float32, device="cuda"),
            torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")]
    o = [t.data_ptr() for t in outs]
    dn, small = spt.Denoiser(W, H, 0), spt.Denoiser(W - 1, H, 0)
    ok = spt.default_denoise_params
    nan, inf = float("nan"), float("inf")
    bad_params = [ok(iterations=-1), ok(iterations=7), ok(normal_squarings=9), ok(flags=2), ok(reserved=1)]
    bad_params += [ok(**{f: v}) for f in ("sigma_color", "sigma_depth", "sigma_albedo", "albedo_floor")
                   for v in (0.0, -1.0, nan, inf)]
    plain = spt.Film(p, 0)
    p2 = spt.default_params(width=W, height=H, spp=SPP, seed=5, shard_index=0, shard_count=2, tile_rows=8)
    shard_film = spt.Film(p2, 0)
    shard_film.enable_noise(BATCH)
    for k in range(2):
        shard_film.render(r, prims, cam, p2, k * BATCH, BATCH)
    empty_guide = spt.Guide(p, 0)

    def args(cands, **kw):
        arr, cnt, bank = spt._bank_args(cands, None, True, None)
        for k, v in kw.items():
            if k == "reserved":
                bank.reserved[v] = 1
            elif k == "n":
                cnt = v
            else:
                setattr(bank, k, v)
        return arr, cnt, bank

    def untouched():
        torch.cuda.synchronize()
        return bool((outs[0] == FILL).all()) and bool((outs[1] == FILL).all()) and bool((outs[2] == 0xA5).all())

    def refused(call, label):
        with pytest.raises(spt.SptError) as e:
            call()
        assert e.value.status == 1, label
        assert untouched(), label

    good = [ok(), ok(sigma_color=8.0)]
    try:
        for k in range(7):
            a = list(ptr)
            a[k] = 0
            refused(lambda: dn.denoise_bank_async(*a, *args(good), *o), f"null plane {k}")
            for slot in range(3):
                oo = list(o)
                oo[slot] = ptr[k]
                refused(lambda: dn.denoise_bank_async(*ptr, *args(good), *oo), f"output {slot} is input {k}")
        refused(lambda: dn.denoise_bank_async(*ptr, *args(good), 0, o[1], o[2]), "null out")
        for i, j in ((0, 1), (0, 2), (1, 2)):
            oo = list(o)
            oo[j] = oo[i]
            refused(lambda: dn.denoise_bank_async(*ptr, *args(good), *oo), f"outputs {i} and {j} are one plane")
            refused(lambda: dn.denoise_film_bank_async(fa, fb, guide, *args(good), *oo), f"film: outputs {i}, {j}")
        bad_bank = [dict(n=0), dict(n=-1), dict(n=5), dict(error_iterations=-1), dict(error_iterations=4),
                    dict(pair_flags=2), dict(pair_flags=0x80000001), dict(reserved=0), dict(reserved=1)]
        for kw in bad_bank:
            refused(lambda: dn.denoise_bank_async(*ptr, *args(good + good, **kw), *o), f"bank {kw}")
            refused(lambda: dn.denoise_film_bank_async(fa, fb, guide, *args(good + good, **kw), *o), f"film bank {kw}")
        for i, bp in enumerate(bad_params):
            cands = [ok(), ok(), ok(), ok()]
            cands[i % 4] = bp
            refused(lambda: dn.denoise_bank_async(*ptr, *args(cands), *o), f"candidate {i}")
            refused(lambda: dn.denoise_film_bank_async(fa, fb, guide, *args(cands), *o), f"film candidate {i}")
        V = ctypes.c_void_p
        null = V(None)
        ins, oo = [V(x) for x in ptr], [V(x) for x in o]
        arr, cnt, bank = args(good)
        assert lib.spt_denoise_bank_async(dn._d, *ins, None, 2, ctypes.byref(bank), *oo, null) == 1
        assert lib.spt_denoise_bank_async(dn._d, *ins, arr, 2, None, *oo, null) == 1
        assert lib.spt_denoise_bank_async(null, *ins, arr, 2, ctypes.byref(bank), *oo, null) == 1
        for a, b, g, d, label in [(fa, fa, guide, dn, "one film twice"), (plain, fb, guide, dn, "a plain film"),
                                  (fa, shard_film, guide, dn, "a sharded film"),
                                  (fa, fb, empty_guide, dn, "an empty guide"),
                                  (fa, fb, guide, small, "the denoiser's size")]:
            refused(lambda: d.denoise_film_bank_async(a, b, g, *args(good), *o), label)
        assert lib.spt_film_pair_denoise_bank(null, fb._f, guide._g, dn._d, arr, 2, ctypes.byref(bank), *oo, null) == 1
        assert lib.spt_film_pair_denoise_bank(fa._f, fb._f, null, dn._d, arr, 2, ctypes.byref(bank), *oo, null) == 1
        s = spt.spt_bank_summary()
        assert lib.spt_denoise_bank_summary(null, oo[1], oo[2], ctypes.byref(s), null) == 1
        assert lib.spt_denoise_bank_summary(dn._d, null, oo[2], ctypes.byref(s), null) == 1
        assert lib.spt_denoise_bank_summary(dn._d, oo[1], null, ctypes.byref(s), null) == 1
        assert lib.spt_denoise_bank_summary(dn._d, oo[1], oo[2], None, null) == 1
        assert untouched()
        # ... and the same arguments in range are accepted
        dn.denoise_film_bank_async(fa, fb, guide, *args(good), *o)
        torch.cuda.synchronize()
        assert bool((outs[0] != FILL).all()) and bool((outs[1] != FILL).all()) and bool((outs[2] < 2).all())
    finally:
        for x in (dn, small, plain, shard_film, empty_guide, guide, fa, fb, r):
            x.close()


# ---- 5. the Python wrappers -----------------------------------------------------------------------
def test_wrappers_equal_the_explicit_calls(spt):
    prims = spt.cornell_scene()
    r, fa, fb, guide, p, cam = _pair_session(spt, prims, seed=1)
    dn = spt.Denoiser(W, H, 0)
    try:
        # render_denoised_bank's defaults: own weights, three smoothing passes
        want = dn.denoise_film_bank(fa, fb, guide, spt.bank_candidates((2.0, 4.0, 8.0)), None, True, 3,
                                    return_summary=True)
        want2 = dn.denoise_film_bank(fa, fb, guide, spt.bank_candidates((1.0, 16.0)), None, False, 1)
    finally:
        for o in (dn, guide, fa, fb, r):
            o.close()
    p = spt.default_params(width=W, height=H, spp=SPP, seed=1)
    got, info = spt.render_denoised_bank(prims, cam, p, guide_spp=GUIDE_SPP, return_info=True)
    same(got, want[0], "render_denoised_bank")
    same(info["mse"], want[1], "mse")
    assert np.array_equal(info["choice"], want[2]) and info["bank"] == want[3]
    got2 = spt.render_denoised_bank(prims, cam, p, (1.0, 16.0), guide_spp=GUIDE_SPP, own_weights=False,
                                    error_iterations=1)
    same(got2, want2[0], "render_denoised_bank with other arguments")
    # render_denoised_until(estimate="bank"): a huge target stops at min_batches, target 0 renders every batch
    out, u = spt.render_denoised_until(prims, cam, p, 1e9, guide_spp=GUIDE_SPP, estimate="bank")
    assert u["batches_done"] == 4 and u["rmse"] == u["bank"]["rmse_est"] > 0
    out, u = spt.render_denoised_until(prims, cam, p, 0.0, guide_spp=GUIDE_SPP, estimate="bank")
    assert u["batches_done"] == SPP // BATCH
    same(out, want[0], "render_denoised_until(estimate='bank', target 0) vs render_denoised_bank")
    assert u["rmse"] == want[3]["rmse_est"]
    with pytest.raises(spt.SptError):
        spt.render_denoised_until(prims, cam, p, 0.0, estimate="other")


def test_the_dropin_program_equals_render_denoised_bank(spt, tmp_path):
    """smallpt_amd --denoise --pair --bank 2,8 --bank-map PREFIX: the image, the mse and the choice planes
    are render_denoised_bank's (the program's guide takes min(SPP, 64) samples)."""
    prims = spt.cornell_scene()
    cam = spt.Camera(aspect=_aspect(W, H))
    p32 = spt.default_params(width=W, height=H, spp=32, seed=1)
    want, info = spt.render_denoised_bank(prims, cam, p32, (2.0, 8.0), guide_spp=32, return_info=True)
    exe = os.path.join(ROOT, "small-pathtracer_amd", "smallpt_amd")
    out_path, prefix = tmp_path / "b.pfm", tmp_path / "map"
    run = subprocess.run([exe, str(W), str(H), "32", "1", str(out_path), "--pfm", "--denoise", "--pair", "--bank",
                          "2,8", "--bank-map", str(prefix)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "BANK : " in run.stdout

    def pfm(path):
        raw = open(path, "rb").read()
        return np.frombuffer(raw[len(raw) - W * H * 12:], dtype="<f4").reshape(H, W, 3)[::-1]

    same(pfm(out_path), want, "smallpt_amd --bank --pfm")
    same(pfm(str(prefix) + "_mse.pfm")[..., 0], info["mse"], "the mse map")
    raw = open(str(prefix) + "_choice.pgm", "rb").read()
    assert raw.startswith(b"P5\n%d %d\n255\n" % (W, H))
    assert np.array_equal(np.frombuffer(raw[-W * H:], np.uint8).reshape(H, W), info["choice"] * 85)
    for bad in (["--bank", "2,8"], ["--denoise", "--pair", "--bank", "2,x"], ["--denoise", "--pair", "--bank", "1,2,3,4,5"],
                ["--denoise", "--pair", "--bank", "2,8", "--denoise-sigma", "3"], ["--denoise", "--pair", "--bank-map", "m"]):
        r = subprocess.run([exe, str(W), str(H), "32", "1", str(tmp_path / "x.pfm")] + bad, capture_output=True,
                           text=True, timeout=120)
        assert r.returncode != 0 and "--bank" in r.stderr, bad
    usage = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--bank" in usage and "--bank-map" in usage

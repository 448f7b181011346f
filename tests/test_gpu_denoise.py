"""The a-trous filter on the GPU (include/spt.h SPT_HAS_DENOISE; spt_denoise.hip): every comparison
of the device kernels is bit for bit against the host statement spt_denoise_host, which
tests/test_denoise.py pins to the header's text.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import denoise_truth as dt

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, BATCH, GUIDE_SPP = 64, 48, 64, 8, 16
FILL = -7.25


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want, label):
    diff = np.argwhere(bits(got) != bits(want))
    assert diff.size == 0, f"{label}: {len(diff)} values differ, first at {diff[:3].tolist()}: " \
                           f"{[(float(got[tuple(i)]), float(want[tuple(i)])) for i in diff[:3]]}"


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def _aspect(w, h):
    return float(np.float32(w) / np.float32(h))


def _upload(torch, planes):
    return [torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1)).cuda() for a in planes]


def _guarded(torch, n):
    """A device buffer one float longer than needed, all NaN."""
    return torch.full((n + 1,), float("nan"), dtype=torch.float32, device="cuda")


# ---- 1. device equals host on synthetic planes ----------------------------------------------------
SYNTH_SIZES = [(1, 1), (3, 2), (17, 13), (70, 50), (300, 4), (4, 300)]


@pytest.mark.parametrize("w,h", SYNTH_SIZES, ids=[f"{w}x{h}" for w, h in SYNTH_SIZES])
def test_device_equals_host_on_synthetic_planes(spt, w, h):
    import torch
    s = dt.synthetic(w, h)
    planes = dt.planes_of(s)
    dev = _upload(torch, planes)
    n = w * h * 3
    dn = spt.Denoiser(w, h, 0)
    try:
        for flags in (0, spt.DENOISE_NO_DEMODULATE):
            for it in (0, 1, 2, 3, 6):
                p = spt.default_denoise_params(iterations=it, flags=flags)
                out, se_out = _guarded(torch, n), _guarded(torch, n)
                dn.denoise_async(*[t.data_ptr() for t in dev], p, out.data_ptr(), se_out.data_ptr())
                torch.cuda.synchronize()
                out, se_out = out.cpu().numpy(), se_out.cpu().numpy()
                assert np.isnan(out[n]) and np.isnan(se_out[n]), "a write past the plane"
                want, want_se = spt.denoise_host(*planes, p, return_se=True)
                same(out[:n].reshape(h, w, 3), want, f"out {w}x{h} it={it} flags={flags}")
                same(se_out[:n].reshape(h, w, 3), want_se, f"se_out {w}x{h} it={it} flags={flags}")
                only = _guarded(torch, n)  # se_out left out
                dn.denoise_async(*[t.data_ptr() for t in dev], p, only.data_ptr(), 0)
                torch.cuda.synchronize()
                same(only.cpu().numpy()[:n].reshape(h, w, 3), want, "out without se_out")
    finally:
        dn.close()


# ---- 2. device equals host on a real render -------------------------------------------------------
def _render_session(spt, prims, seed=5, adaptive=False, spp=SPP, batch=BATCH):
    """-> (renderer, film, guide, params, cam): 64x48, every batch in, a guide of GUIDE_SPP samples; an
    adaptive film has had one selection after four batches."""
    p = spt.default_params(width=W, height=H, spp=spp, seed=seed)
    cam = spt.Camera(aspect=_aspect(W, H))
    r, film, guide = spt.Renderer(0), spt.Film(p, 0), spt.Guide(p, 0)
    film.enable_noise(batch)
    if adaptive:
        film.enable_adaptive()
    for k in range(spp // batch):
        if adaptive and k == 4:
            left = film.adaptive_select(0.02)
            assert 0 < left < W * H
        film.render(r, prims, cam, p, k * batch, batch)
        r.stats()
    guide.render(r, prims, cam, p, 0, GUIDE_SPP)
    return r, film, guide, p, cam


def _host_planes(spt, film, guide, adaptive):
    """The five planes by the existing host statements, from the downloaded sums, moments, records."""
    fi, ni, gi = film.info(), film.noise_info(), guide.info()
    sums, m2 = film.to_numpy(), film.noise_to_numpy()
    if adaptive:
        counts = film.counts_to_numpy()
        rgb = spt.film_adaptive_resolve_host(sums, counts, fi["width"], fi["rows"], fi["spp_total"], ni["batch"])
        se = spt.film_adaptive_noise_map_host(sums, m2, counts, fi["width"], fi["rows"], fi["spp_total"],
                                              ni["batch"])
    else:
        rgb = spt.film_resolve_host(sums, fi["width"], fi["rows"], fi["spp_total"], fi["samples_done"])
        se = spt.film_noise_map_host(sums, m2, fi["width"], fi["rows"], fi["spp_total"], fi["samples_done"],
                                     ni["batch"], ni["batches_done"])
    g = spt.guide_resolve_host(guide.to_numpy(), gi["width"], gi["rows"], gi["spp_total"], gi["samples_done"])
    return [rgb, se, g["albedo"], g["normal"], g["depth"]]


@pytest.mark.parametrize("scene,adaptive", [("head", False), ("spheres32", False), ("head", True)],
                         ids=["head", "spheres32", "head_adaptive"])
def test_film_denoise_equals_the_separate_calls_and_the_host(spt, scene, adaptive):
    prims = spt.cornell_scene() if scene == "head" else spt.spheres32_scene()
    r, film, guide, p, cam = _render_session(spt, prims, adaptive=adaptive)
    dn = spt.Denoiser(W, H, 0)
    try:
        sums, rec = film.to_numpy(), guide.to_numpy()
        fused, fused_se = dn.denoise_film(film, guide, return_se=True)
        g = guide.resolve()
        planes = [film.resolve(), film.noise_map(), g["albedo"], g["normal"], g["depth"]]
        apart, apart_se = dn.denoise(*planes, return_se=True)
        same(fused, apart, "film_denoise vs denoise_async")
        same(fused_se, apart_se, "se_out: film_denoise vs denoise_async")
        host_planes = _host_planes(spt, film, guide, adaptive)
        for a, b, name in zip(planes, host_planes, dt.PLANES):
            same(a, b, f"resolved plane {name}")
        want, want_se = spt.denoise_host(*host_planes, return_se=True)
        same(fused, want, "film_denoise vs host")
        same(fused_se, want_se, "se_out: film_denoise vs host")
        # the denoise read the film and the guide, and only read them
        assert np.array_equal(film.to_numpy(), sums) and np.array_equal(guide.to_numpy(), rec)
        assert (fused != planes[0]).any()
    finally:
        dn.close()
        guide.close()
        film.close()
        r.close()


# ---- 3. determinism and isolation -----------------------------------------------------------------
def test_two_runs_give_the_same_bits_and_a_context_does_not_notice(spt):
    import torch
    prims = spt.cornell_scene()
    r, film, guide, p, cam = _render_session(spt, prims)
    dn = spt.Denoiser(W, H, 0)
    frame = spt.default_params(width=W, height=H, spp=4, seed=9)
    keys = [k for k in spt.STAT_KEYS]

    def frames(with_denoise):
        got = []
        for k, prm in enumerate((frame, spt.default_params(width=W, height=H, spp=4, seed=10))):
            buf = torch.zeros(W * H * 3, dtype=torch.float32, device="cuda")
            r.render_async(prims, cam, prm, buf.data_ptr())
            if with_denoise and k == 0:
                got.append(dn.denoise_film(film, guide))
            torch.cuda.synchronize()
            st = r.stats()
            got.append((buf.cpu().numpy(), [st[x] for x in keys], r.kernel()))
        return got

    try:
        a = frames(True)
        b = frames(False)
        again = dn.denoise_film(film, guide)
        same(a[0], again, "two runs")
        for (img_a, st_a, k_a), (img_b, st_b, k_b) in zip(a[1:], b):
            assert np.array_equal(img_a, img_b) and st_a == st_b and k_a == k_b
    finally:
        dn.close()
        guide.close()
        film.close()
        r.close()


# ---- 4. rejected calls ----------------------------------------------------------------------------
def test_rejected_calls_leave_out_untouched(spt):
    import torch
    lib = spt.load_library()
    prims = spt.cornell_scene()
    r, film, guide, p, cam = _render_session(spt, prims)
    s = dt.synthetic(W, H)
    dev = _upload(torch, dt.planes_of(s))
    n = W * H * 3
    out = torch.full((n,), FILL, dtype=torch.float32, device="cuda")
    se_out = torch.full((n,), FILL, dtype=torch.float32, device="cuda")
    dn, small = spt.Denoiser(W, H, 0), spt.Denoiser(W - 1, H, 0)
    ok = spt.default_denoise_params
    nan, inf = float("nan"), float("inf")
    bad_params = [ok(iterations=-1), ok(iterations=7), ok(normal_squarings=-1), ok(normal_squarings=9),
                  ok(flags=2), ok(flags=0x80000001), ok(reserved=1)]
    bad_params += [ok(**{f: v}) for f in ("sigma_color", "sigma_depth", "sigma_albedo", "albedo_floor")
                   for v in (0.0, -1.0, nan, inf)]
    plain = spt.Film(p, 0)
    young = spt.Film(p, 0)
    young.enable_noise(BATCH)
    young.render(r, prims, cam, p, 0, BATCH)
    empty_guide = spt.Guide(p, 0)
    p2 = spt.default_params(width=W, height=H, spp=SPP, seed=5, shard_index=0, shard_count=2, tile_rows=8)
    shard_film, shard_guide = spt.Film(p2, 0), spt.Guide(p2, 0)
    shard_film.enable_noise(BATCH)
    for k in range(2):
        shard_film.render(r, prims, cam, p2, k * BATCH, BATCH)
    shard_guide.render(r, prims, cam, p2, 0, GUIDE_SPP)
    ptr = [t.data_ptr() for t in dev]

    def refused(call, label):
        with pytest.raises(spt.SptError) as e:
            call()
        assert e.value.status == 1, label
        torch.cuda.synchronize()
        assert bool((out == FILL).all()) and bool((se_out == FILL).all()), label

    try:
        for k in range(5):
            a = list(ptr)
            a[k] = 0
            refused(lambda: dn.denoise_async(*a, ok(), out.data_ptr(), se_out.data_ptr()), f"null plane {k}")
            refused(lambda: dn.denoise_async(*ptr, ok(), ptr[k], se_out.data_ptr()), f"out is input {k}")
            refused(lambda: dn.denoise_async(*ptr, ok(), out.data_ptr(), ptr[k]), f"se_out is input {k}")
        refused(lambda: dn.denoise_async(*ptr, ok(), 0, se_out.data_ptr()), "null out")
        refused(lambda: dn.denoise_async(*ptr, ok(), out.data_ptr(), out.data_ptr()), "out is se_out")
        for i, bp in enumerate(bad_params):
            refused(lambda: dn.denoise_async(*ptr, bp, out.data_ptr(), se_out.data_ptr()), f"params {i}")
            refused(lambda: dn.denoise_film_async(film, guide, bp, out.data_ptr(), se_out.data_ptr()),
                    f"film params {i}")
        null = ctypes.c_void_p(None)
        V = ctypes.c_void_p
        assert lib.spt_denoise_async(dn._d, *[V(x) for x in ptr], None, V(out.data_ptr()), null, null) == 1
        assert lib.spt_denoise_async(null, *[V(x) for x in ptr], ctypes.byref(ok()), V(out.data_ptr()), null,
                                     null) == 1
        for f, g, d, label in [(plain, guide, dn, "a plain film"), (young, guide, dn, "one batch"),
                               (film, empty_guide, dn, "an empty guide"), (film, guide, small, "sizes"),
                               (shard_film, guide, dn, "a sharded film"),
                               (film, shard_guide, dn, "a sharded guide")]:
            refused(lambda: d.denoise_film_async(f, g, ok(), out.data_ptr(), se_out.data_ptr()), label)
        refused(lambda: dn.denoise_film_async(film, guide, ok(), 0, se_out.data_ptr()), "film: null out")
        assert lib.spt_film_denoise(null, guide._g, dn._d, ctypes.byref(ok()), V(out.data_ptr()), null, null) == 1
        assert lib.spt_film_denoise(film._f, null, dn._d, ctypes.byref(ok()), V(out.data_ptr()), null, null) == 1
        assert lib.spt_film_denoise(film._f, guide._g, null, ctypes.byref(ok()), V(out.data_ptr()), null, null) == 1
        torch.cuda.synchronize()
        assert bool((out == FILL).all())
        for w, h in [(0, 4), (4, 0), (-1, 4), (65536, 32768), (1, 67108861), (2**30, 1)]:
            with pytest.raises(spt.SptError) as e:
                spt.Denoiser(w, h, 0)
            assert e.value.status == 1
        # ... and the same arguments in range are accepted
        dn.denoise_film_async(film, guide, ok(), out.data_ptr(), se_out.data_ptr())
        torch.cuda.synchronize()
        assert bool((out != FILL).all()) and bool((se_out != FILL).all())
    finally:
        for o in (dn, small, plain, young, empty_guide, shard_film, shard_guide, guide, film, r):
            o.close()


# ---- 5. quality -----------------------------------------------------------------------------------
QUALITY_SEEDS = (1, 2, 3, 4)
# rmse(denoised) / rmse(noisy) against the 8192-spp truth, measured on an MI355X with the default
# parameters (profiles/r19_denoise.json, "test_quality"); every value is bit-deterministic.
MEASURED_RATIO = {1: 0.471978, 2: 0.478238, 3: 0.474328, 4: 0.475560}
_truth = {}


def _truth_image(spt):
    if "img" not in _truth:
        p = spt.default_params(width=W, height=H, spp=8192, seed=77)
        _truth["img"] = spt.render(spt.cornell_scene(), spt.Camera(aspect=_aspect(W, H)), p)
    return _truth["img"]


@pytest.mark.parametrize("seed", QUALITY_SEEDS)
def test_denoised_is_closer_to_the_truth(spt, seed):
    """HEAD at 64x48, 64 spp in batches of 8, a guide of 16 samples; the truth is the library's own
    8192-spp render with another seed (its own error is about 1/11 of the noisy image's). Hard
    condition: the denoised RMSE is strictly below the noisy one and the image mean moves by at most
    2 %. Pinned: the ratio per seed is at most the value measured on the GPU x 1.25 (the margin is for
    later deliberate changes of the defaults). Measured, seeds 1..4: ratios 0.471978, 0.478238,
    0.474328, 0.475560 (noisy RMSE 0.1448, 0.1445, 0.1456, 0.1477), the mean moved by 0.29, 0.28, 0.52
    and 0.42 %."""
    truth = _truth_image(spt)
    r, film, guide, p, cam = _render_session(spt, spt.cornell_scene(), seed=seed)
    dn = spt.Denoiser(W, H, 0)
    try:
        noisy = film.resolve()
        den = dn.denoise_film(film, guide)
    finally:
        dn.close()
        guide.close()
        film.close()
        r.close()
    e_noisy, e_den = rmse(noisy, truth), rmse(den, truth)
    mean_shift = abs(float(den.mean(dtype=np.float64)) / float(noisy.mean(dtype=np.float64)) - 1.0)
    print(f"seed {seed}: rmse noisy {e_noisy:.6f} denoised {e_den:.6f} ratio {e_den / e_noisy:.6f} "
          f"mean shift {mean_shift:.6f}")
    assert e_den < e_noisy
    assert mean_shift <= 0.02
    assert e_den / e_noisy <= MEASURED_RATIO[seed] * 1.25


# ---- 6. the Python wrapper and the drop-in program ------------------------------------------------
def test_render_denoised_and_the_dropin_program_equal_the_explicit_calls(spt, tmp_path):
    prims = spt.cornell_scene()
    r, film, guide, p, cam = _render_session(spt, prims, seed=1)
    dn = spt.Denoiser(W, H, 0)
    try:
        noisy = film.resolve()
        want, want_se = dn.denoise_film(film, guide, return_se=True)
        want3 = dn.denoise_film(film, guide, spt.default_denoise_params(iterations=3, sigma_color=2.0))
        summary = film.noise_summary()
        planes = guide.resolve()
    finally:
        dn.close()
        guide.close()
        film.close()
        r.close()
    p = spt.default_params(width=W, height=H, spp=SPP, seed=1)
    got, info = spt.render_denoised(prims, cam, p, guide_spp=GUIDE_SPP, return_info=True)
    same(got, want, "render_denoised")
    same(info["se"], want_se, "render_denoised se")
    same(info["noisy"], noisy, "render_denoised noisy")
    assert info["noise"] == summary
    for k in planes:
        same(info["guides"][k], planes[k], f"render_denoised guide {k}")
    same(spt.render_denoised(prims, cam, p, batch=BATCH, guide_spp=GUIDE_SPP,
                             denoise=spt.default_denoise_params(iterations=3, sigma_color=2.0)), want3,
         "render_denoised with parameters")
    # the program's guide takes min(SPP, 64) samples: SPP = 16 makes that the 16 of this file
    p16 = spt.default_params(width=W, height=H, spp=16, seed=1)
    want16 = spt.render_denoised(prims, cam, p16, guide_spp=16,
                                 denoise=spt.default_denoise_params(iterations=3, sigma_color=2.0))
    exe = os.path.join(ROOT, "small-pathtracer_amd", "smallpt_amd")
    out = tmp_path / "d.pfm"
    run = subprocess.run([exe, str(W), str(H), "16", "1", str(out), "--pfm", "--denoise",
                          "--denoise-iters", "3", "--denoise-sigma", "2"], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    raw = out.read_bytes()
    data = np.frombuffer(raw[len(raw) - W * H * 12:], dtype="<f4").reshape(H, W, 3)[::-1]
    same(data, want16, "smallpt_amd --denoise --pfm")
    bad = subprocess.run([exe, str(W), str(H), "16", "1", str(out), "--denoise", "--devices", "2"],
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "--denoise" in bad.stderr
    usage = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert all(f in usage for f in ("--denoise", "--denoise-iters", "--denoise-sigma"))

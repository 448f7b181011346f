"""The two-half a-trous filter on the GPU (include/spt.h SPT_HAS_DENOISE_PAIR; spt_denoise.hip): every
comparison of the device kernels is bit for bit against the host statement spt_denoise_pair_host, which
tests/test_denoise_pair.py pins to the header's text.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import denoise_pair_truth as dpt

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, BATCH, GUIDE_SPP = 64, 48, 64, 8, 16
FILL = -7.25
REL_SUM = 1e-9  # tests/test_gpu_film_noise.py's tolerance for the noise summary


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


def _close(a, b, rel):
    return abs(a - b) <= rel * max(abs(a), abs(b))


# ---- 1. device equals host on synthetic halves ----------------------------------------------------
SYNTH_SIZES = [(1, 1), (3, 2), (17, 13), (70, 50), (300, 4), (4, 300)]


@pytest.mark.parametrize("w,h", SYNTH_SIZES, ids=[f"{w}x{h}" for w, h in SYNTH_SIZES])
def test_device_equals_host_on_synthetic_halves(spt, w, h):
    import torch
    planes, _clean = dpt.synthetic_halves(w, h)
    dev = _upload(torch, planes)
    ptr = [t.data_ptr() for t in dev]
    n = w * h * 3
    dn = spt.Denoiser(w, h, 0)
    try:
        for pf in (0, spt.DENOISE_PAIR_OWN_WEIGHTS):
            for flags in (0, spt.DENOISE_NO_DEMODULATE):
                for it in (0, 1, 2, 3, 6):
                    p = spt.default_denoise_params(iterations=it, flags=flags)
                    bufs = [_guarded(torch, n) for _ in range(3)]
                    dn.denoise_pair_async(*ptr, p, pf, *[b.data_ptr() for b in bufs])
                    torch.cuda.synchronize()
                    got = [b.cpu().numpy() for b in bufs]
                    assert all(np.isnan(g[n]) for g in got), "a write past the plane"
                    want = spt.denoise_pair_host(*planes, p, pf)
                    label = f"{w}x{h} it={it} flags={flags} pair_flags={pf}"
                    for g, wnt, name in zip(got, want, ("out", "se_out", "diff")):
                        same(g[:n].reshape(h, w, 3), wnt, f"{name} {label}")
                    only = _guarded(torch, n)  # se_out and diff left out
                    dn.denoise_pair_async(*ptr, p, pf, only.data_ptr(), 0, 0)
                    torch.cuda.synchronize()
                    only = only.cpu().numpy()
                    assert np.isnan(only[n])
                    same(only[:n].reshape(h, w, 3), want[0], f"out alone {label}")
    finally:
        dn.close()


# ---- 2. the film path -----------------------------------------------------------------------------
def _pair_session(spt, prims, seed=5, adaptive=False):
    """-> (renderer, film A, film B, guide, params, cam): 64x48, 64 spp in batches of 8, even batches in
    A and odd ones in B (four each), a guide of GUIDE_SPP samples; adaptive films have had one selection
    after two batches each."""
    p = spt.default_params(width=W, height=H, spp=SPP, seed=seed)
    cam = spt.Camera(aspect=_aspect(W, H))
    r, fa, fb, guide = spt.Renderer(0), spt.Film(p, 0), spt.Film(p, 0), spt.Guide(p, 0)
    for f in (fa, fb):
        f.enable_noise(BATCH)
        if adaptive:
            f.enable_adaptive()
    for k in range(SPP // BATCH):
        f = fb if k & 1 else fa
        if adaptive:
            # an adaptive film takes only its next window, so each half takes windows 0..3 and the
            # halves are made independent by the seed instead of by the window
            pk = p if f is fa else spt.default_params(width=W, height=H, spp=SPP, seed=seed + 100)
            if k // 2 == 2:
                left = f.adaptive_select(0.03)
                assert 0 < left < W * H
            f.render(r, prims, cam, pk, (k // 2) * BATCH, BATCH)
        else:
            f.render(r, prims, cam, p, k * BATCH, BATCH)
        r.stats()
    guide.render(r, prims, cam, p, 0, GUIDE_SPP)
    return r, fa, fb, guide, p, cam


def _host_film_planes(spt, film, adaptive):
    fi, ni = film.info(), film.noise_info()
    sums, m2 = film.to_numpy(), film.noise_to_numpy()
    if adaptive:
        counts = film.counts_to_numpy()
        return (spt.film_adaptive_resolve_host(sums, counts, fi["width"], fi["rows"], fi["spp_total"], ni["batch"]),
                spt.film_adaptive_noise_map_host(sums, m2, counts, fi["width"], fi["rows"], fi["spp_total"],
                                                 ni["batch"]))
    return (spt.film_resolve_host(sums, fi["width"], fi["rows"], fi["spp_total"], fi["samples_done"]),
            spt.film_noise_map_host(sums, m2, fi["width"], fi["rows"], fi["spp_total"], fi["samples_done"],
                                    ni["batch"], ni["batches_done"]))


@pytest.mark.parametrize("scene,adaptive", [("head", False), ("spheres32", False), ("head", True)],
                         ids=["head", "spheres32", "head_adaptive"])
def test_film_pair_denoise_equals_the_separate_calls_and_the_host(spt, scene, adaptive):
    prims = spt.cornell_scene() if scene == "head" else spt.spheres32_scene()
    r, fa, fb, guide, p, cam = _pair_session(spt, prims, adaptive=adaptive)
    dn = spt.Denoiser(W, H, 0)
    merged = spt.Film(p, 0)
    try:
        state = [fa.to_numpy(), fa.noise_to_numpy(), fb.to_numpy(), fb.noise_to_numpy(), guide.to_numpy()]
        g = guide.resolve()
        planes = [fa.resolve(), fa.noise_map(), fb.resolve(), fb.noise_map(), g["albedo"], g["normal"], g["depth"]]
        gi = guide.info()
        hg = spt.guide_resolve_host(guide.to_numpy(), gi["width"], gi["rows"], gi["spp_total"], gi["samples_done"])
        host_planes = list(_host_film_planes(spt, fa, adaptive) + _host_film_planes(spt, fb, adaptive)) + \
            [hg["albedo"], hg["normal"], hg["depth"]]
        for a, b, name in zip(planes, host_planes, ("rgb_a", "se_a", "rgb_b", "se_b", "albedo", "normal", "depth")):
            same(a, b, f"resolved plane {name}")
        for own in (False, True):
            fused = dn.denoise_film_pair(fa, fb, guide, own_weights=own)
            apart = dn.denoise_pair(*planes, own_weights=own)
            want = spt.denoise_pair_host(*host_planes, None, own)
            for f_, a_, w_, name in zip(fused, apart, want, ("out", "se_out", "diff")):
                same(f_, a_, f"{name}: film_pair_denoise vs denoise_pair_async, own={own}")
                same(f_, w_, f"{name}: film_pair_denoise vs host, own={own}")
            assert (fused[2] != 0).any()
        # the denoise read the films and the guide, and only read them
        after = [fa.to_numpy(), fa.noise_to_numpy(), fb.to_numpy(), fb.noise_to_numpy(), guide.to_numpy()]
        assert all(np.array_equal(a, b) for a, b in zip(state, after))
        if not adaptive:  # A merged with B is the one-shot film
            merged.enable_noise(BATCH)
            merged.merge(fa)
            merged.merge(fb)
            same(merged.resolve(), spt.render(prims, cam, p), "A + B vs render()")
    finally:
        for o in (merged, dn, guide, fa, fb, r):
            o.close()


# ---- 3. the summary -------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (17, 13), (70, 50), (640, 103)], ids=lambda v: str(v))
def test_summary_device_equals_host_and_repeats(spt, w, h):
    rng = np.random.default_rng(w * 1000 + h)
    diff = (rng.normal(0.0, 0.05, (h, w, 3)) * rng.random((h, w, 1))).astype(np.float32)
    dn = spt.Denoiser(w, h, 0)
    try:
        one, two = dn.pair_summary(diff), dn.pair_summary(diff)
    finally:
        dn.close()
    host = spt.pair_summary_host(diff)
    assert one == two, "two device runs differ"
    for k in range(3):
        assert _close(one["rmse"][k], host["rmse"][k], REL_SUM), (k, one, host)
    assert _close(one["rmse_all"], host["rmse_all"], REL_SUM)
    assert one["diff_max"] == host["diff_max"] == float(np.abs(diff).max())


# ---- 4. isolation ---------------------------------------------------------------------------------
def test_a_context_and_the_single_filter_do_not_notice(spt):
    import torch
    prims = spt.cornell_scene()
    r, fa, fb, guide, p, cam = _pair_session(spt, prims)
    dn = spt.Denoiser(W, H, 0)
    keys = [k for k in spt.STAT_KEYS]

    def frames(with_pair):
        got = []
        for k, seed in enumerate((9, 10)):
            prm = spt.default_params(width=W, height=H, spp=4, seed=seed)
            buf = torch.zeros(W * H * 3, dtype=torch.float32, device="cuda")
            r.render_async(prims, cam, prm, buf.data_ptr())
            if with_pair and k == 0:
                got.append(dn.denoise_film_pair(fa, fb, guide))
            torch.cuda.synchronize()
            st = r.stats()
            got.append((buf.cpu().numpy(), [st[x] for x in keys], r.kernel()))
        return got

    try:
        single_before = dn.denoise_film(fa, guide, return_se=True)  # before the pair scratch exists
        a = frames(True)
        b = frames(False)
        again = dn.denoise_film_pair(fa, fb, guide)
        for x, y, name in zip(a[0], again, ("out", "se_out", "diff")):
            same(x, y, f"two runs: {name}")
        for (img_a, st_a, k_a), (img_b, st_b, k_b) in zip(a[1:], b):
            assert np.array_equal(img_a, img_b) and st_a == st_b and k_a == k_b
        single_after = dn.denoise_film(fa, guide, return_se=True)
        same(single_before[0], single_after[0], "the single filter around the first pair call")
        same(single_before[1], single_after[1], "the single filter's se_out around the first pair call")
    finally:
        for o in (dn, guide, fa, fb, r):
            o.close()


# ---- 5. rejected calls ----------------------------------------------------------------------------
def test_rejected_calls_leave_every_output_untouched(spt):
    import torch
    lib = spt.load_library()
    prims = spt.cornell_scene()
    r, fa, fb, guide, p, cam = _pair_session(spt, prims)
    planes, _clean = dpt.synthetic_halves(W, H)
    dev = _upload(torch, planes)
    ptr = [t.data_ptr() for t in dev]
    n = W * H * 3
    outs = [torch.full((n,), FILL, dtype=torch.float32, device="cuda") for _ in range(3)]
    o = [t.data_ptr() for t in outs]
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
    p128 = spt.default_params(width=W, height=H, spp=2 * SPP, seed=5)  # another spp_total
    other_spp = spt.Film(p128, 0)
    other_spp.enable_noise(BATCH)
    for k in range(2):
        other_spp.render(r, prims, cam, p128, k * BATCH, BATCH)
    pw = spt.default_params(width=W - 1, height=H, spp=SPP, seed=5)  # another width
    narrow = spt.Film(pw, 0)
    narrow.enable_noise(BATCH)
    camw = spt.Camera(aspect=_aspect(W - 1, H))
    for k in range(2):
        narrow.render(r, prims, camw, pw, k * BATCH, BATCH)
    state = [fa.to_numpy(), fa.noise_to_numpy(), fb.to_numpy(), fb.noise_to_numpy(), guide.to_numpy()]

    def refused(call, label):
        with pytest.raises(spt.SptError) as e:
            call()
        assert e.value.status == 1, label
        torch.cuda.synchronize()
        assert all(bool((t == FILL).all()) for t in outs), label

    try:
        for k in range(7):
            a = list(ptr)
            a[k] = 0
            refused(lambda: dn.denoise_pair_async(*a, ok(), 0, *o), f"null plane {k}")
            for slot in range(3):
                oo = list(o)
                oo[slot] = ptr[k]
                refused(lambda: dn.denoise_pair_async(*ptr, ok(), 0, *oo), f"output {slot} is input {k}")
        refused(lambda: dn.denoise_pair_async(*ptr, ok(), 0, 0, o[1], o[2]), "null out")
        for i, j in ((0, 1), (0, 2), (1, 2)):
            oo = list(o)
            oo[j] = oo[i]
            refused(lambda: dn.denoise_pair_async(*ptr, ok(), 0, *oo), f"outputs {i} and {j} are one plane")
            refused(lambda: dn.denoise_film_pair_async(fa, fb, guide, ok(), 0, *oo), f"film: outputs {i}, {j}")
        for pf in (2, 3, 0x80000000, 0x80000001):
            refused(lambda: dn.denoise_pair_async(*ptr, ok(), pf, *o), f"pair_flags {pf}")
            refused(lambda: dn.denoise_film_pair_async(fa, fb, guide, ok(), pf, *o), f"film pair_flags {pf}")
        for i, bp in enumerate(bad_params):
            refused(lambda: dn.denoise_pair_async(*ptr, bp, 0, *o), f"params {i}")
            refused(lambda: dn.denoise_film_pair_async(fa, fb, guide, bp, 0, *o), f"film params {i}")
        V = ctypes.c_void_p
        null = V(None)
        ins, oo = [V(x) for x in ptr], [V(x) for x in o]
        assert lib.spt_denoise_pair_async(dn._d, *ins, None, 0, *oo, null) == 1
        assert lib.spt_denoise_pair_async(null, *ins, ctypes.byref(ok()), 0, *oo, null) == 1
        film_cases = [(fa, fa, guide, dn, "one film twice")]
        for bad, label in [(plain, "a plain film"), (young, "one batch"), (shard_film, "a sharded film"),
                           (other_spp, "another spp_total"), (narrow, "another width")]:
            film_cases += [(bad, fb, guide, dn, label + " as A"), (fa, bad, guide, dn, label + " as B")]
        film_cases += [(fa, fb, empty_guide, dn, "an empty guide"), (fa, fb, shard_guide, dn, "a sharded guide"),
                       (fa, fb, guide, small, "the denoiser's size")]
        for a, b, g, d, label in film_cases:
            refused(lambda: d.denoise_film_pair_async(a, b, g, ok(), 0, *o), label)
        refused(lambda: dn.denoise_film_pair_async(fa, fb, guide, ok(), 0, 0, o[1], o[2]), "film: null out")
        byref = ctypes.byref(ok())
        assert lib.spt_film_pair_denoise(null, fb._f, guide._g, dn._d, byref, 0, *oo, null) == 1
        assert lib.spt_film_pair_denoise(fa._f, null, guide._g, dn._d, byref, 0, *oo, null) == 1
        assert lib.spt_film_pair_denoise(fa._f, fb._f, null, dn._d, byref, 0, *oo, null) == 1
        assert lib.spt_film_pair_denoise(fa._f, fb._f, guide._g, null, byref, 0, *oo, null) == 1
        s = spt.spt_pair_summary()
        assert lib.spt_denoise_pair_summary(null, oo[2], ctypes.byref(s), null) == 1
        assert lib.spt_denoise_pair_summary(dn._d, null, ctypes.byref(s), null) == 1
        assert lib.spt_denoise_pair_summary(dn._d, oo[2], None, null) == 1
        torch.cuda.synchronize()
        assert all(bool((t == FILL).all()) for t in outs)
        after = [fa.to_numpy(), fa.noise_to_numpy(), fb.to_numpy(), fb.noise_to_numpy(), guide.to_numpy()]
        assert all(np.array_equal(x, y) for x, y in zip(state, after)), "the films or the guide changed"
        # ... and the same arguments in range are accepted
        dn.denoise_film_pair_async(fa, fb, guide, ok(), spt.DENOISE_PAIR_OWN_WEIGHTS, *o)
        torch.cuda.synchronize()
        assert all(bool((t != FILL).any()) for t in outs) and bool((outs[0] != FILL).all())
    finally:
        for x in (dn, small, plain, young, empty_guide, shard_film, shard_guide, other_spp, narrow, guide, fa,
                  fb, r):
            x.close()


# ---- 6. quality -----------------------------------------------------------------------------------
QUALITY_SEEDS = (1, 2, 3, 4)
# rmse(pair result) / rmse(noisy merged film) against the 8192-spp truth, measured on an MI355X with the
# default parameters (profiles/r27_denoise_pair.json, "test_quality"); every value is bit-deterministic.
MEASURED_RATIO = {
    "cross": {1: 0.433233, 2: 0.462805, 3: 0.450989, 4: 0.434349},
    "own": {1: 0.467395, 2: 0.479380, 3: 0.472803, 4: 0.468541},
}
_truth = {}


def _truth_image(spt):
    if "img" not in _truth:
        p = spt.default_params(width=W, height=H, spp=8192, seed=77)
        _truth["img"] = spt.render(spt.cornell_scene(), spt.Camera(aspect=_aspect(W, H)), p)
    return _truth["img"]


@pytest.mark.parametrize("seed", QUALITY_SEEDS)
def test_pair_result_is_closer_to_the_truth(spt, seed):
    """HEAD at 64x48, 64 spp in batches of 8 (four per half), a guide of 16 samples; the truth is the
    library's own 8192-spp render with another seed. Hard conditions, both modes: the pair result's RMSE
    is strictly below the noisy merged film's and the image mean moves by at most 2 %. Pinned: the ratio
    per seed and mode is at most the value measured on the GPU x 1.25 (the margin is for later deliberate
    changes of the defaults). Measured, seeds 1..4 (noisy RMSE 0.1448, 0.1445, 0.1456, 0.1477): cross
    weights 0.433233, 0.462805, 0.450989, 0.434349, the mean moved by 0.19, 0.18, 0.69 and 0.49 %; own
    weights 0.467395, 0.479380, 0.472803, 0.468541, the mean moved by 1.28, 1.25, 0.93 and 1.03 %. (The
    single filter on the merged film: 0.471978, 0.478238, 0.474328, 0.475560, tests/test_gpu_denoise.py.)"""
    truth = _truth_image(spt)
    p = spt.default_params(width=W, height=H, spp=SPP, seed=seed)
    cam = spt.Camera(aspect=_aspect(W, H))
    for mode, own in (("cross", False), ("own", True)):
        den, info = spt.render_denoised_pair(spt.cornell_scene(), cam, p, batch=BATCH, guide_spp=GUIDE_SPP,
                                             own_weights=own, return_info=True)
        noisy = info["noisy"]
        e_noisy, e_den = rmse(noisy, truth), rmse(den, truth)
        mean_shift = abs(float(den.mean(dtype=np.float64)) / float(noisy.mean(dtype=np.float64)) - 1.0)
        print(f"seed {seed} {mode}: rmse noisy {e_noisy:.6f} pair {e_den:.6f} ratio {e_den / e_noisy:.6f} "
              f"mean shift {mean_shift:.6f} diff rmse {max(info['pair']['rmse']):.6f}")
        assert e_den < e_noisy
        assert mean_shift <= 0.02
        assert e_den / e_noisy <= MEASURED_RATIO[mode][seed] * 1.25


# ---- 7. the Python wrappers and the drop-in program -----------------------------------------------
def test_wrappers_and_the_dropin_program_equal_the_explicit_calls(spt, tmp_path):
    prims = spt.cornell_scene()
    r, fa, fb, guide, p, cam = _pair_session(spt, prims, seed=1)
    dn = spt.Denoiser(W, H, 0)
    merged = spt.Film(p, 0)
    try:
        want = {own: dn.denoise_film_pair(fa, fb, guide, own_weights=own, return_summary=True)
                for own in (False, True)}
        planes = guide.resolve()
        merged.enable_noise(BATCH)
        merged.merge(fa)
        merged.merge(fb)
        noisy = merged.resolve()
    finally:
        for o in (merged, dn, guide, fa, fb, r):
            o.close()
    p = spt.default_params(width=W, height=H, spp=SPP, seed=1)
    same(noisy, spt.render(prims, cam, p), "A + B vs render()")
    for own in (False, True):
        got, info = spt.render_denoised_pair(prims, cam, p, guide_spp=GUIDE_SPP, own_weights=own, return_info=True)
        same(got, want[own][0], f"render_denoised_pair own={own}")
        same(info["se"], want[own][1], "se")
        same(info["diff"], want[own][2], "diff")
        assert info["pair"] == want[own][3]
        same(info["noisy"], noisy, "noisy")
        for k in planes:
            same(info["guides"][k], planes[k], f"guide {k}")
    same(spt.render_denoised_pair(prims, cam, p, guide_spp=GUIDE_SPP), want[False][0], "without info")
    for bad in (dict(batch=16 * 2 + 1), dict(batch=SPP // 2), dict(batch=SPP // 3 + 1)):
        with pytest.raises(spt.SptError):
            spt.render_denoised_pair(prims, cam, p, **bad)
    # render_denoised_until: a huge target stops at min_batches, target 0 renders every batch
    out, info = spt.render_denoised_until(prims, cam, p, 1e9, guide_spp=GUIDE_SPP)
    assert info["batches_done"] == 4 and info["samples_done"] == 4 * BATCH and max(info["rmse"]) > 0
    out6, info6 = spt.render_denoised_until(prims, cam, p, 1e9, min_batches=5, guide_spp=GUIDE_SPP)
    assert info6["batches_done"] == 6
    out, info = spt.render_denoised_until(prims, cam, p, 0.0, guide_spp=GUIDE_SPP)
    assert info["batches_done"] == SPP // BATCH and info["samples_done"] == SPP
    same(out, want[True][0], "render_denoised_until(target 0) vs render_denoised_pair(own_weights=True)")
    assert info["rmse"] == want[True][3]["rmse"]
    # the program's guide takes min(SPP, 64) samples: SPP = 32 with batches of 4 gives 8 batches
    p32 = spt.default_params(width=W, height=H, spp=32, seed=1)
    exe = os.path.join(ROOT, "small-pathtracer_amd", "smallpt_amd")
    for flag, own in (([], False), (["--pair-own"], True)):
        want32 = spt.render_denoised_pair(prims, cam, p32, guide_spp=32, own_weights=own)
        out_path = tmp_path / f"d{int(own)}.pfm"
        run = subprocess.run([exe, str(W), str(H), "32", "1", str(out_path), "--pfm", "--denoise", "--pair"] + flag,
                             capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stdout + run.stderr
        raw = out_path.read_bytes()
        data = np.frombuffer(raw[len(raw) - W * H * 12:], dtype="<f4").reshape(H, W, 3)[::-1]
        same(data, want32, f"smallpt_amd --denoise --pair {flag} --pfm")
    bad = subprocess.run([exe, str(W), str(H), "32", "1", str(tmp_path / "x.pfm"), "--denoise", "--pair",
                          "--devices", "2"], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "--denoise" in bad.stderr
    alone = subprocess.run([exe, str(W), str(H), "32", "1", str(tmp_path / "x.pfm"), "--pair"],
                           capture_output=True, text=True, timeout=120)
    assert alone.returncode != 0 and "--pair" in alone.stderr
    usage = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert all(f in usage for f in ("--pair", "--pair-own"))

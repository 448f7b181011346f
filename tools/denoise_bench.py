"""Time and quality of the a-trous denoiser on the GPU (profiles/r19_denoise.json).

usage (on an MI355X, from the repo root):  python tools/denoise_bench.py [OUT.json]
(OUT.json defaults to build/r19_denoise.json)

Time: spt_denoise_async on synthetic planes at 1024x768 and 4096x4096, by device events, 20 timed
runs after 5 warm-up runs, for iterations = 0..6. T(k) - T(k-1) is iteration k's variance pass and
a-trous pass (step 2^(k-1)); T(1) also holds the pack kernel, and the last iteration of every call
is the variant with the finish fused in. Beside it the render kernel's time of one 64-spp frame at
1024x768 from the same session, and the bytes one iteration requests per pixel.
Single kernels (only with the bench library: `make -C small-pathtracer_amd/csrc denoise_bench`, then
SPT_LIB=build/libspt_denoise_bench.so): pack, the variance pass, and the a-trous pass at every step with
and without the fused finish, each as 50 launches between one pair of device events, 7 rounds, the
forms of one step alternating round by round (the plain-load form against the LDS-tiled form where the
build has one).
Quality: the HEAD scene at 256x192, 16 seeds at 64, 256 and 1024 spp in 8 batches with a guide of 64
samples, against the library's own 65536-spp render merged from 16 seeds of 4096.

--chain (python tools/denoise_bench.py --chain [OUT.json], default build/guide_chain_denoise.json):
instead of the above, the quality by region on the scenes with specular primitives (mirror_glass,
cornell_specular), same protocol, first-hit guides against guides of the specular chain
(SPT_GUIDE_THROUGH_SPECULAR): the RMSE of the clamped image over the whole frame, over the pixels whose
first hit is a SPEC or REFR primitive (at least half of the 64 samples of a first-hit guide of the
scene with the specular primitives white and the rest black), over the band within 2 pixels of that
set, and over the rest; the image-mean shift and se_out^2 / true err^2. And the configuration that
tests/test_gpu_guide_chain.py pins.

--pair (python tools/denoise_bench.py --pair [OUT.json], default build/r27_denoise_pair.json): the
two-half filter (SPT_HAS_DENOISE_PAIR). Time: at both shapes, 20 timed rounds after 5 warm-up rounds,
every round measuring by device events one spt_denoise_async, two of them, and one
spt_denoise_pair_async (cross and own weights), the order rotating round by round; with the bench
library also the pair call with plain loads against the pair call with the LDS-tiled form at steps 1
and 2, and the single pair kernels (pack, variance, a-trous at every step, both forms where the tiled
one exists) in kernel_times' shape. Quality and calibration: HEAD and mirror_glass (by region, first-hit
guides) at 256x192, 16 seeds, 8 batches (four per half), a guide of 64 samples, truth 16 x 4096 spp, at
64 / 256 / 1024 spp: the RMSE of the single filter, of pair-cross and of pair-own over the film's, the
image-mean shift, and for both modes mean diff^2 and mean se_out^2 over the variance of `out` across
the seeds and over the mean squared error against the truth. And the configuration that
tests/test_gpu_denoise_pair.py pins.

--bank (python tools/denoise_bench.py --bank [OUT.json], default build/r28_denoise_bank.json): the filter
bank (SPT_HAS_DENOISE_BANK). Cost: at both shapes, 20 timed rounds after 5 warm-up rounds, every round
measuring by device events K spt_denoise_pair_async calls and one spt_denoise_bank_async of K candidates,
for K = 2 and 3 (sigma_color 2, 8 and 2, 4, 8), own weights, the order rotating; the bank's overhead over
the K pair calls per round; with the bench library the single bank kernels (error, smoothing at steps 1
and 2, blend, the halves-storing pair pass) beside a plain pair a-trous pass of the same session. Quality
and calibration: --pair's protocol (HEAD, and mirror_glass by region; 256x192, 16 seeds, 8 batches, a
guide of 64 samples, truth 16 x 4096 spp, at 64 / 256 / 1024 spp): the RMSE over the film's of the bank of
sigma_color {2, 4, 8} with own and with cross weights (and of that bank with three smoothing passes, of a
bank of {4, 8} and of one candidate alone, where no selection takes place), of each candidate alone (pair,
own and cross), the share of the pixels per candidate by region, and mean mse and mean own-weight diff^2
over the mean squared error against the truth.

--light-guide (python tools/denoise_bench.py --light-guide [OUT.json], default
build/guide_light_denoise.json): what shading the albedo plane by a light guide's visibility
(SPT_HAS_GUIDE_LIGHT, render_denoised(light_guide=True)) buys, by region, with --pair's protocol (HEAD and
mirror_glass, first-hit guides; 256x192, 16 seeds, 8 batches, guide and light guide of 64 samples, truth
16 x 4096 spp, at 64 / 256 / 1024 spp): the RMSE of the denoised image over the film's for the single
filter and the cross-weighted pair, without the light guide and with it at shade_floor 0.1, 0.25 and
0.5; over the whole frame, over the shadow band (the pixels with 0.05 < visibility < 0.95 in a light guide
of 1024 samples, seed 1000, and the pixels within 2 of them) and over the fully lit and fully shadowed
rest; the seeds in which the shaded run beats the plain one; and the image-mean shift. mirror_glass has
no light rectangle: its light guide samples a 24 x 24 square of the light sphere's cap (prim 8).
"""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# per pixel and iteration: 25 taps x three 16-byte loads, the centre's gradient, the 3x3 variance
# reads (nine 4-byte components of 16-byte elements) and its 4-byte write, 16 bytes out
BYTES_PER_PIXEL_ITERATION = 25 * 48 + 8 + 9 * 4 + 4 + 16


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def time_denoise(spt, torch, w, h, runs=20, warmup=5):
    import denoise_truth as dt
    tile = dt.synthetic(256, 192)
    reps = (-(-h // 192), -(-w // 256))
    planes = [np.tile(tile[k], reps + ((1,) if tile[k].ndim == 3 else ()))[:h, :w] for k in dt.PLANES]
    dev = [torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda() for a in planes]
    out = torch.empty(w * h * 3, dtype=torch.float32, device="cuda")
    se_out = torch.empty(w * h * 3, dtype=torch.float32, device="cuda")
    dn = spt.Denoiser(w, h, 0)
    res = {}
    try:
        for it in range(7):
            p = spt.default_denoise_params(iterations=it)
            ms = []
            for k in range(warmup + runs):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                dn.denoise_async(*[t.data_ptr() for t in dev], p, out.data_ptr(), se_out.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
                b.record()
                torch.cuda.synchronize()
                if k >= warmup:
                    ms.append(a.elapsed_time(b))
            res[str(it)] = {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)),
                            "max_ms": float(np.max(ms))}
    finally:
        dn.close()
    med = [res[str(k)]["median_ms"] for k in range(7)]
    per_iter = [med[k] - med[k - 1] for k in range(2, 7)]
    res["iteration_ms_steps_2_to_32"] = per_iter
    res["bytes_per_pixel_iteration"] = BYTES_PER_PIXEL_ITERATION
    res["requested_TB_per_s_steps_2_to_32"] = [BYTES_PER_PIXEL_ITERATION * w * h / (t * 1e-3) / 1e12
                                               for t in per_iter]
    return res


def kernel_times(spt, torch, w, h, launches=50, rounds=7):
    """Per-launch milliseconds of every denoise kernel alone (the bench library's entry point)."""
    import ctypes
    import denoise_truth as dt
    lib = spt.load_library()
    if not hasattr(lib, "spt_denoise_bench_kernel"):
        return {"skipped": "the loaded library has no bench entry points (make denoise_bench)"}
    V, I32 = ctypes.c_void_p, ctypes.c_int32
    lib.spt_denoise_bench_kernel.argtypes = [V, I32, I32, I32, V, V, V, V, V,
                                             ctypes.POINTER(spt.spt_denoise_params), V, V, V]
    lib.spt_denoise_bench_kernel.restype = I32
    tile = dt.synthetic(256, 192)
    reps = (-(-h // 192), -(-w // 256))
    planes = [np.tile(tile[k], reps + ((1,) if tile[k].ndim == 3 else ()))[:h, :w] for k in dt.PLANES]
    dev = [torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda() for a in planes]
    out = torch.empty(w * h * 3, dtype=torch.float32, device="cuda")
    se_out = torch.empty(w * h * 3, dtype=torch.float32, device="cuda")
    p = spt.default_denoise_params()
    dn = spt.Denoiser(w, h, 0)
    stream = torch.cuda.current_stream().cuda_stream

    def launch(which, step, form):
        return lib.spt_denoise_bench_kernel(dn._d, which, step, form, *[V(t.data_ptr()) for t in dev],
                                            ctypes.byref(p), V(out.data_ptr()), V(se_out.data_ptr()), V(stream))

    def once(which, step, form):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            launch(which, step, form)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / launches

    def stat(ms):
        return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}

    res = {"launches_per_round": launches, "rounds": rounds}
    try:
        assert launch(0, 1, 1) == 0 and launch(1, 1, 1) == 0  # the scratch holds a packed image from here on
        has_tiled = launch(2, 1, 2) == 0
        torch.cuda.synchronize()
        res["tiled_form_in_this_build"] = bool(has_tiled)
        for name, which in (("pack", 0), ("variance", 1)):
            once(which, 1, 1)
            res[name] = stat([once(which, 1, 1) for _ in range(rounds)])
        for step in (1, 2, 4, 8, 16, 32):
            forms = [("plain", 1)] + ([("tiled", 2)] if has_tiled and step <= 2 else [])
            for name, which in (("atrous", 2), ("atrous_finish", 3)):
                ms = {f: [] for f, _ in forms}
                for f, form in forms:
                    once(which, step, form)
                for _ in range(rounds):
                    for f, form in forms:
                        ms[f].append(once(which, step, form))
                for f, _ in forms:
                    res[f"{name}_step{step}_{f}"] = stat(ms[f])
    finally:
        dn.close()
    return res


def test_quality(spt):
    """The configuration tests/test_gpu_denoise.py pins: HEAD 64x48, 64 spp in batches of 8, a guide of
    16 samples, seeds 1..4, the truth 8192 spp with seed 77; the default parameters."""
    w, h = 64, 48
    prims = spt.cornell_scene()
    cam = spt.Camera(aspect=float(np.float32(w) / np.float32(h)))
    truth = spt.render(prims, cam, spt.default_params(width=w, height=h, spp=8192, seed=77))
    seeds = {}
    for seed in (1, 2, 3, 4):
        p = spt.default_params(width=w, height=h, spp=64, seed=seed)
        r, film, guide, dn = spt.Renderer(0), spt.Film(p, 0), spt.Guide(p, 0), spt.Denoiser(w, h, 0)
        try:
            film.enable_noise(8)
            for k in range(8):
                film.render(r, prims, cam, p, k * 8, 8)
                r.stats()
            guide.render(r, prims, cam, p, 0, 16)
            noisy, den = film.resolve(), dn.denoise_film(film, guide)
        finally:
            for o in (dn, guide, film, r):
                o.close()
        seeds[str(seed)] = {"rmse_noisy": rmse(noisy, truth), "rmse_denoised": rmse(den, truth),
                            "ratio": rmse(den, truth) / rmse(noisy, truth),
                            "mean_shift": abs(float(den.mean(dtype=np.float64) / noisy.mean(dtype=np.float64)) - 1.0)}
    return {"what": "tests/test_gpu_denoise.py::test_denoised_is_closer_to_the_truth", "seeds": seeds}


def quality(spt, w=256, h=192, seeds=16, spps=(64, 256, 1024)):
    prims = spt.cornell_scene()
    cam = spt.Camera(aspect=float(np.float32(w) / np.float32(h)))
    truth = np.zeros((h, w, 3), np.float64)
    for s in range(16):
        truth += spt.render(prims, cam, spt.default_params(width=w, height=h, spp=4096, seed=1000 + s))
    truth = (truth / 16).astype(np.float32)
    variants = {"default": {}, "no_demodulate": {"flags": spt.DENOISE_NO_DEMODULATE},
                "sigma_color_2": {"sigma_color": 2.0}, "sigma_color_8": {"sigma_color": 8.0}}
    acc = {v: {spp: [] for spp in spps} for v in variants}
    noisy_rmse = {spp: [] for spp in spps}
    for spp in spps:
        for seed in range(1, seeds + 1):
            p = spt.default_params(width=w, height=h, spp=spp, seed=seed)
            r, film, guide, dn = spt.Renderer(0), spt.Film(p, 0), spt.Guide(p, 0), spt.Denoiser(w, h, 0)
            try:
                film.enable_noise(spp // 8)
                for k in range(8):
                    film.render(r, prims, cam, p, k * (spp // 8), spp // 8)
                    r.stats()
                guide.render(r, prims, cam, p, 0, 64)
                noisy = film.resolve()
                noisy_rmse[spp].append(rmse(noisy, truth))
                for v, kw in variants.items():
                    den, se = dn.denoise_film(film, guide, spt.default_denoise_params(**kw), return_se=True)
                    acc[v][spp].append({
                        "rmse": rmse(den, truth),
                        "mean_change": float(den.mean(dtype=np.float64) / noisy.mean(dtype=np.float64) - 1.0),
                        "se2_over_err2": float(np.mean(se.astype(np.float64) ** 2) /
                                               np.mean((den.astype(np.float64) - truth) ** 2))})
            finally:
                for o in (dn, guide, film, r):
                    o.close()
    res = {"scene": "HEAD", "width": w, "height": h, "seeds": seeds, "truth": "16 seeds x 4096 spp",
           "noisy_rmse": {str(s): float(np.mean(noisy_rmse[s])) for s in spps}, "variants": {}}
    inv = np.array([1.0 / np.sqrt(s) for s in spps])
    base = np.array([np.mean(noisy_rmse[s]) for s in spps])
    for v in variants:
        res["variants"][v] = {}
        for spp in spps:
            rows = acc[v][spp]
            d = float(np.mean([x["rmse"] for x in rows]))
            n = float(np.mean(noisy_rmse[spp]))
            # the sample count at which the plain film reaches d: the noisy RMSE is linear in 1/sqrt(spp)
            # (a least-squares line through the three measured counts), solved for the count
            slope, icpt = np.polyfit(inv, base, 1)
            x = (d - icpt) / slope
            equal_spp = float(1.0 / (x * x)) if x > 0 else float("inf")
            res["variants"][v][str(spp)] = {
                "rmse_noisy": n, "rmse_denoised": d, "ratio": d / n,
                "ratio_min_max": [float(min(x["rmse"] / m for x, m in zip(rows, noisy_rmse[spp]))),
                                  float(max(x["rmse"] / m for x, m in zip(rows, noisy_rmse[spp])))],
                "mean_change": float(np.mean([x["mean_change"] for x in rows])),
                "plain_spp_for_equal_rmse": equal_spp, "times_fewer_samples": equal_spp / spp,
                "mean_se_out2_over_true_err2": float(np.mean([x["se2_over_err2"] for x in rows]))}
    return res


def specular_masks(spt, prims, cam, w, h, seed=1000, **kw):
    """-> {"specular", "band", "rest"}: boolean (h, w) masks from a first-hit guide of the scene with
    its specular primitives white and the others black (the same geometry, so the same hits)."""
    marker = [spt.spt_prim.from_buffer_copy(q) for q in prims]
    for q in marker:
        for k in range(3):
            q.c[k] = 0.0 if q.refl == spt.DIFF else 1.0
    p = spt.default_params(width=w, height=h, spp=64, seed=seed, **kw)
    spec = spt.render_guides(marker, cam, p)["albedo"][..., 0] >= 0.5
    near = np.zeros_like(spec)
    pad = np.pad(spec, 2)
    for dy in range(5):
        for dx in range(5):
            near |= pad[dy:dy + h, dx:dx + w]
    band = near & ~spec
    return {"specular": spec, "band": band, "rest": ~near}


def _film_and_guides(spt, prims, cam, p, batch, guide_spp):
    """-> (noisy, {chain: (denoised, se_out)}) of one film denoised with either kind of guide."""
    r, film, dn = spt.Renderer(0), spt.Film(p, 0), spt.Denoiser(p.width, p.height, 0)
    guides = {c: spt.Guide(p, 0, through_specular=c) for c in (False, True)}
    try:
        film.enable_noise(batch)
        for k in range(p.spp // batch):
            film.render(r, prims, cam, p, k * batch, batch)
            r.stats()
        out = {}
        for c, g in guides.items():
            g.render(r, prims, cam, p, 0, min(p.spp, guide_spp))
            out[c] = dn.denoise_film(film, g, return_se=True)
        return film.resolve(), out
    finally:
        for o in (dn, film, r, *guides.values()):
            o.close()


CHAIN_SCENES = {"mirror_glass": ("smallpt_mirror_glass_scene", dict(nee_prob=0.0)),
                "cornell_specular": ("cornell_specular_scene", {})}


def chain_quality(spt, name, w=256, h=192, seeds=16, spps=(64, 256, 1024)):
    prims = getattr(spt, CHAIN_SCENES[name][0])()
    kw = CHAIN_SCENES[name][1]
    cam = spt.Camera(aspect=float(np.float32(w) / np.float32(h)))
    truth = np.zeros((h, w, 3), np.float64)
    for s in range(16):
        truth += spt.render(prims, cam, spt.default_params(width=w, height=h, spp=4096, seed=1000 + s, **kw))
    truth = (truth / 16).astype(np.float32)
    masks = specular_masks(spt, prims, cam, w, h, **kw)
    masks["frame"] = np.ones((h, w), bool)
    res = {"scene": name, "width": w, "height": h, "seeds": seeds, "truth": "16 seeds x 4096 spp",
           "guide_spp": 64, "pixels": {k: int(m.sum()) for k, m in masks.items()}, "by_spp": {}}
    for spp in spps:
        rows = {k: {"noisy": [], "first_hit": [], "chain": []} for k in masks}
        extra = {g: {"mean_change": [], "se2_over_err2": []} for g in ("first_hit", "chain")}
        for seed in range(1, seeds + 1):
            p = spt.default_params(width=w, height=h, spp=spp, seed=seed, **kw)
            noisy, out = _film_and_guides(spt, prims, cam, p, spp // 8, 64)
            for k, m in masks.items():
                rows[k]["noisy"].append(rmse(noisy[m], truth[m]))
                rows[k]["first_hit"].append(rmse(out[False][0][m], truth[m]))
                rows[k]["chain"].append(rmse(out[True][0][m], truth[m]))
            for g, c in (("first_hit", False), ("chain", True)):
                den, se = out[c]
                extra[g]["mean_change"].append(float(den.mean(dtype=np.float64) / noisy.mean(dtype=np.float64) - 1.0))
                extra[g]["se2_over_err2"].append(float(np.mean(se.astype(np.float64) ** 2) /
                                                       np.mean((den.astype(np.float64) - truth) ** 2)))
        one = {"regions": {}}
        for k in masks:
            n, f, c = (float(np.mean(rows[k][x])) for x in ("noisy", "first_hit", "chain"))
            one["regions"][k] = {"rmse_noisy": n, "rmse_first_hit": f, "rmse_chain": c,
                                 "ratio_first_hit": f / n, "ratio_chain": c / n, "chain_over_first_hit": c / f,
                                 "seeds_where_chain_is_better": int(sum(a < b for a, b in zip(rows[k]["chain"],
                                                                                              rows[k]["first_hit"])))}
        for g in extra:
            one[g] = {"mean_change": float(np.mean(extra[g]["mean_change"])),
                      "mean_se_out2_over_true_err2": float(np.mean(extra[g]["se2_over_err2"]))}
        res["by_spp"][str(spp)] = one
    return res


def chain_test_quality(spt):
    """The configuration tests/test_gpu_guide_chain.py pins: mirror_glass 64x48, 64 spp in batches of
    8, guides of 16 samples, seeds 1..4, the truth 8192 spp with seed 77; the default parameters."""
    w, h = 64, 48
    prims = spt.smallpt_mirror_glass_scene()
    cam = spt.Camera(aspect=float(np.float32(w) / np.float32(h)))
    truth = spt.render(prims, cam, spt.default_params(width=w, height=h, spp=8192, seed=77, nee_prob=0.0))
    m = specular_masks(spt, prims, cam, w, h, seed=77, nee_prob=0.0)["specular"]
    seeds = {}
    for seed in (1, 2, 3, 4):
        p = spt.default_params(width=w, height=h, spp=64, seed=seed, nee_prob=0.0)
        noisy, out = _film_and_guides(spt, prims, cam, p, 8, 16)
        row = {"rmse_noisy": rmse(noisy, truth), "mask_rmse_noisy": rmse(noisy[m], truth[m])}
        for g, c in (("first_hit", False), ("chain", True)):
            den = out[c][0]
            row[g] = {"rmse": rmse(den, truth), "mask_rmse": rmse(den[m], truth[m]),
                      "mask_ratio": rmse(den[m], truth[m]) / rmse(noisy[m], truth[m]),
                      "mean_shift": abs(float(den.mean(dtype=np.float64) / noisy.mean(dtype=np.float64)) - 1.0)}
        seeds[str(seed)] = row
    return {"what": "tests/test_gpu_guide_chain.py::test_denoised_with_chain_guides_is_closer_to_the_truth",
            "mask_pixels": int(m.sum()), "seeds": seeds}


def main_chain(out):
    import torch
    spt = importlib.import_module("small-pathtracer_amd")
    spt.load_library()
    assert torch.cuda.is_available(), "denoise_bench needs the GPU"
    rec = {"kernel_sources_sha16": spt.build_sources_sha16(), "device": torch.cuda.get_device_name(0),
           "utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime())}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    rec["test_quality"] = chain_test_quality(spt)
    json.dump(rec, open(out, "w"), indent=1)
    rec["quality"] = {}
    for name in CHAIN_SCENES:
        rec["quality"][name] = chain_quality(spt, name)
        json.dump(rec, open(out, "w"), indent=1)  # what is measured survives a failure further on
        print(name, json.dumps({s: v["regions"] for s, v in rec["quality"][name]["by_spp"].items()}), flush=True)


# ---- the two-half filter (--pair) -------------------------------------------------------------------
def _pair_planes(w, h):
    import denoise_pair_truth as dpt
    tile, _clean = dpt.synthetic_halves(256, 192)
    reps = (-(-h // 192), -(-w // 256))
    return [np.ascontiguousarray(np.tile(a, reps + ((1,) if a.ndim == 3 else ()))[:h, :w]) for a in tile]


def _stat(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


def time_pair(spt, torch, w, h, runs=20, warmup=5):
    """One single call, two single calls and one pair call per round, the order rotating."""
    import ctypes
    lib = spt.load_library()
    planes = _pair_planes(w, h)
    dev = [torch.from_numpy(a.reshape(-1)).cuda() for a in planes]
    ra, sa, rb, sb, al, no, de = [t.data_ptr() for t in dev]
    outs = [torch.empty(w * h * 3, dtype=torch.float32, device="cuda") for _ in range(3)]
    o = [t.data_ptr() for t in outs]
    dn = spt.Denoiser(w, h, 0)
    p = spt.default_denoise_params()
    stream = torch.cuda.current_stream().cuda_stream
    has_form = hasattr(lib, "spt_denoise_pair_bench_form")
    if has_form:
        lib.spt_denoise_pair_bench_form.argtypes = [ctypes.c_int32]
        lib.spt_denoise_pair_bench_form.restype = ctypes.c_int32

    def single(n):
        def run():
            dn.denoise_async(ra, sa, al, no, de, p, o[0], o[1], stream)
            if n == 2:
                dn.denoise_async(rb, sb, al, no, de, p, o[2], o[1], stream)
        return run

    def pair(flags, form=None):
        def run():
            if form is not None:
                assert lib.spt_denoise_pair_bench_form(form) == 0
            dn.denoise_pair_async(ra, sa, rb, sb, al, no, de, p, flags, o[0], o[1], o[2], stream)
            if form is not None:
                lib.spt_denoise_pair_bench_form(0)
        return run

    what = [("single", single(1)), ("two_singles", single(2)), ("pair_cross", pair(0)),
            ("pair_own", pair(spt.DENOISE_PAIR_OWN_WEIGHTS))]
    if has_form:
        what += [("pair_cross_plain_loads", pair(0, 1)), ("pair_cross_tiled_steps_1_2", pair(0, 2))]
    ms = {k: [] for k, _ in what}
    try:
        for r in range(warmup + runs):
            for j in range(len(what)):
                name, run = what[(j + r) % len(what)]
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                run()
                b.record()
                torch.cuda.synchronize()
                if r >= warmup:
                    ms[name].append(a.elapsed_time(b))
    finally:
        dn.close()
    res = {k: _stat(v) for k, v in ms.items()}
    res["pair_over_single"] = res["pair_cross"]["median_ms"] / res["single"]["median_ms"]
    res["pair_over_two_singles"] = res["pair_cross"]["median_ms"] / res["two_singles"]["median_ms"]
    # per round: the pair call against the two single calls of the same round
    per = np.array(ms["pair_cross"]) / np.array(ms["two_singles"])
    res["pair_over_two_singles_per_round_min_max"] = [float(per.min()), float(per.max())]
    if has_form:
        per = np.array(ms["pair_cross_tiled_steps_1_2"]) / np.array(ms["pair_cross_plain_loads"])
        res["tiled_over_plain"] = {"median": float(np.median(per)), "min": float(per.min()), "max": float(per.max())}
    return res


def pair_kernel_times(spt, torch, w, h, launches=50, rounds=7):
    """Per-launch milliseconds of every pair kernel alone (the bench library's entry point)."""
    import ctypes
    lib = spt.load_library()
    if not hasattr(lib, "spt_denoise_pair_bench_kernel"):
        return {"skipped": "the loaded library has no bench entry points (make denoise_bench)"}
    V, I32 = ctypes.c_void_p, ctypes.c_int32
    lib.spt_denoise_pair_bench_kernel.argtypes = [V, I32, I32, I32] + [V] * 7 + [
        ctypes.POINTER(spt.spt_denoise_params), ctypes.c_uint32, V, V, V, V]
    lib.spt_denoise_pair_bench_kernel.restype = I32
    dev = [torch.from_numpy(a.reshape(-1)).cuda() for a in _pair_planes(w, h)]
    outs = [torch.empty(w * h * 3, dtype=torch.float32, device="cuda") for _ in range(3)]
    p = spt.default_denoise_params()
    dn = spt.Denoiser(w, h, 0)
    stream = torch.cuda.current_stream().cuda_stream

    def launch(which, step, form):
        return lib.spt_denoise_pair_bench_kernel(dn._d, which, step, form, *[V(t.data_ptr()) for t in dev],
                                                 ctypes.byref(p), 0, *[V(t.data_ptr()) for t in outs], V(stream))

    def once(which, step, form):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            launch(which, step, form)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / launches

    res = {"launches_per_round": launches, "rounds": rounds}
    try:
        assert launch(0, 1, 1) == 0 and launch(1, 1, 1) == 0  # the scratch holds a packed pair from here on
        has_tiled = launch(2, 1, 2) == 0
        torch.cuda.synchronize()
        res["tiled_form_in_this_build"] = bool(has_tiled)
        for name, which in (("pair_pack", 0), ("pair_variance", 1)):
            once(which, 1, 1)
            res[name] = _stat([once(which, 1, 1) for _ in range(rounds)])
        for step in (1, 2, 4, 8, 16, 32):
            forms = [("plain", 1)] + ([("tiled", 2)] if has_tiled and step <= 2 else [])
            for name, which in (("pair_atrous", 2), ("pair_atrous_finish", 3)):
                ms = {f: [] for f, _ in forms}
                for f, form in forms:
                    once(which, step, form)
                for _ in range(rounds):
                    for f, form in forms:
                        ms[f].append(once(which, step, form))
                for f, _ in forms:
                    res[f"{name}_step{step}_{f}"] = _stat(ms[f])
    finally:
        dn.close()
    return res


def pair_test_quality(spt):
    """The configuration tests/test_gpu_denoise_pair.py pins: HEAD 64x48, 64 spp in batches of 8 (even
    batches in A, odd in B), a guide of 16 samples, seeds 1..4, the truth 8192 spp with seed 77."""
    w, h = 64, 48
    prims = spt.cornell_scene()
    cam = spt.Camera(aspect=float(np.float32(w) / np.float32(h)))
    truth = spt.render(prims, cam, spt.default_params(width=w, height=h, spp=8192, seed=77))
    res = {"cross": {}, "own": {}}
    for seed in (1, 2, 3, 4):
        p = spt.default_params(width=w, height=h, spp=64, seed=seed)
        for mode, own in (("cross", False), ("own", True)):
            den, info = spt.render_denoised_pair(prims, cam, p, batch=8, guide_spp=16, own_weights=own,
                                                 return_info=True)
            noisy = info["noisy"]
            res[mode][str(seed)] = {
                "rmse_noisy": rmse(noisy, truth), "rmse_pair": rmse(den, truth),
                "ratio": rmse(den, truth) / rmse(noisy, truth),
                "mean_shift": abs(float(den.mean(dtype=np.float64) / noisy.mean(dtype=np.float64)) - 1.0),
                "diff_rmse": info["pair"]["rmse"]}
    return {"what": "tests/test_gpu_denoise_pair.py::test_pair_result_is_closer_to_the_truth", "modes": res}


PAIR_SCENES = {"HEAD": ("cornell_scene", {}), "mirror_glass": ("smallpt_mirror_glass_scene", dict(nee_prob=0.0))}


def pair_quality(spt, name, w=256, h=192, seeds=16, spps=(64, 256, 1024)):
    prims = getattr(spt, PAIR_SCENES[name][0])()
    kw = PAIR_SCENES[name][1]
    cam = spt.Camera(aspect=float(np.float32(w) / np.float32(h)))
    truth = np.zeros((h, w, 3), np.float64)
    for s in range(16):
        truth += spt.render(prims, cam, spt.default_params(width=w, height=h, spp=4096, seed=1000 + s, **kw))
    truth = (truth / 16).astype(np.float32)
    masks = {"frame": np.ones((h, w), bool)}
    if name != "HEAD":
        masks.update(specular_masks(spt, prims, cam, w, h, **kw))
    res = {"scene": name, "width": w, "height": h, "seeds": seeds, "truth": "16 seeds x 4096 spp", "guide_spp": 64,
           "batches": 8, "pixels": {k: int(m.sum()) for k, m in masks.items()}, "by_spp": {}}
    modes = ("single", "cross", "own")
    for spp in spps:
        batch = spp // 8
        outs = {m: [] for m in modes}
        est = {m: {"diff2": [], "se2": []} for m in modes}
        noisy_all = []
        for seed in range(1, seeds + 1):
            p = spt.default_params(width=w, height=h, spp=spp, seed=seed, **kw)
            r, fa, fb, film, guide, dn = (spt.Renderer(0), spt.Film(p, 0), spt.Film(p, 0), spt.Film(p, 0),
                                          spt.Guide(p, 0), spt.Denoiser(w, h, 0))
            try:
                for f in (fa, fb, film):
                    f.enable_noise(batch)
                for k in range(8):
                    (fb if k & 1 else fa).render(r, prims, cam, p, k * batch, batch)
                    r.stats()
                film.merge(fa)
                film.merge(fb)
                guide.render(r, prims, cam, p, 0, min(spp, 64))
                noisy_all.append(film.resolve())
                den, se = dn.denoise_film(film, guide, return_se=True)
                outs["single"].append(den)
                est["single"]["se2"].append(se.astype(np.float64) ** 2)
                for m, own in (("cross", False), ("own", True)):
                    out, se, diff = dn.denoise_film_pair(fa, fb, guide, own_weights=own)
                    outs[m].append(out)
                    est[m]["se2"].append(se.astype(np.float64) ** 2)
                    est[m]["diff2"].append(diff.astype(np.float64) ** 2)
            finally:
                for o in (dn, guide, film, fa, fb, r):
                    o.close()
        one = {"regions": {}, "calibration": {}}
        for k, mk in masks.items():
            n = float(np.mean([rmse(x[mk], truth[mk]) for x in noisy_all]))
            row = {"rmse_noisy": n}
            for m in modes:
                d = float(np.mean([rmse(x[mk], truth[mk]) for x in outs[m]]))
                row[f"rmse_{m}"] = d
                row[f"ratio_{m}"] = d / n
            row["cross_over_single"] = row["rmse_cross"] / row["rmse_single"]
            row["own_over_single"] = row["rmse_own"] / row["rmse_single"]
            row["seeds_where_cross_beats_single"] = int(sum(
                rmse(a[mk], truth[mk]) < rmse(b[mk], truth[mk]) for a, b in zip(outs["cross"], outs["single"])))
            one["regions"][k] = row
        for m in modes:
            stack = np.stack([x.astype(np.float64) for x in outs[m]])
            var = float(stack.var(axis=0, ddof=1).mean())
            mse = float(np.mean((stack - truth.astype(np.float64)) ** 2))
            noisy_mean = float(np.mean([x.mean(dtype=np.float64) for x in noisy_all]))
            cal = {"variance_of_out_across_seeds": var, "mse_against_truth": mse,
                   "mean_change": float(stack.mean() / noisy_mean - 1.0),
                   "se_out2_over_variance": float(np.mean(est[m]["se2"]) / var),
                   "se_out2_over_mse": float(np.mean(est[m]["se2"]) / mse)}
            if est[m]["diff2"]:
                cal["diff2_over_variance"] = float(np.mean(est[m]["diff2"]) / var)
                cal["diff2_over_mse"] = float(np.mean(est[m]["diff2"]) / mse)
            one["calibration"][m] = cal
        res["by_spp"][str(spp)] = one
    return res


def main_pair(out):
    import torch
    spt = importlib.import_module("small-pathtracer_amd")
    spt.load_library()
    assert torch.cuda.is_available(), "denoise_bench needs the GPU"
    rec = {"kernel_sources_sha16": spt.build_sources_sha16(), "device": torch.cuda.get_device_name(0),
           "utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()), "time": {}, "kernels": {}}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    for w, h in ((1024, 768), (4096, 4096)):
        rec["time"][f"{w}x{h}"] = time_pair(spt, torch, w, h)
        rec["kernels"][f"{w}x{h}"] = pair_kernel_times(spt, torch, w, h)
        json.dump(rec, open(out, "w"), indent=1)
        print(f"{w}x{h}", json.dumps(rec["time"][f"{w}x{h}"]), flush=True)
    rec["test_quality"] = pair_test_quality(spt)
    json.dump(rec, open(out, "w"), indent=1)
    rec["quality"] = {}
    for name in PAIR_SCENES:
        rec["quality"][name] = pair_quality(spt, name)
        json.dump(rec, open(out, "w"), indent=1)  # what is measured survives a failure further on
        print(name, json.dumps({s: (v["regions"]["frame"], v["calibration"])
                                for s, v in rec["quality"][name]["by_spp"].items()}), flush=True)


# ---- the filter bank (--bank) -----------------------------------------------------------------------
BANK_SIGMAS = (2.0, 4.0, 8.0)
# the banks of the quality protocol: name -> (sigma_colors, own weights, error_iterations or None = default).
# Beside the bank of the issue with own and cross weights: the widest smoothing, a bank without the narrow
# candidate, and one candidate alone (no selection: what the estimate reads before an argmin is taken).
BANK_VARIANTS = {"bank_own": (BANK_SIGMAS, True, None), "bank_cross": (BANK_SIGMAS, False, None),
                 "bank_own_3_passes": (BANK_SIGMAS, True, 3), "bank_own_4_8": ((4.0, 8.0), True, None),
                 "one_own_4": ((4.0,), True, None), "one_own_8": ((8.0,), True, None)}


def time_bank(spt, torch, w, h, runs=20, warmup=5):
    """K pair calls and one bank call of K candidates per round, K = 2 and 3, the order rotating."""
    planes = _pair_planes(w, h)
    dev = [torch.from_numpy(a.reshape(-1)).cuda() for a in planes]
    ptr = [t.data_ptr() for t in dev]
    outs = [torch.empty(w * h * 3, dtype=torch.float32, device="cuda") for _ in range(3)]
    o = [t.data_ptr() for t in outs]
    mse = torch.empty(w * h, dtype=torch.float32, device="cuda")
    choice = torch.empty(w * h, dtype=torch.uint8, device="cuda")
    dn = spt.Denoiser(w, h, 0)
    stream = torch.cuda.current_stream().cuda_stream
    own = spt.DENOISE_PAIR_OWN_WEIGHTS
    sets = {2: (2.0, 8.0), 3: BANK_SIGMAS}

    def pairs(k):
        cands = spt.bank_candidates(sets[k])

        def run():
            for c in cands:
                dn.denoise_pair_async(*ptr, c, own, o[0], 0, o[2], stream)
        return run

    def bank(k):
        arr, n, b = spt._bank_args(spt.bank_candidates(sets[k]), None, True, None)

        def run():
            dn.denoise_bank_async(*ptr, arr, n, b, o[1], mse.data_ptr(), choice.data_ptr(), stream)
        return run

    what = [("pairs_2", pairs(2)), ("bank_2", bank(2)), ("pairs_3", pairs(3)), ("bank_3", bank(3))]
    ms = {k: [] for k, _ in what}
    try:
        for r in range(warmup + runs):
            for j in range(len(what)):
                name, run = what[(j + r) % len(what)]
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                run()
                b.record()
                torch.cuda.synchronize()
                if r >= warmup:
                    ms[name].append(a.elapsed_time(b))
    finally:
        dn.close()
    res = {k: _stat(v) for k, v in ms.items()}
    for k in (2, 3):
        over = np.array(ms[f"bank_{k}"]) - np.array(ms[f"pairs_{k}"])
        ratio = np.array(ms[f"bank_{k}"]) / np.array(ms[f"pairs_{k}"])
        res[f"overhead_{k}_ms_per_round"] = _stat(over)
        res[f"bank_over_pairs_{k}_per_round"] = {"median": float(np.median(ratio)), "min": float(ratio.min()),
                                                 "max": float(ratio.max())}
    return res


def bank_kernel_times(spt, torch, w, h, launches=50, rounds=7):
    """Per-launch milliseconds of the bank kernels alone, beside a plain pair a-trous pass."""
    import ctypes
    lib = spt.load_library()
    if not hasattr(lib, "spt_denoise_bank_bench_kernel"):
        return {"skipped": "the loaded library has no bench entry points (make denoise_bench)"}
    V, I32 = ctypes.c_void_p, ctypes.c_int32
    P = ctypes.POINTER(spt.spt_denoise_params)
    lib.spt_denoise_bank_bench_kernel.argtypes = [V, I32, I32, I32] + [V] * 4 + [P, V, V, V, V]
    lib.spt_denoise_bank_bench_kernel.restype = I32
    lib.spt_denoise_pair_bench_kernel.argtypes = [V, I32, I32, I32] + [V] * 7 + [P, ctypes.c_uint32, V, V, V, V]
    lib.spt_denoise_pair_bench_kernel.restype = I32
    dev = [torch.from_numpy(a.reshape(-1)).cuda() for a in _pair_planes(w, h)]
    ptr = [t.data_ptr() for t in dev]
    outs = [torch.empty(w * h * 3, dtype=torch.float32, device="cuda") for _ in range(3)]
    mse = torch.empty(w * h, dtype=torch.float32, device="cuda")
    choice = torch.empty(w * h, dtype=torch.uint8, device="cuda")
    p = spt.default_denoise_params()
    dn = spt.Denoiser(w, h, 0)
    stream = torch.cuda.current_stream().cuda_stream
    arr, n, b = spt._bank_args(spt.bank_candidates(BANK_SIGMAS), None, True, None)

    def bank_kernel(which, step):
        return lib.spt_denoise_bank_bench_kernel(dn._d, which, step, 3, *[V(x) for x in ptr[:4]], ctypes.byref(p),
                                                 V(outs[0].data_ptr()), V(mse.data_ptr()), V(choice.data_ptr()),
                                                 V(stream))

    def pair_kernel(which, step):
        return lib.spt_denoise_pair_bench_kernel(dn._d, which, step, 1, *[V(x) for x in ptr], ctypes.byref(p), 1,
                                                 *[V(t.data_ptr()) for t in outs], V(stream))

    def once(launch, *a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            assert launch(*a) == 0
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / launches

    what = [("bank_error", bank_kernel, 0, 1), ("bank_smooth_step1", bank_kernel, 1, 1),
            ("bank_smooth_step2", bank_kernel, 1, 2), ("bank_blend", bank_kernel, 2, 1),
            ("pair_halves_finish_step16_plain", bank_kernel, 3, 16),
            ("pair_atrous_step1_plain", pair_kernel, 2, 1), ("pair_atrous_step2_plain", pair_kernel, 2, 2),
            ("pair_atrous_step4_plain", pair_kernel, 2, 4), ("pair_atrous_finish_step16_plain", pair_kernel, 3, 16)]
    res = {"launches_per_round": launches, "rounds": rounds}
    try:
        dn.denoise_bank_async(*ptr, arr, n, b, outs[0].data_ptr(), mse.data_ptr(), choice.data_ptr(), stream)
        torch.cuda.synchronize()  # the scratch holds a packed pair, the halves and the estimates from here on
        ms = {name: [] for name, *_ in what}
        for name, launch, which, step in what:
            once(launch, which, step)
        for _ in range(rounds):
            for name, launch, which, step in what:
                ms[name].append(once(launch, which, step))
        res.update({k: _stat(v) for k, v in ms.items()})
    finally:
        dn.close()
    return res


def bank_quality(spt, name, w=256, h=192, seeds=16, spps=(64, 256, 1024)):
    prims = getattr(spt, PAIR_SCENES[name][0])()
    kw = PAIR_SCENES[name][1]
    cam = spt.Camera(aspect=float(np.float32(w) / np.float32(h)))
    truth = np.zeros((h, w, 3), np.float64)
    for s in range(16):
        truth += spt.render(prims, cam, spt.default_params(width=w, height=h, spp=4096, seed=1000 + s, **kw))
    truth = (truth / 16).astype(np.float32)
    masks = {"frame": np.ones((h, w), bool)}
    if name != "HEAD":
        masks.update(specular_masks(spt, prims, cam, w, h, **kw))
    res = {"scene": name, "width": w, "height": h, "seeds": seeds, "truth": "16 seeds x 4096 spp", "guide_spp": 64,
           "batches": 8, "sigma_colors": list(BANK_SIGMAS),
           "banks": {k: {"sigma_colors": list(v[0]), "own_weights": v[1], "error_iterations": 2 if v[2] is None else v[2]}
                     for k, v in BANK_VARIANTS.items()}, "pixels": {k: int(m.sum()) for k, m in masks.items()},
           "by_spp": {}}
    modes = list(BANK_VARIANTS) + [f"pair_{m}_{sc:g}" for m in ("own", "cross") for sc in BANK_SIGMAS]
    for spp in spps:
        batch = spp // 8
        outs = {m: [] for m in modes}
        mse_est = {m: [] for m in BANK_VARIANTS}
        choices = {m: [] for m in BANK_VARIANTS}
        diff2_own = {sc: [] for sc in BANK_SIGMAS}
        noisy_all = []
        for seed in range(1, seeds + 1):
            p = spt.default_params(width=w, height=h, spp=spp, seed=seed, **kw)
            r, fa, fb, film, guide, dn = (spt.Renderer(0), spt.Film(p, 0), spt.Film(p, 0), spt.Film(p, 0),
                                          spt.Guide(p, 0), spt.Denoiser(w, h, 0))
            try:
                for f in (fa, fb, film):
                    f.enable_noise(batch)
                for k in range(8):
                    (fb if k & 1 else fa).render(r, prims, cam, p, k * batch, batch)
                    r.stats()
                film.merge(fa)
                film.merge(fb)
                guide.render(r, prims, cam, p, 0, min(spp, 64))
                noisy_all.append(film.resolve())
                for v, (sigmas, own, passes) in BANK_VARIANTS.items():
                    out, mse, choice = dn.denoise_film_bank(fa, fb, guide, spt.bank_candidates(sigmas), None, own,
                                                            passes)
                    outs[v].append(out)
                    mse_est[v].append(float(mse.mean(dtype=np.float64)))
                    choices[v].append(choice)
                for m, own in (("own", True), ("cross", False)):
                    for sc in BANK_SIGMAS:
                        out, _se, diff = dn.denoise_film_pair(fa, fb, guide, spt.default_denoise_params(sigma_color=sc),
                                                              own)
                        outs[f"pair_{m}_{sc:g}"].append(out)
                        if own:
                            diff2_own[sc].append(float(np.mean(diff.astype(np.float64) ** 2)))
            finally:
                for o in (dn, guide, film, fa, fb, r):
                    o.close()
        one = {"regions": {}, "calibration": {}}
        for k, mk in masks.items():
            nz = float(np.mean([rmse(x[mk], truth[mk]) for x in noisy_all]))
            row = {"rmse_noisy": nz}
            for m in modes:
                row[f"ratio_{m}"] = float(np.mean([rmse(x[mk], truth[mk]) for x in outs[m]])) / nz
            for m, (sigmas, _own, _passes) in BANK_VARIANTS.items():
                if len(sigmas) > 1:
                    row[f"share_{m}"] = [float(np.mean([(c[mk] == j).mean() for c in choices[m]]))
                                         for j in range(len(sigmas))]
            one["regions"][k] = row
        for m in BANK_VARIANTS:
            true = float(np.mean((np.stack(outs[m]).astype(np.float64) - truth.astype(np.float64)) ** 2))
            one["calibration"][m] = {"mean_mse_estimate": float(np.mean(mse_est[m])), "mse_against_truth": true,
                                     "mse_over_truth": float(np.mean(mse_est[m])) / true}
        for sc in BANK_SIGMAS:
            true = float(np.mean((np.stack(outs[f"pair_own_{sc:g}"]).astype(np.float64) - truth.astype(np.float64)) ** 2))
            one["calibration"][f"pair_own_{sc:g}"] = {"diff2_over_truth": float(np.mean(diff2_own[sc])) / true}
        res["by_spp"][str(spp)] = one
    return res


def main_bank(out):
    import torch
    spt = importlib.import_module("small-pathtracer_amd")
    spt.load_library()
    assert torch.cuda.is_available(), "denoise_bench needs the GPU"
    rec = {"kernel_sources_sha16": spt.build_sources_sha16(), "device": torch.cuda.get_device_name(0),
           "utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()), "time": {}, "kernels": {}}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    for w, h in ((1024, 768), (4096, 4096)):
        rec["time"][f"{w}x{h}"] = time_bank(spt, torch, w, h)
        rec["kernels"][f"{w}x{h}"] = bank_kernel_times(spt, torch, w, h)
        json.dump(rec, open(out, "w"), indent=1)
        print(f"{w}x{h}", json.dumps(rec["time"][f"{w}x{h}"]), json.dumps(rec["kernels"][f"{w}x{h}"]), flush=True)
    rec["quality"] = {}
    for name in PAIR_SCENES:
        rec["quality"][name] = bank_quality(spt, name)
        json.dump(rec, open(out, "w"), indent=1)  # what is measured survives a failure further on
        print(name, json.dumps(rec["quality"][name]["by_spp"]), flush=True)


# ---- --light-guide: the albedo plane shaded by a light guide's visibility --------------------------------
LIGHT_FLOORS = (0.1, 0.25, 0.5)


def _light_scene_params(name, p):
    if name == "mirror_glass":  # the classic box: a square of the light sphere's cap (tools/guide_bench.py)
        p.light_id = 8
        p.light_x0, p.light_dx, p.light_z0, p.light_dz = 38.0, 24.0, 69.6, 24.0
        p.light_y, p.light_area = 81.6, 576.0
    return p


def _dilate(mask, radius):
    out = mask.copy()
    h, w = mask.shape
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            ys, yd = (slice(max(dy, 0), h + min(dy, 0)), slice(max(-dy, 0), h + min(-dy, 0)))
            xs, xd = (slice(max(dx, 0), w + min(dx, 0)), slice(max(-dx, 0), w + min(-dx, 0)))
            out[yd, xd] |= mask[ys, xs]
    return out


def light_quality(spt, name, w=256, h=192, seeds=16, spps=(64, 256, 1024)):
    prims = getattr(spt, PAIR_SCENES[name][0])()
    kw = PAIR_SCENES[name][1]
    cam = spt.Camera(aspect=float(np.float32(w) / np.float32(h)))
    truth = np.zeros((h, w, 3), np.float64)
    for s in range(16):
        truth += spt.render(prims, cam, spt.default_params(width=w, height=h, spp=4096, seed=1000 + s, **kw))
    truth = (truth / 16).astype(np.float32)
    ref = spt.render_light_guides(prims, cam, _light_scene_params(
        name, spt.default_params(width=w, height=h, spp=1024, seed=1000, **kw)))
    band = _dilate((ref["visibility"] > 0.05) & (ref["visibility"] < 0.95), 2)
    masks = {"frame": np.ones((h, w), bool), "shadow_band": band, "rest": ~band}
    variants = ["off"] + [f"floor_{f}" for f in LIGHT_FLOORS]
    res = {"scene": name, "width": w, "height": h, "seeds": seeds, "truth": "16 seeds x 4096 spp", "guide_spp": 64,
           "light_guide_spp": 64, "band": "0.05 < visibility < 0.95 at 1024 samples (seed 1000), dilated by 2",
           "batches": 8, "pixels": {k: int(m.sum()) for k, m in masks.items()},
           "reference_visibility_mean": float(ref["visibility"].mean()),
           "reference_tested_mean": float(ref["tested"].mean()), "by_spp": {}}
    for spp in spps:
        batch = spp // 8
        outs = {(f, v): [] for f in ("single", "cross") for v in variants}
        noisy_all = []
        for seed in range(1, seeds + 1):
            p = _light_scene_params(name, spt.default_params(width=w, height=h, spp=spp, seed=seed, **kw))
            r, fa, fb, film, guide, lg, dn = (spt.Renderer(0), spt.Film(p, 0), spt.Film(p, 0), spt.Film(p, 0),
                                              spt.Guide(p, 0), spt.LightGuide(p, 0), spt.Denoiser(w, h, 0))
            try:
                for f in (fa, fb, film):
                    f.enable_noise(batch)
                for k in range(8):
                    (fb if k & 1 else fa).render(r, prims, cam, p, k * batch, batch)
                    r.stats()
                film.merge(fa)
                film.merge(fb)
                guide.render(r, prims, cam, p, 0, min(spp, 64))
                lg.render(r, prims, cam, p, 0, min(spp, 64))
                g, vis = guide.resolve(), lg.resolve(("visibility",))["visibility"]
                rgb, se = film.resolve(), film.noise_map()
                halves = [fa.resolve(), fa.noise_map(), fb.resolve(), fb.noise_map()]
                noisy_all.append(rgb)
                outs[("single", "off")].append(dn.denoise_film(film, guide))
                outs[("cross", "off")].append(dn.denoise_film_pair(fa, fb, guide)[0])
                for f in LIGHT_FLOORS:
                    shaded = spt.light_shade(g["albedo"], vis, f)
                    outs[("single", f"floor_{f}")].append(dn.denoise(rgb, se, shaded, g["normal"], g["depth"]))
                    outs[("cross", f"floor_{f}")].append(dn.denoise_pair(*halves, shaded, g["normal"], g["depth"])[0])
            finally:
                for o in (dn, lg, guide, film, fa, fb, r):
                    o.close()
        one = {"regions": {}, "mean_change": {}}
        noisy_mean = float(np.mean([x.mean(dtype=np.float64) for x in noisy_all]))
        for k, mk in masks.items():
            n = float(np.mean([rmse(x[mk], truth[mk]) for x in noisy_all]))
            row = {"rmse_noisy": n}
            for f in ("single", "cross"):
                per = {v: [rmse(x[mk], truth[mk]) for x in outs[(f, v)]] for v in variants}
                for v in variants:
                    row[f"ratio_{f}_{v}"] = float(np.mean(per[v])) / n
                for v in variants[1:]:
                    row[f"{f}_{v}_over_off"] = float(np.mean(per[v]) / np.mean(per["off"]))
                    row[f"seeds_where_{f}_{v}_beats_off"] = int(sum(a < b for a, b in zip(per[v], per["off"])))
            one["regions"][k] = row
        for (f, v), xs in outs.items():
            one["mean_change"][f"{f}_{v}"] = float(np.mean([x.mean(dtype=np.float64) for x in xs]) / noisy_mean - 1.0)
        res["by_spp"][str(spp)] = one
    return res


def main_light(out):
    import torch
    spt = importlib.import_module("small-pathtracer_amd")
    spt.load_library()
    assert torch.cuda.is_available(), "denoise_bench needs the GPU"
    rec = {"kernel_sources_sha16": spt.build_sources_sha16(), "device": torch.cuda.get_device_name(0),
           "utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()), "shade_floors": list(LIGHT_FLOORS), "quality": {}}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    for name in PAIR_SCENES:
        rec["quality"][name] = light_quality(spt, name)
        json.dump(rec, open(out, "w"), indent=1)  # what is measured survives a failure further on
        print(name, json.dumps({s: v["regions"]["shadow_band"] for s, v in rec["quality"][name]["by_spp"].items()}),
              flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--light-guide":
        return main_light(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "build", "guide_light_denoise.json"))
    if len(sys.argv) > 1 and sys.argv[1] == "--chain":
        return main_chain(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "build", "guide_chain_denoise.json"))
    if len(sys.argv) > 1 and sys.argv[1] == "--pair":
        return main_pair(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "build", "r27_denoise_pair.json"))
    if len(sys.argv) > 1 and sys.argv[1] == "--bank":
        return main_bank(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "build", "r28_denoise_bank.json"))
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "build", "r19_denoise.json")
    import torch
    spt = importlib.import_module("small-pathtracer_amd")
    spt.load_library()
    assert torch.cuda.is_available(), "denoise_bench needs the GPU"
    rec = {"kernel_sources_sha16": spt.build_sources_sha16(), "device": torch.cuda.get_device_name(0),
           "utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()), "time": {}}
    rec["kernels"] = {}
    for w, h in ((1024, 768), (4096, 4096)):
        rec["time"][f"{w}x{h}"] = time_denoise(spt, torch, w, h)
        rec["kernels"][f"{w}x{h}"] = kernel_times(spt, torch, w, h)
    rec["test_quality"] = test_quality(spt)
    p = spt.default_params(width=1024, height=768, spp=64, seed=1)
    cam = spt.Camera(aspect=float(np.float32(1024) / np.float32(768)))
    ms = []
    for _ in range(4):
        _, st = spt.render(spt.cornell_scene(), cam, p, return_stats=True)
        ms.append(st["kernel_ms"])
    rec["render_kernel_ms_1024x768_64spp"] = float(np.median(ms[1:]))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    json.dump(rec, open(out, "w"), indent=1)  # the timings survive a failure below
    rec["quality"] = quality(spt)
    json.dump(rec, open(out, "w"), indent=1)
    print(json.dumps({"time_1024x768": rec["time"]["1024x768"]["iteration_ms_steps_2_to_32"],
                      "default": rec["quality"]["variants"]["default"]}))


if __name__ == "__main__":
    main()

"""Temporal accumulation on the GPU (include/spt.h SPT_HAS_TEMPORAL; spt_temporal.hip): every comparison
of the kernel is bit for bit against the host statement spt_temporal_accumulate_host, which
tests/test_temporal.py pins to the header's text; then the film path, render_sequence, and what the
feature is for: an orbiting camera's last frame is closer to the truth with its history than without.
"""
import numpy as np
import pytest

import temporal_truth as tt

pytestmark = pytest.mark.gpu
W, H, SPP, BATCH, GUIDE_SPP = 64, 48, 16, 4, 16
FILL = -7.25
OUTS = (("rgb", 3), ("se", 3), ("n", 1), ("hist", 3))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want, label):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, label
    diff = np.argwhere(bits(got) != bits(want))
    assert diff.size == 0, f"{label}: {len(diff)} values differ, first at {diff[:3].tolist()}: " \
                           f"{[(float(got[tuple(i)]), float(want[tuple(i)])) for i in diff[:3]]}"


def same_result(got, want, label, keys=("rgb", "se", "n", "hist")):
    for k in keys:
        same(got[k], want[k], f"{label}: {k}")


def same_state(got, want, label):
    for k in tt.STATE_PLANES:
        same(got[k], want[k], f"{label}: state {k}")


def rmse(a, b, mask=None):
    d = (a.astype(np.float64) - b.astype(np.float64)) ** 2
    return float(np.sqrt(np.mean(d if mask is None else d[mask])))


def _aspect(w, h):
    return float(np.float32(w) / np.float32(h))


def _upload(torch, planes):
    return [torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1)).cuda() for a in planes]


# ---- 1. device equals host on the synthetic sequences ---------------------------------------------
SYNTH_SIZES = [(1, 1), (3, 2), (17, 13), (70, 50), (300, 4), (4, 300)]


@pytest.mark.parametrize("w,h", SYNTH_SIZES, ids=[f"{w}x{h}" for w, h in SYNTH_SIZES])
def test_device_equals_host_on_synthetic_sequences(spt, w, h):
    """Three chained frames (first, same camera, moved camera: the ping-pong is crossed twice), both flag
    values, n_out and hist given and left null, outputs one float too long and filled with NaN."""
    import torch
    cam0, cam1 = tt.camera(w, h), tt.camera(w, h, origin=(1.3, -0.7, 0.5))
    seq = [(tt.frame(cam0, w, h, 1), cam0), (tt.frame(cam0, w, h, 2), cam0), (tt.frame(cam1, w, h, 3), cam1)]
    dev = [_upload(torch, tt.planes_of(f)) for f, _ in seq]
    n = w * h
    full, bare = spt.TemporalAccumulator(w, h, 0), spt.TemporalAccumulator(w, h, 0)
    try:
        for flags in (0, spt.TEMPORAL_NO_DEMODULATE):
            p = spt.default_temporal_params(flags=flags)
            full.reset()
            bare.reset()
            assert full.info() == {"frames": 0, "width": w, "height": h, "has_history": False}
            with pytest.raises(spt.SptError):
                full.state_to_numpy()
            prev, prev_cam = None, None
            for k, (f, cam) in enumerate(seq):
                cs = tt.to_struct(spt, cam)
                want = spt.temporal_accumulate_host(*tt.planes_of(f), cs, p, prev,
                                                    tt.to_struct(spt, prev_cam) if prev is not None else None)
                o = {key: torch.full((n * c + 1,), float("nan"), dtype=torch.float32, device="cuda") for key, c in OUTS}
                ptr = [t.data_ptr() for t in dev[k]]
                full.accumulate_async(*ptr, cs, p, o["rgb"].data_ptr(), o["se"].data_ptr(), o["n"].data_ptr(),
                                      o["hist"].data_ptr())
                b = {key: torch.full((n * 3 + 1,), float("nan"), dtype=torch.float32, device="cuda")
                     for key in ("rgb", "se")}
                bare.accumulate_async(*ptr, cs, p, b["rgb"].data_ptr(), b["se"].data_ptr())
                torch.cuda.synchronize()
                label = f"{w}x{h} flags={flags} frame {k}"
                for key, c in OUTS:
                    got = o[key].cpu().numpy()
                    assert np.isnan(got[n * c]), f"{label}: a write past {key}"
                    same(got[:n * c].reshape(want[key].shape), want[key], f"{label}: {key}")
                for key in ("rgb", "se"):
                    got = b[key].cpu().numpy()
                    assert np.isnan(got[n * 3]), f"{label}: a write past {key} (no optional planes)"
                    same(got[:n * 3].reshape(h, w, 3), want[key], f"{label}: {key} without the optional planes")
                state, cam_back = full.state_to_numpy(return_camera=True)
                same_state(state, want["state"], label)
                same_state(bare.state_to_numpy(), want["state"], label + " (no optional planes)")
                assert list(cam_back.origin) == list(cs.origin) and list(cam_back.vertical) == list(cs.vertical)
                assert full.info()["frames"] == k + 1 and full.info()["has_history"]
                prev, prev_cam = want["state"], cam
            if min(w, h) >= 13:  # the moved camera did reproject
                assert np.any(want["hist"] != seq[2][0]["rgb"])
    finally:
        full.close()
        bare.close()


def test_the_host_wrapper_equals_the_async_call(spt):
    w, h = 17, 13
    cam = tt.camera(w, h)
    f = tt.frame(cam, w, h, 1)
    acc = spt.TemporalAccumulator(w, h, 0)
    try:
        first = acc.accumulate(*tt.planes_of(f), tt.to_struct(spt, cam))
        second = acc.accumulate(*tt.planes_of(f), tt.to_struct(spt, cam))
        w1 = spt.temporal_accumulate_host(*tt.planes_of(f), tt.to_struct(spt, cam))
        w2 = spt.temporal_accumulate_host(*tt.planes_of(f), tt.to_struct(spt, cam), None, w1["state"],
                                          tt.to_struct(spt, cam))
        same_result(first, w1, "first")
        same_result(second, w2, "second")
        with pytest.raises(spt.SptError):
            acc.accumulate(*tt.planes_of(tt.frame(tt.camera(5, 3), 5, 3, 1)), tt.to_struct(spt, cam))
    finally:
        acc.close()


def test_rejected_plane_calls_leave_outputs_and_state_untouched(spt):
    import torch
    w, h = 17, 13
    cam = tt.camera(w, h)
    cs = tt.to_struct(spt, cam)
    f = tt.frame(cam, w, h, 1)
    dev = _upload(torch, tt.planes_of(f))
    ptr = [t.data_ptr() for t in dev]
    n = w * h
    o = {key: torch.full((n * c,), FILL, dtype=torch.float32, device="cuda") for key, c in OUTS}
    op = [o[key].data_ptr() for key, _ in OUTS]
    ok = spt.default_temporal_params
    nan, inf = float("nan"), float("inf")
    bad_params = [ok(n_max=0.5), ok(n_max=nan), ok(n_max=inf), ok(normal_min=1.5), ok(normal_min=nan),
                  ok(plane_tol=-1.0), ok(plane_tol=inf), ok(albedo_floor=0.0), ok(albedo_floor=nan), ok(flags=2),
                  ok(flags=0x80000001), ok(reserved=1)]
    flat = cam.copy()
    flat[3] = flat[2]
    acc = spt.TemporalAccumulator(w, h, 0)

    def refused(call, label):
        with pytest.raises(spt.SptError) as e:
            call()
        assert e.value.status == 1, label
        torch.cuda.synchronize()
        assert all(bool((t == FILL).all()) for t in o.values()), label

    try:
        want1 = acc.accumulate(*tt.planes_of(f), cs)
        state = acc.state_to_numpy()
        for k in range(5):
            a = list(ptr)
            a[k] = 0
            refused(lambda: acc.accumulate_async(*a, cs, ok(), *op), f"null plane {k}")
            for j in range(4):
                b = list(op)
                b[j] = ptr[k]
                refused(lambda: acc.accumulate_async(*ptr, cs, ok(), *b), f"output {j} is input {k}")
        for j in range(4):
            for i in range(j):
                b = list(op)
                b[j] = b[i]
                refused(lambda: acc.accumulate_async(*ptr, cs, ok(), *b), f"output {j} is output {i}")
        refused(lambda: acc.accumulate_async(*ptr, cs, ok(), 0, op[1], op[2], op[3]), "null rgb_out")
        refused(lambda: acc.accumulate_async(*ptr, cs, ok(), op[0], 0, op[2], op[3]), "null se_out")
        for i, bp in enumerate(bad_params):
            refused(lambda: acc.accumulate_async(*ptr, cs, bp, *op), f"params {i}")
        refused(lambda: acc.accumulate_async(*ptr, tt.to_struct(spt, flat), ok(), *op), "a singular camera")
        for ww, hh in [(0, 4), (4, 0), (-1, 4), (65536, 32768), (1, 67108861)]:
            with pytest.raises(spt.SptError) as e:
                spt.TemporalAccumulator(ww, hh, 0)
            assert e.value.status == 1
        # the state is the first frame's still: the next frame is the host's second
        assert acc.info()["frames"] == 1
        same_state(acc.state_to_numpy(), state, "after the refusals")
        got2 = acc.accumulate(*tt.planes_of(f), cs)
        want2 = spt.temporal_accumulate_host(*tt.planes_of(f), cs, None, state, cs)
        same_result(got2, want2, "the frame after the refusals")
        same_result(want1, spt.temporal_accumulate_host(*tt.planes_of(f), cs), "the first frame")
    finally:
        acc.close()


# ---- 2. the film path -----------------------------------------------------------------------------
def _cams(spt, n, degrees=2.0):
    return spt.orbit_cameras(n, degrees, aspect=_aspect(W, H))


def _frame(spt, r, prims, cam, seed, adaptive=False, through_specular=False):
    """-> (film, guide, params): 64x48, 16 spp in batches of 4, a guide of 16 samples; an adaptive film has
    had one selection after two batches."""
    p = spt.default_params(width=W, height=H, spp=SPP, seed=seed)
    film, guide = spt.Film(p, 0), spt.Guide(p, 0, through_specular)
    film.enable_noise(BATCH)
    if adaptive:
        film.enable_adaptive()
    for k in range(SPP // BATCH):
        if adaptive and k == 2:
            left = film.adaptive_select(0.05)
            assert 0 < left < W * H, left
        film.render(r, prims, cam, p, k * BATCH, BATCH)
        r.stats()
    guide.render(r, prims, cam, p, 0, GUIDE_SPP)
    return film, guide, p


@pytest.mark.parametrize("adaptive", [False, True], ids=["plain", "adaptive"])
def test_film_accumulate_equals_the_plane_call(spt, adaptive):
    import torch
    prims = spt.cornell_scene()
    r = spt.Renderer(0)
    fused_acc, apart_acc = spt.TemporalAccumulator(W, H, 0), spt.TemporalAccumulator(W, H, 0)
    n = W * H
    try:
        for k, cam in enumerate(_cams(spt, 3)):
            film, guide, _ = _frame(spt, r, prims, cam, 5 + k, adaptive)
            try:
                sums, rec = film.to_numpy(), guide.to_numpy()
                o = {key: torch.full((n * c,), FILL, dtype=torch.float32, device="cuda") for key, c in OUTS}
                g_out = {key: torch.full((n * c,), FILL, dtype=torch.float32, device="cuda")
                         for key, c in (("albedo", 3), ("normal", 3), ("depth", 1))}
                fused_acc.accumulate_film_async(film, guide, cam, spt.default_temporal_params(),
                                                *[o[key].data_ptr() for key, _ in OUTS],
                                                *[g_out[key].data_ptr() for key in ("albedo", "normal", "depth")])
                torch.cuda.synchronize()
                g = guide.resolve()
                planes = [film.resolve(), film.noise_map(), g["albedo"], g["normal"], g["depth"]]
                apart = apart_acc.accumulate(*planes, cam)
                for key, _ in OUTS:
                    same(o[key].cpu().numpy().reshape(apart[key].shape), apart[key], f"frame {k}: {key}")
                for key in g_out:
                    same(g_out[key].cpu().numpy().reshape(g[key].shape), g[key], f"frame {k}: guide plane {key}")
                same_state(fused_acc.state_to_numpy(), apart_acc.state_to_numpy(), f"frame {k}")
                # ... and without the guide planes asked for, through the wrapper
                if k == 0:
                    again = spt.TemporalAccumulator(W, H, 0)
                    try:
                        same_result(again.accumulate_film(film, guide, cam), apart, "accumulate_film")
                    finally:
                        again.close()
                assert np.array_equal(film.to_numpy(), sums) and np.array_equal(guide.to_numpy(), rec)
                if k:
                    assert (apart["n"] > 1).mean() > 0.5, "the orbit reprojects most of the frame"
            finally:
                guide.close()
                film.close()
    finally:
        fused_acc.close()
        apart_acc.close()
        r.close()


def test_film_accumulate_refusals_queue_nothing(spt):
    """A chain guide, a plain film, a sharded film and a size mismatch: refused, the outputs untouched, and
    the frame that follows equals the unperturbed run's."""
    import torch
    prims = spt.cornell_scene()
    cams = _cams(spt, 3)
    r = spt.Renderer(0)
    calm, upset, small = (spt.TemporalAccumulator(W, H, 0), spt.TemporalAccumulator(W, H, 0),
                          spt.TemporalAccumulator(W - 1, H, 0))
    n = W * H
    o = {key: torch.full((n * c,), FILL, dtype=torch.float32, device="cuda") for key, c in OUTS}
    op = [o[key].data_ptr() for key, _ in OUTS]
    frames = [_frame(spt, r, prims, cam, 5 + k) for k, cam in enumerate(cams)]
    p = frames[2][2]
    chain = spt.Guide(p, 0, True)
    chain.render(r, prims, cams[2], p, 0, GUIDE_SPP)
    plain = spt.Film(p, 0)
    young = spt.Film(p, 0)
    young.enable_noise(BATCH)
    young.render(r, prims, cams[2], p, 0, BATCH)
    empty_guide = spt.Guide(p, 0)
    p2 = spt.default_params(width=W, height=H, spp=SPP, seed=7, shard_index=0, shard_count=2, tile_rows=8)
    shard_film = spt.Film(p2, 0)
    shard_film.enable_noise(BATCH)
    for k in range(2):
        shard_film.render(r, prims, cams[2], p2, k * BATCH, BATCH)
    ok = spt.default_temporal_params()

    def refused(call, label):
        with pytest.raises(spt.SptError) as e:
            call()
        assert e.value.status == 1, label
        torch.cuda.synchronize()
        assert all(bool((t == FILL).all()) for t in o.values()), label

    try:
        for acc in (calm, upset):
            for k in range(2):
                acc.accumulate_film(frames[k][0], frames[k][1], cams[k])
        film, guide = frames[2][0], frames[2][1]
        before = upset.state_to_numpy()
        refused(lambda: upset.accumulate_film_async(film, chain, cams[2], ok, *op), "a chain guide")
        refused(lambda: upset.accumulate_film_async(plain, guide, cams[2], ok, *op), "a plain film")
        refused(lambda: upset.accumulate_film_async(young, guide, cams[2], ok, *op), "one batch")
        refused(lambda: upset.accumulate_film_async(film, empty_guide, cams[2], ok, *op), "an empty guide")
        refused(lambda: upset.accumulate_film_async(shard_film, guide, cams[2], ok, *op), "a sharded film")
        refused(lambda: small.accumulate_film_async(film, guide, cams[2], ok, *op), "a size mismatch")
        refused(lambda: upset.accumulate_film_async(film, guide, cams[2], spt.default_temporal_params(flags=4), *op),
                "flag bits")
        refused(lambda: upset.accumulate_film_async(film, guide, cams[2], ok, op[0], op[1], op[2], op[3], op[0]),
                "the albedo plane is rgb_out")
        assert upset.info()["frames"] == 2 and small.info()["frames"] == 0
        same_state(upset.state_to_numpy(), before, "after the refusals")
        want = calm.accumulate_film(film, guide, cams[2])
        got = upset.accumulate_film(film, guide, cams[2])
        same_result(got, want, "the frame after the refusals")
        same_state(upset.state_to_numpy(), calm.state_to_numpy(), "the frame after the refusals")
    finally:
        for x in (calm, upset, small, chain, plain, young, empty_guide, shard_film, r):
            x.close()
        for film, guide, _ in frames:
            guide.close()
            film.close()


# ---- 3. render_sequence ---------------------------------------------------------------------------
def test_render_sequence_without_temporal_is_render_denoised(spt):
    prims = spt.cornell_scene()
    cams = _cams(spt, 2)
    p = spt.default_params(width=W, height=H, spp=SPP, seed=11)
    dp = spt.default_denoise_params(iterations=3)
    got = spt.render_sequence(prims, cams, p, batch=BATCH, temporal=False, denoise_params=dp)
    assert len(got) == 2
    for k, cam in enumerate(cams):
        pk = spt.default_params(width=W, height=H, spp=SPP, seed=11 + k)
        same(got[k], spt.render_denoised(prims, cam, pk, BATCH, denoise=dp), f"frame {k}")
    noisy = spt.render_sequence(prims, cams[1:], spt.default_params(width=W, height=H, spp=SPP, seed=12),
                                batch=BATCH, temporal=False, denoise=False)
    same(noisy[0], spt.render(prims, cams[1], spt.default_params(width=W, height=H, spp=SPP, seed=12)), "the film")


def test_render_sequence_equals_the_explicit_calls(spt):
    prims = spt.cornell_scene()
    cams = _cams(spt, 3)
    p = spt.default_params(width=W, height=H, spp=SPP, seed=5)
    tp = spt.default_temporal_params(n_max=8)
    got = spt.render_sequence(prims, cams, p, batch=BATCH, temporal_params=tp)
    film_only = spt.render_sequence(prims, cams, p, batch=BATCH, denoise=False, temporal_params=tp)
    r = spt.Renderer(0)
    acc, dn = spt.TemporalAccumulator(W, H, 0), spt.Denoiser(W, H, 0)
    try:
        for k, cam in enumerate(cams):
            film, guide, _ = _frame(spt, r, prims, cam, 5 + k)
            try:
                a = acc.accumulate_film(film, guide, cam, tp)
                g = guide.resolve()
                same(film_only[k], a["rgb"], f"frame {k}: accumulated")
                same(got[k], dn.denoise(a["rgb"], a["se"], g["albedo"], g["normal"], g["depth"]), f"frame {k}")
            finally:
                guide.close()
                film.close()
    finally:
        acc.close()
        dn.close()
        r.close()


# ---- 4. what it is for ----------------------------------------------------------------------------
QUALITY_SEEDS = (10, 20, 30, 40)
FRAMES, ORBIT = 8, 1.0
_truth = {}


def _scene_params(spt, scene, **kw):
    """mirror_glass has no light rectangle: pure path tracing, as its renders have."""
    if scene == "mirror_glass":
        kw["nee_prob"] = 0.0
    return spt.default_params(width=W, height=H, **kw)


def _orbit_truth(spt, scene):
    if scene not in _truth:
        prims = spt.cornell_scene() if scene == "head" else spt.smallpt_mirror_glass_scene()
        cams = spt.orbit_cameras(FRAMES, ORBIT, aspect=_aspect(W, H))
        p = _scene_params(spt, scene, spp=16384, seed=77)
        _truth[scene] = (prims, cams, spt.render(prims, cams[-1], p))
    return _truth[scene]


def _orbit_errors(spt, scene, seed, mask=None):
    prims, cams, truth = _orbit_truth(spt, scene)
    p = _scene_params(spt, scene, spp=SPP, seed=seed)
    last = _scene_params(spt, scene, spp=SPP, seed=seed + FRAMES - 1)
    images = {
        "film": spt.render_sequence(prims, cams[-1:], last, batch=BATCH, temporal=False, denoise=False)[0],
        "denoised": spt.render_sequence(prims, cams[-1:], last, batch=BATCH, temporal=False)[0],
        "accumulated": spt.render_sequence(prims, cams, p, batch=BATCH, denoise=False)[-1],
        "accumulated+denoised": spt.render_sequence(prims, cams, p, batch=BATCH)[-1],
    }
    return {k: rmse(v, truth, mask) for k, v in images.items()}, images, truth


@pytest.mark.parametrize("seed", QUALITY_SEEDS)
def test_an_orbit_accumulates_towards_the_truth(spt, seed):
    """HEAD at 64x48, eight frames of 16 spp in batches of 4, the camera orbiting 1 degree per frame; the
    truth is the last camera at 16384 spp. The last frame with its history must beat the last frame alone,
    as a film and after the filter. Frames that were independent and all accepted would give the film a
    ratio near 1/sqrt(8) = 0.35; the measured ratios are in profiles/r32_temporal.json."""
    e, _, _ = _orbit_errors(spt, "head", seed)
    print(f"seed {seed}: " + " ".join(f"{k} {v:.6f}" for k, v in e.items()) +
          f" ratios film {e['accumulated'] / e['film']:.4f} denoised {e['accumulated+denoised'] / e['denoised']:.4f}")
    assert e["accumulated+denoised"] < e["denoised"]
    assert e["accumulated"] < e["film"]


@pytest.mark.parametrize("seed", QUALITY_SEEDS)
def test_an_orbit_accumulates_on_the_diffuse_part_of_mirror_glass(spt, seed):
    """The same on mirror_glass, over the pixels whose first hit is DIFF. The balls (first hit SPEC or
    REFR) are the documented weak spot: what is seen in them lags the camera. They are measured and
    printed, not asserted."""
    prims, cams, _ = _orbit_truth(spt, "mirror_glass")
    refl = tt.first_hit_refl(prims, tt.camera_of(cams[-1]._c), W, H)
    diff, balls = refl == 0, refl > 0
    assert diff.mean() > 0.8 and balls.sum() > 100
    e, images, truth = _orbit_errors(spt, "mirror_glass", seed, diff)
    eb = {k: rmse(v, truth, balls) for k, v in images.items()}
    print(f"seed {seed}: DIFF " + " ".join(f"{k} {v:.6f}" for k, v in e.items()) +
          " | balls " + " ".join(f"{k} {v:.6f}" for k, v in eb.items()))
    assert e["accumulated+denoised"] < e["denoised"]
    assert e["accumulated"] < e["film"]


# ---- 5. the drop-in program -----------------------------------------------------------------------
def _read_pfm(path):
    raw = path.read_bytes()
    return np.frombuffer(raw[len(raw) - W * H * 12:], dtype="<f4").reshape(H, W, 3)[::-1]


def test_the_dropin_program_renders_an_orbit(spt, tmp_path):
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "small-pathtracer_amd",
                       "smallpt_amd")
    prims, cams = spt.cornell_scene(), _cams(spt, 3)
    p = spt.default_params(width=W, height=H, spp=SPP, seed=5)
    dp = spt.default_denoise_params(iterations=3, sigma_color=2.0)
    base = [exe, str(W), str(H), str(SPP), "5", str(tmp_path / "o.pfm"), "--pfm", "--frames", "3", "--orbit", "2",
            "--batch", str(BATCH)]
    dn = ["--denoise", "--denoise-iters", "3", "--denoise-sigma", "2"]
    cases = [
        (["--temporal", "--temporal-nmax", "8"] + dn,
         spt.render_sequence(prims, cams, p, batch=BATCH, denoise_params=dp,
                             temporal_params=spt.default_temporal_params(n_max=8))),
        (["--temporal"], spt.render_sequence(prims, cams, p, batch=BATCH, denoise=False)),
        (dn, spt.render_sequence(prims, cams, p, batch=BATCH, temporal=False, denoise_params=dp)),
        ([], spt.render_sequence(prims, cams, p, batch=BATCH, temporal=False, denoise=False)),
    ]
    for flags, want in cases:
        run = subprocess.run(base + flags, capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stdout + run.stderr
        for k in range(3):
            same(_read_pfm(tmp_path / f"o.{k:04d}.pfm"), want[k], f"smallpt_amd {' '.join(flags)} frame {k}")
    assert not (tmp_path / "o.pfm").exists()
    for bad in (["--temporal"], ["--frames", "3"], ["--frames", "3", "--orbit", "1", "--devices", "2"],
                ["--frames", "3", "--orbit", "1", "--noise", "0.01"], ["--frames", "2", "--orbit", "1", "--temporal-nmax", "4"],
                ["--frames", "2", "--orbit", "1", "--temporal", "--temporal-nmax", "0.5"]):
        run = subprocess.run([exe, str(W), str(H), str(SPP), "5", str(tmp_path / "bad.pfm")] + bad,
                             capture_output=True, text=True, timeout=120)
        assert run.returncode != 0 and ("--frames" in run.stderr or "--temporal" in run.stderr), bad
    usage = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert all(f in usage for f in ("--frames", "--orbit", "--temporal", "--temporal-nmax"))

"""The render loop's event counters (spt_kernel.hip, render_kernel): misses, shadow rays resolved,
shadow rays proven and traced light hits are counted on the scalar unit, by ballots at the convergent
top level of the trace-to-path-end region, which runs under a wave-uniform guard. Idle lanes run the
trace there on stale state, and nothing they compute may be counted or kept.

Each shape is the smallest at which that counting can go wrong on its own, and each render is compared
bit for bit with the oracle's counter mode over all its pixels: the image and every key of
spt.STAT_KEYS, no tolerance (the contract is exact). The variant that ran is the one the case means.
Where the early resolve matters, the proven shadow rays are the oracle's own count of the same claims
(oracle.proof_check)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LEAKS = 4  # SPT_FLAG_REFERENCE_LEAKS
TILTED = dict(lookfrom=(40, 55, 160), lookat=(55, 35, 10), vup=(0.1, 1, 0))

# family -> (scene, camera, spt_params fields, kernel cap, the variant, the variant with
# SPT_FLAG_REFERENCE_LEAKS)
FAMILIES = {
    "const_nee": ("head", {}, dict(), "auto", "const_nee", "const_nee_ref"),
    "const_cos": ("head", {}, dict(nee_prob=0.0), "auto", "const_cos", "const_cos_ref"),
    "moved_box": ("moved", {}, dict(), "auto", "upbox_nee", "cornell"),
    # (the reference-leaks kernels have no any-camera form: the run-time estimator's literal kernel)
    "tilted": ("head", TILTED, dict(), "auto", "const_nee_cam", "const"),
    "generic": ("specular", {}, dict(), "auto", "generic", "generic"),
}

SHAPES = {
    # lanes idle for the whole launch, in the wave that works: 63 and 61 of them
    "1x1_s1": dict(width=1, height=1, spp=1),
    "3x1_s1": dict(width=3, height=1, spp=1),
    # idle and busy lanes mixed, stale state in the idle ones: the queue dry at once and stealing all
    # the way down; a pool of one entry
    "2x2_s2048": dict(width=2, height=2, spp=2048),
    "13x5_s1": dict(width=13, height=5, spp=1),
    # every miss is counted, not only first misses
    "16x8_s7_leaks": dict(width=16, height=8, spp=7, flags=LEAKS),
    # the second of three shards
    "32x24_s4_shard": dict(width=32, height=24, spp=4, tile_rows=4, shard_index=1, shard_count=3),
}


def _scene(spt, name):
    if name == "head":
        return spt.cornell_scene()
    if name == "moved":
        return spt.move_short_box(spt.cornell_scene(), 3.0)
    if name == "spheres":
        return spt.spheres32_scene()
    return spt.cornell_specular_scene()


def _shard_pixels(spt, p):
    rows = np.asarray(spt.shard_rows(p), dtype=np.uint32)
    return (rows[:, None] * np.uint32(p.width) + np.arange(p.width, dtype=np.uint32)[None, :]).reshape(-1)


def _check(spt, oracle, prims, cam, p, kernel):
    gpu, st = spt.render(prims, cam, p, return_stats=True)
    pixels = _shard_pixels(spt, p)
    cpu, cst = oracle.counter_render_pixels(prims, cam._c, p, pixels)
    assert st["kernel"] == kernel
    assert gpu.shape == (len(pixels) // p.width, p.width, 3)
    assert np.array_equal(gpu.reshape(-1, 3), cpu)
    for k in spt.STAT_KEYS:
        assert st[k] == cst[k], (k, st[k], cst[k])
    assert st["samples"] == len(pixels) * p.spp
    return st, cst


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_event_counts(spt, oracle, shape, family):
    scene, camkw, pkw, level, kernel, kernel_leaks = FAMILIES[family]
    kw = dict(SHAPES[shape], **pkw)
    flags = kw.pop("flags", 0)
    p = spt.default_params(seed=7, device=0, flags=flags | spt.kernel_flag(level), **kw)
    cam = spt.Camera(aspect=p.width / p.height, **camkw)
    st, _ = _check(spt, oracle, _scene(spt, scene), cam, p, kernel_leaks if flags & LEAKS else kernel)
    if family == "generic":
        assert st["path_rays"] >= st["samples"] and st["cosine_samples"] <= st["path_rays"]


def test_all_four_event_kinds(spt, oracle):
    """64x48 @ 16 on the HEAD scene: misses, proven shadow rays, traced shadow rays and traced light
    hits are all present (asserted from the oracle's own statistics), and each count is the oracle's."""
    p = spt.default_params(width=64, height=48, spp=16, seed=7, device=0)
    cam = spt.Camera(aspect=64 / 48)
    prims = spt.cornell_scene()
    oracle.proof_check(True)
    try:
        st, cst = _check(spt, oracle, prims, cam, p, "const_nee")
        claims, bad = oracle.proof_counts()
    finally:
        oracle.proof_check(False)
    assert bad == 0
    assert cst["misses"] > 0                         # misses
    assert claims > 0                                # shadow rays proven
    assert cst["shadow_traced"] - claims > 0         # shadow rays traced
    assert cst["nee_light_hits"] - claims > 0        # traced shadow rays that reach the light
    assert cst["nee_light_hits"] < cst["shadow_traced"]  # ... and traced ones that do not
    assert st["shadow_proven"] == claims, (st["shadow_proven"], claims)


def test_sphere_nee_kernel(spt, oracle):
    """The sphere NEE kernel on the 32-sphere scene at 32x32 @ 4, depth cap 16: sphere vertices, and
    the proven shadow rays (counted by a ballot, no longer through LDS)."""
    p = spt.default_params(width=32, height=32, spp=4, seed=7, device=0, max_depth=16)
    cam = spt.Camera(aspect=1.0)
    oracle.proof_check(True, sphere_y0=13.0)
    try:
        st, cst = _check(spt, oracle, spt.spheres32_scene(), cam, p, "sphdiff_nee")
        claims, bad = oracle.proof_counts()
    finally:
        oracle.proof_check(False)
    assert bad == 0 and claims > 0
    assert cst["sphere_vertices"] > 0 and cst["misses"] > 0
    assert st["shadow_proven"] == claims, (st["shadow_proven"], claims)


def _minus(a, b):
    return {k: a[k] - b[k] for k in a}


@pytest.mark.parametrize("family", ["const_nee", "const_cos", "generic"])
def test_sample_window_and_pixel_list(spt, oracle, family):
    """An 8x8 film of 12 samples in batches of 4. The first pass renders samples [0, 4) of every
    pixel and the second the window [4, 8) (s_base > 0, no list); then all but 5 pixels retire, and
    the third pass renders the window [8, 12) over the list of those 5 (the LIST instantiation). A
    sample's path depends on its own index alone, so a window's statistics are the oracle's at the
    window's end less the oracle's at its start, over the same pixels; the listed pixels then hold all
    12 samples and resolve to the oracle's 12-sample image."""
    scene, camkw, pkw, level, kernel, _ = FAMILIES[family]
    w = h = 8
    batch = 4
    prims = _scene(spt, scene)

    def params(spp):
        return spt.default_params(width=w, height=h, spp=spp, seed=7, device=0,
                                  flags=spt.kernel_flag(level), **pkw)

    p = params(3 * batch)
    cam = spt.Camera(aspect=1.0, **camkw)
    everyone = np.arange(w * h, dtype=np.uint32)
    listed = np.array([0, 9, 27, 36, 63], dtype=np.uint32)
    keep = np.zeros(w * h, np.uint8)
    keep[listed] = 1
    _, all_4 = oracle.counter_render_pixels(prims, cam._c, params(batch), everyone)
    _, all_8 = oracle.counter_render_pixels(prims, cam._c, params(2 * batch), everyone)
    _, listed_8 = oracle.counter_render_pixels(prims, cam._c, params(2 * batch), listed)
    img_listed, listed_12 = oracle.counter_render_pixels(prims, cam._c, p, listed)
    want = [all_4, _minus(all_8, all_4), _minus(listed_12, listed_8)]
    got = []
    r, film = spt.Renderer(0), spt.Film(p, 0)
    try:
        film.enable_noise(batch)
        film.enable_adaptive()
        for k in range(3):
            if k == 2:
                assert film.adaptive_select(-1.0, keep.reshape(h, w)) == len(listed)
            film.render(r, prims, cam, p, k * batch, batch)
            got.append(r.stats())
            assert r.kernel() == kernel
        res = film.resolve()
    finally:
        film.close()
        r.close()
    for k in spt.STAT_KEYS:
        for n in range(3):
            assert got[n][k] == want[n][k], (n, k, got[n][k], want[n][k])
    assert got[2]["samples"] == len(listed) * batch
    assert np.array_equal(res.reshape(-1, 3)[listed], img_listed)

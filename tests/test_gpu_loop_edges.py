"""The edges of the render loop (spt_kernel.hip, render_kernel): the loop's exit (one scalar
condition at the back edge: no lane with work, or the runaway guard), the one-pass refill of the
idle lanes, in-wave stealing, and the wave-uniform counters.

Each shape is one at which the exit, the refill or a counter can go wrong on its own, and each is
rendered by the literal NEE and cosine kernels, an uploaded-geometry variant (the short box moved)
and the generic kernel. Every render is compared bit for bit, the image and every statistic, with
the oracle's counter mode over all pixels (no tolerance: the contract is exact), and the variant that
ran is the one the case means. No case runs a wave into the runaway guard."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LEAKS = 4  # SPT_FLAG_REFERENCE_LEAKS

# (scene, spt_params fields, kernel cap) -> the variant with and without SPT_FLAG_REFERENCE_LEAKS
VARIANTS = {
    "const_nee": ("head", dict(), "auto", "const_nee", "const_nee_ref"),
    "const_cos": ("head", dict(nee_prob=0.0), "auto", "const_cos", "const_cos_ref"),
    "moved_box": ("moved", dict(), "auto", "upbox_nee", "cornell"),
    "generic": ("head", dict(), "generic", "generic", "generic"),
}

SHAPES = {
    # 1 unit: every wave but one finds the queue dry at its first refill and leaves at once
    "1x1_s1": dict(width=1, height=1, spp=1),
    # 64 units: exactly one pool, every lane of one wave served by one fill
    "8x8_s1": dict(width=8, height=8, spp=1),
    # 65 units: the 65th is a pool of its own (a fill of one entry)
    "13x5_s1": dict(width=13, height=5, spp=1),
    # 9216 units of one sample: many pools per wave, s_end reached at every sample, and pools whose
    # last units do not serve every idle lane (the others take theirs an iteration later)
    "64x48_s3_chunk1": dict(width=64, height=48, spp=3, chunk=1),
    # 4 pixels: the queue is dry at once, the lanes split the ranges by stealing all the way down,
    # and the stolen ranges add into the accumulator with atomics
    "2x2_s2048": dict(width=2, height=2, spp=2048),
    # leaked paths go on from their miss vertex (the LEAK == 0 kernels)
    "16x8_s7_leaks": dict(width=16, height=8, spp=7, flags=LEAKS),
}


def _scene(spt, name):
    if name == "head":
        return spt.cornell_scene()
    if name == "moved":
        return spt.move_short_box(spt.cornell_scene(), 3.0)
    return spt.cornell_specular_scene()


def _check(spt, oracle, prims, p, kernel):
    cam = spt.Camera(aspect=p.width / p.height)
    gpu, st = spt.render(prims, cam, p, return_stats=True)
    pixels = np.arange(p.width * p.height, dtype=np.uint32)
    cpu, cst = oracle.counter_render_pixels(prims, cam._c, p, pixels)
    assert st["kernel"] == kernel
    assert gpu.shape == (p.height, p.width, 3)
    assert np.array_equal(gpu.reshape(-1, 3), cpu)
    for k in spt.STAT_KEYS:
        assert st[k] == cst[k], (k, st[k], cst[k])
    assert st["samples"] == p.width * p.height * p.spp
    return st


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_loop_edge(spt, oracle, shape, variant):
    scene, pkw, level, kernel, kernel_leaks = VARIANTS[variant]
    kw = dict(SHAPES[shape], **pkw)
    flags = kw.pop("flags", 0)
    p = spt.default_params(seed=7, device=0, flags=flags | spt.kernel_flag(level), **kw)
    _check(spt, oracle, _scene(spt, scene), p, kernel_leaks if flags & LEAKS else kernel)


def test_spec_refr_restart(spt, oracle):
    """Mirror and glass balls at 16x16 @ 4 spp (the generic kernel): n_path counts the SPEC/REFR
    rays that restart at kStSpec, and a REFR split's pending child is popped at the path end."""
    p = spt.default_params(width=16, height=16, spp=4, seed=7, device=0)
    st = _check(spt, oracle, _scene(spt, "spec"), p, "generic")
    assert st["path_rays"] > st["samples"]

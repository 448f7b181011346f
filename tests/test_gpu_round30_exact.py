"""Round 30's instruction choices change no bit: every render-kernel variant that took one (the literal
kernels: a random word's unit-interval float as one funnel shift, the hit's plane axis in the slot's
bits, a miss that reads its own table entry; spt_variants.h, KernelTraits) and `generic` as the
control, 64x48 @ 16 spp, against the oracle's counter mode: the image bit for bit and the statistics.

The HEAD scene, a moved short box (upbox_*) and a light at y = 81.4 (uplight_*), the reference camera
and a tilted one (*_cam), NEE and cosine-only, the leak-end rule and the reference's leaks (*_ref), and
the level caps `const` and `generic`. The HEAD scene's NEE and cosine images are also the committed
tests/golden/counter_64x48_s16_{nee,cos}.npy. In the leak-end kernels misses > 0: a miss there reads
table entry 63 (about 0.047 misses per sample: some 2 300 of 49 152).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
W, H, SPP = 64, 48, 16
LEAKS = 4  # SPT_FLAG_REFERENCE_LEAKS
TILTED = dict(lookfrom=(40, 55, 160), lookat=(55, 35, 10), vup=(0.1, 1, 0))
STATS = ("path_rays", "vertices", "shadow_traced", "misses", "nee_light_hits")  # (+ shadow_proven, below)
# the early-resolve kernels whose claims the oracle can check (oracle.proof_check): its proof mode
PROOF = {"const_nee": "literal", "const_nee_cam": "literal", "upbox_nee": "edited", "upbox_nee_cam": "edited"}
EARLY = {"const_nee", "const_nee_ref", "const_nee_cam", "upbox_nee", "upbox_nee_cam", "uplight_nee", "uplight_nee_cam"}

# variant -> (scene, tilted camera, nee_prob, flags, level)
CASES = {
    "const_nee": ("head", False, 1.0, 0, "auto"),
    "const_cos": ("head", False, 0.0, 0, "auto"),
    "const_nee_ref": ("head", False, 1.0, LEAKS, "auto"),
    "const_cos_ref": ("head", False, 0.0, LEAKS, "auto"),
    "const_nee_cam": ("head", True, 1.0, 0, "auto"),
    "const_cos_cam": ("head", True, 0.0, 0, "auto"),
    "const": ("head", False, 1.0, 0, "const"),
    "upbox_nee": ("movebox", False, 1.0, 0, "auto"),
    "upbox_cos": ("movebox", False, 0.0, 0, "auto"),
    "upbox_nee_cam": ("movebox", True, 1.0, 0, "auto"),
    "upbox_cos_cam": ("movebox", True, 0.0, 0, "auto"),
    "uplight_nee": ("light", False, 1.0, 0, "auto"),
    "uplight_cos": ("light", False, 0.0, 0, "auto"),
    "uplight_nee_cam": ("light", True, 1.0, 0, "auto"),
    "uplight_cos_cam": ("light", True, 0.0, 0, "auto"),
    "generic": ("head", False, 1.0, 0, "generic"),
}
LEAK_END = {k for k in CASES if k not in ("const_nee_ref", "const_cos_ref")}


def scene(spt, name):
    head = spt.cornell_scene()
    if name == "movebox":
        return spt.move_short_box(head, 1.0)
    if name == "light":
        return spt.edit_light(head, y=81.4)
    return head


_truth = {}


def truth(spt, oracle, sc, tilted, nee, flags, proof=None):
    """The oracle's render of a case, once per (scene, camera, estimator, leaks): the kernel-level cap
    is no part of the contract. With a proof mode also the shadow rays the early resolve claims."""
    key = (sc, tilted, nee, flags, proof)
    if key not in _truth:
        p = spt.default_params(width=W, height=H, spp=SPP, seed=1, nee_prob=nee, flags=flags)
        cam = spt.Camera(aspect=W / H, **(TILTED if tilted else {}))
        claims = None
        if proof:
            oracle.proof_check(True, edited=proof == "edited")
        try:
            img, st = oracle.counter_render(scene(spt, sc), cam._c, p)
            if proof:
                claims, wrong = oracle.proof_counts()
                assert wrong == 0
        finally:
            oracle.proof_check(False)
        img.setflags(write=False)
        _truth[key] = (img, st, claims)
    return _truth[key]


@pytest.mark.parametrize("variant", list(CASES))
def test_variant_bit_exact(spt, oracle, variant):
    sc, tilted, nee, flags, level = CASES[variant]
    p = spt.default_params(width=W, height=H, spp=SPP, seed=1, nee_prob=nee,
                           flags=flags | spt.kernel_flag(level))
    cam = spt.Camera(aspect=W / H, **(TILTED if tilted else {}))
    gpu, st = spt.render(scene(spt, sc), cam, p, return_stats=True)
    assert st["kernel"] == variant
    cpu, cst, claims = truth(spt, oracle, sc, tilted, nee, flags, PROOF.get(variant))
    assert gpu.shape == cpu.shape == (H, W, 3)
    diff = np.argwhere(gpu != cpu)
    assert diff.size == 0, f"{len(diff)} values differ, first {diff[:4].tolist()}"
    for k in STATS:
        assert st[k] == cst[k], (k, st[k], cst[k])
    assert {k: st[k] for k in spt.STAT_KEYS} == cst
    assert st["samples"] == W * H * SPP
    if claims is not None:
        assert st["shadow_proven"] == claims
    assert (st["shadow_proven"] > 0) == (variant in EARLY)
    if variant in LEAK_END:
        assert st["misses"] > 0
    if sc == "head" and not tilted and not flags:
        gold = np.load(os.path.join(GOLDEN, f"counter_64x48_s16_{'nee' if nee else 'cos'}.npy"))
        assert np.array_equal(gpu, gold)

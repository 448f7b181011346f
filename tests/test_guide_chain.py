"""The specular chain of the guide (include/spt.h SPT_HAS_GUIDE_CHAIN) on the CPU: the truth helper
tests/guide_chain_truth.py against the first-hit truth where the two must agree, the properties the
header promises for a scene with a mirror and a glass ball, and the statement's presence in the header,
the mirror and the library (spt_guide_create_ex refuses unknown flags before it looks for a device).
"""
import ctypes
import os
import re

import numpy as np
import pytest

import guide_chain_truth as gct
import guide_truth as gt

SEED = 5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(spt, w, h, spp, **kw):
    return spt.default_params(width=w, height=h, spp=spp, seed=SEED, **kw)


def _aspect(w, h):
    return float(np.float32(w) / np.float32(h))


@pytest.mark.parametrize("name,w,h,spp", [("head", 32, 24, 4), ("spheres32", 32, 24, 4)])
def test_without_specular_primitives_the_chain_is_the_first_hit(spt, oracle, name, w, h, spp):
    prims = gct.scene(spt, name)
    assert all(p.refl == gct.DIFF for p in prims)
    cam = spt.Camera(aspect=_aspect(w, h))
    p = _params(spt, w, h, spp)
    want = gt.guide_truth(oracle, prims, cam._c, p)
    got, segs = gct.chain_truth(oracle, prims, cam._c, p, return_segments=True)
    assert want[..., 7].sum() > 0 and np.array_equal(got, want)
    assert segs.max() == 1


@pytest.fixture(scope="module")
def mirror_glass_rays(spt, oracle):
    """Per ray (not per pixel) of mirror_glass 32x24 @ 4: first-hit records, chain records, the chain's
    segment counts, the first hit's primitive."""
    prims = gct.scene(spt, "mirror_glass")
    w, h, spp = 32, 24, 4
    p = _params(spt, w, h, spp, nee_prob=0.0)
    cam = spt.Camera(aspect=_aspect(w, h))
    unit = gt.unit_dirs(prims)
    assert unit
    o, d = gt.camera_rays(oracle, cam._c, p, np.arange(h), 0, spp, unit)
    d = d.reshape(-1, 3)
    first = gt.ray_records(oracle, prims, p, o, d)
    chain, segs = gct.chain_records(oracle, prims, p, o, d, unit)
    _, ids = oracle.intersect_batch(prims, p, np.broadcast_to(o, d.shape), d)
    return prims, p, first, chain, segs, ids


def test_mirror_glass_hits_and_diffuse_first_hits(mirror_glass_rays):
    prims, p, first, chain, segs, ids = mirror_glass_rays
    refl = np.array([q.refl for q in prims])
    assert (chain[:, 7] <= first[:, 7]).all()
    diff = (ids >= 0) & (refl[np.maximum(ids, 0)] == gct.DIFF)
    assert diff.any() and np.array_equal(chain[diff], first[diff])
    assert (segs[diff] == 1).all()
    spec = (ids >= 0) & (refl[np.maximum(ids, 0)] != gct.DIFF)
    assert spec.any() and (segs[spec] >= 2).all()
    assert 1 <= segs.min() and segs.max() <= gct.MAX_CHAIN
    # the pixel sums are the rays' sums
    w, h, spp = p.width, p.height, p.spp
    assert (chain.reshape(h, w, spp, 8).sum(axis=2)[..., 7] <= first.reshape(h, w, spp, 8).sum(axis=2)[..., 7]).all()


def test_mirror_glass_albedo_through_the_mirror(oracle, mirror_glass_rays):
    """Where the first hit is SPEC the albedo is fix(.999^k * c), c a diffuse primitive's colour (a
    wall or the light) after k specular hits, or fix(.999^8) where the chain ran out on a ball."""
    prims, p, first, chain, segs, ids = mirror_glass_rays
    F = np.float32
    refl = np.array([q.refl for q in prims])
    inv_spp = F(1.0) / F(p.spp)
    cols = sorted({tuple(np.array(list(q.c), dtype=np.float64).astype(F)) for q in prims if q.refl == gct.DIFF})
    allowed = set()
    a = F(1.0)
    for k in range(1, gct.MAX_CHAIN + 1):
        a = F(a * F(0.999))
        cands = [tuple(F(a * F(c)) for c in col) for col in cols] if k < gct.MAX_CHAIN else []
        if k == gct.MAX_CHAIN:
            cands = [(a, a, a)]
        for cand in cands:
            allowed.add(tuple(int(v) for v in oracle.fix_batch(np.array(cand, dtype=F), inv_spp)))
    spec = (ids >= 0) & (refl[np.maximum(ids, 0)] == gct.SPEC) & (chain[:, 7] == 1)
    assert spec.sum() > 20
    seen = {tuple(int(v) for v in r[:3]) for r in chain[spec]}
    assert seen <= allowed, sorted(seen - allowed)[:4]
    assert len(seen) >= 3  # more than one wall is seen in the mirror
    # ... and none of them is the mirror's own .999, which is what the first-hit guide holds there
    own = tuple(int(v) for v in oracle.fix_batch(np.full(3, 0.999, dtype=F), inv_spp))
    assert all(tuple(r[:3]) == own for r in first[spec]) and own not in seen


def test_hall_of_mirrors_runs_into_the_cap(spt, oracle):
    prims = gct.scene(spt, "hall")
    assert not gt.unit_dirs(prims)
    w, h, spp = 32, 24, 4
    p = _params(spt, w, h, spp)
    cam = spt.Camera(aspect=_aspect(w, h), **gct.HALL_CAM)
    rec, segs = gct.chain_truth(oracle, prims, cam._c, p, return_segments=True)
    assert segs.max() == gct.MAX_CHAIN and segs.min() < gct.MAX_CHAIN
    assert len(np.unique(segs)) >= 4  # chains of many lengths
    capped = (segs == gct.MAX_CHAIN) & (rec[..., 7] == spp)
    assert capped.any()  # an exhausted chain records its last mirror as if it were diffuse
    first = gt.guide_truth(oracle, prims, cam._c, p)
    assert (rec[..., 7] <= first[..., 7]).all() and not np.array_equal(rec, first)


def test_the_header_announces_the_chain(spt):
    text = open(os.path.join(ROOT, "include", "spt.h")).read()
    assert re.search(r"^#define SPT_HAS_GUIDE_CHAIN 1\b", text, re.M)
    assert re.search(r"^#define SPT_GUIDE_THROUGH_SPECULAR 1u\b", text, re.M)
    assert re.search(r"^#define SPT_GUIDE_MAX_CHAIN 8\b", text, re.M)
    assert re.search(r"^#define SPT_ABI_VERSION 6\b", text, re.M)
    assert spt.load_library().spt_abi_version() == 6
    assert (spt.SPT_HAS_GUIDE_CHAIN, spt.GUIDE_THROUGH_SPECULAR, spt.GUIDE_MAX_CHAIN) == (1, 1, 8)
    assert gct.MAX_CHAIN == spt.GUIDE_MAX_CHAIN
    assert "spt_guide_create_ex" in spt.EXPORTS
    assert ctypes.sizeof(spt.spt_guide_info) == spt.load_library().spt_guide_info_size() == 32
    assert spt.spt_guide_info.flags.offset == 28


def test_create_ex_refuses_unknown_flags_before_it_looks_for_a_device(spt):
    lib = spt.load_library()
    p = _params(spt, 8, 4, 4)
    for flags in (2, 3, 0x80000000, 0xFFFFFFFE):
        out = ctypes.c_void_p(0x1234)
        assert lib.spt_guide_create_ex(0, ctypes.byref(p), flags, ctypes.byref(out)) == 1, flags
        assert out.value == 0x1234
        assert b"flags" in lib.spt_last_error()
    assert lib.spt_guide_create_ex(0, ctypes.byref(p), 1, None) == 1  # a null out
    assert lib.spt_guide_create_ex(0, None, 1, ctypes.byref(ctypes.c_void_p())) == 1


@pytest.mark.parametrize("name", ["one_mirror_ball", "one_mirror_wall"])
def test_truth_albedo_through_one_mirror_is_the_oracles_render(spt, oracle, name):
    """With one specular primitive, every DIFF primitive emitting its colour and reflecting nothing,
    nee_prob = 0 and no roulette, the oracle's render (c_path: its own SPEC step) is the chain guide's
    resolved albedo, bit for bit: the helper's reflected segment is the contract's ray."""
    prims = gct.scene(spt, name)
    w, h, spp = 48, 32, 4
    cam = spt.Camera(aspect=_aspect(w, h))
    p = _params(spt, w, h, spp, nee_prob=0.0, rr_depth=64)
    img, st = oracle.counter_render(gct.albedo_render_scene(spt, prims), cam._c, p)
    rec, segs = gct.chain_truth(oracle, prims, cam._c, p, return_segments=True)
    assert st["misses"] == 0 and (rec[..., 7] == spp).all() and segs.max() == 2
    assert st["vertices"] > st["samples"]
    alb = gt.resolve_numpy(rec, spp, spp)["albedo"]
    assert np.array_equal(img.view(np.uint32), alb.view(np.uint32))
    assert not np.array_equal(rec, gt.guide_truth(oracle, prims, cam._c, p))

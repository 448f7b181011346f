"""The guide planes (include/spt.h SPT_HAS_GUIDE) on the CPU: the truth helper (tests/guide_truth.py)
against the oracle's own renders, the library's host resolve against a numpy statement of the header's
rule, and the mirror's presence. No GPU.

The truth is the oracle's: with every primitive emitting its colour, max_depth = 1 and nee_prob = 0,
oracle.counter_render is the mean first-hit albedo (where no camera ray misses), and that image must
equal the truth's resolved albedo bit for bit.
"""
import ctypes

import numpy as np
import pytest

import guide_truth as gt
import ray_truth as rt

W, H, SPP, SEED = 64, 48, 8, 5
MAX_LEFT_OUT = 0.02  # of the pixels, where a scene has misses


def _params(spt, w=W, h=H, spp=SPP, **kw):
    return spt.default_params(width=w, height=h, spp=spp, seed=SEED, **kw)


def _aspect(w, h):
    return float(np.float32(w) / np.float32(h))


VIEWS = [("head_ref", "head", {}), ("head_tilted", "head", rt.TILTED), ("spheres32", "spheres32", {})]


@pytest.mark.parametrize("label,name,camkw", VIEWS, ids=[v[0] for v in VIEWS])
def test_truth_albedo_is_the_oracles_render(spt, oracle, label, name, camkw):
    prims = rt.scene(spt, name)
    cam = spt.Camera(aspect=_aspect(W, H), **camkw)
    p = _params(spt, max_depth=1, nee_prob=0.0)
    img, st = oracle.counter_render(gt.albedo_scene(spt, prims), cam._c, p)
    rec = gt.guide_truth(oracle, prims, cam._c, p)
    alb = gt.resolve_numpy(rec, SPP, SPP)["albedo"]
    full = rec[..., 7] == SPP
    if st["misses"] == 0:
        assert full.all()
    assert (~full).sum() == 0 or st["misses"] > 0
    assert (~full).mean() <= MAX_LEFT_OUT, (label, st["misses"], (~full).sum())
    assert int((SPP - rec[..., 7]).sum()) == st["misses"]
    diff = np.argwhere(img.view(np.uint32)[full] != alb.view(np.uint32)[full])
    assert diff.size == 0, (label, len(diff))
    if label == "head_ref":
        assert st["misses"] == 0


def _edge_records(spp):
    """Records that hit every branch of the resolve: hits 0, 0 < hits < n, negative normal sums, an
    albedo sum at the clamp 2^31 * spp exactly and above it, the largest depth."""
    one = 1 << 31
    return np.array([
        [0, 0, 0, 0, 0, 0, 0, 0],
        [one * spp, one * spp // 2, 12345, -one * spp, one * 3, -7, (1 << 36) * spp, spp],
        [one * spp + 1, one * (spp + 3), 1, one * spp, -(one * spp - 1), 0, 65536 * 3 + 1, 3],
        [one, 3 * one, (one * spp) - 1, -1, 1, -(one // 3), 1, 1],
        [0, 0, 0, 0, 0, 0, 0, 0],
        [one * 2, one * 2, one * 2, -one, -one, -one, 123456789012, 2],
    ], dtype=np.int64)


@pytest.mark.parametrize("spp,done", [(8, 8), (8, 3), (8, 1), (96, 5), (1 << 24, 1 << 24), (7, 0)])
def test_resolve_host_is_the_headers_rule(spt, spp, done):
    rec = _edge_records(spp).reshape(2, 3, 8)
    got = spt.guide_resolve_host(rec, 3, 2, spp, done)
    want = gt.resolve_numpy(rec, spp, done)
    for k in spt.GUIDE_PLANES:
        assert got[k].shape == want[k].shape
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (k, got[k], want[k])
    if done == spp:
        assert got["albedo"][0, 1, 0] == 1.0 and got["albedo"][0, 2, 0] == 1.0  # the clamp, at and above
        assert got["albedo"][1, 0, 0] == 1.0 and got["albedo"][1, 0, 1] == 1.0  # 2^31 exactly; 3 * 2^31
        # the normal is not clamped: a sum of 2^31 * spp reads spp, one of -2^31 reads -1
        assert got["normal"][0, 1, 0] == -float(spp) and got["normal"][1, 2, 0] == -1.0
    if done:
        assert got["coverage"][0, 0] == 0.0 and got["depth"][0, 0] == 0.0
    else:
        assert all(not got[k].any() for k in spt.GUIDE_PLANES)


def test_resolve_host_rejects_and_accepts_an_empty_guide(spt):
    lib = spt.load_library()
    info = spt.spt_guide_info(0, 0, 4, 2, 0, 0)
    assert lib.spt_guide_resolve_host(None, ctypes.byref(info), None, None, None, None) == 0
    bad = spt.spt_guide_info(2, 2, 4, 5, 0, 0)  # samples_done > spp_total
    rec = np.zeros(32, dtype=np.int64)
    assert lib.spt_guide_resolve_host(rec.ctypes.data, ctypes.byref(bad), None, None, None, None) == 1
    with pytest.raises(spt.SptError):
        spt.guide_resolve_host(np.zeros(7, dtype=np.int64), 1, 1, 4, 4)


def test_presence_and_struct_size(spt):
    assert spt.SPT_HAS_GUIDE == 1
    lib = spt.load_library()
    assert ctypes.sizeof(spt.spt_guide_info) == lib.spt_guide_info_size() == 32
    assert spt.spt_guide_info.lanes_per_pixel.offset == 24
    for name in ("Guide", "render_guides", "guide_resolve_host"):
        assert hasattr(spt, name)
    assert {"spt_guide_create", "spt_guide_render_async", "spt_guide_resolve_host"} <= set(spt.EXPORTS)

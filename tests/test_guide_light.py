"""The light guide (include/spt.h SPT_HAS_GUIDE_LIGHT) on the CPU: the two host statements against
numpy statements of the header's rule (tests/guide_light_truth.py), what creation refuses before it looks
for a device, the truth helper's own properties on the scenes the GPU tests use, and the statement's
presence in the header, the mirror and the library.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import guide_chain_truth as gct
import guide_light_truth as glt

SEED = 5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ONE = 1 << 31


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _records(rng, rows, w, spp):
    """Hand-made records: the edges first, then random ones that a pass could have written."""
    rec = np.zeros((rows, w, 4), dtype=np.int64)
    tested = rng.integers(0, spp + 1, size=(rows, w))
    lit = (tested * rng.random((rows, w))).astype(np.int64)
    rec[..., 0], rec[..., 1] = tested, lit
    rec[..., 2] = (lit * rng.random((rows, w)) * ONE).astype(np.int64)
    rec[0, 0] = (0, 0, 0, 0)                # never tested
    rec[0, 1] = (spp, spp, ONE * spp, 0)    # every sample at the per-sample clamp: direct = spp
    rec[0, 2] = (spp, 0, 0, 0)              # tested, never lit
    rec[0, 3] = (3, 1, (1 << 29) + 1, 0)    # a sum that the float conversion rounds
    rec[0, 4] = (7, 2, 3, 0)
    return rec


@pytest.mark.parametrize("spp,done", [(8, 8), (8, 3), (96, 5), (1 << 24, 1 << 24), (8, 0)])
def test_resolve_host_is_the_headers_rule(spt, spp, done):
    rows, w = 5, 7
    rec = _records(np.random.default_rng(spp + done), rows, w, min(spp, 1000))
    got = spt.light_guide_resolve_host(rec, w, rows, spp, done)
    want = glt.resolve_numpy(rec, spp, done)
    assert set(got) == {"visibility", "direct", "tested"}
    for k in want:
        assert got[k].shape == (rows, w) and got[k].dtype == F
        assert np.array_equal(_bits(got[k]), _bits(want[k])), k
    if done == 0:
        assert all((got[k] == 0).all() for k in got)
    elif done == spp == 8:
        assert got["visibility"][0, 0] == 0 and got["tested"][0, 0] == 0  # tested == 0
        assert got["direct"][0, 1] == 8.0 and got["visibility"][0, 1] == 1.0  # not clamped
        assert got["visibility"][0, 2] == 0 and got["tested"][0, 2] == 1.0
        assert got["visibility"][0, 4] == F(2.0 / 7.0)


def test_resolve_host_refuses_bad_arguments(spt):
    rec = np.zeros((2, 3, 4), dtype=np.int64)
    with pytest.raises(spt.SptError):
        spt.light_guide_resolve_host(rec, 3, 2, 8, 9)  # more samples than spp
    with pytest.raises(spt.SptError):
        spt.light_guide_resolve_host(rec, 3, 2, 0, 0)
    with pytest.raises(spt.SptError):
        spt.light_guide_resolve_host(rec[:1], 3, 2, 8, 8)  # too few records
    assert spt.light_guide_resolve_host(np.zeros((0, 3, 4), np.int64), 3, 0, 8, 4)["direct"].shape == (0, 3)


@pytest.mark.parametrize("floor", [0.1, 0.25, 0.5, 1.0, float(np.finfo(F).tiny)])
def test_shade_host_is_a_multiply_an_add_and_a_product(spt, floor):
    rng = np.random.default_rng(11)
    h, w = 9, 13
    alb = rng.random((h, w, 3)).astype(F)
    vis = rng.random((h, w)).astype(F)
    vis[0, :4] = (0.0, 1.0, 0.375, F(2.0 / 7.0))
    want = glt.shade_numpy(alb, vis, floor)
    got = spt.light_shade_host(alb, vis, floor)
    assert got.shape == alb.shape and np.array_equal(_bits(got), _bits(want))
    if floor == 1.0:
        assert np.array_equal(_bits(got), _bits(alb))
    assert np.array_equal(_bits(got[0, 1]), _bits(alb[0, 1]))  # floor + (1 - floor) * 1 is exactly 1
    io = alb.copy()  # in place
    assert spt.light_shade_host(io, vis, floor, out=io) is io
    assert np.array_equal(_bits(io), _bits(want))


def test_shade_host_is_not_contracted(spt):
    """A floor and a visibility whose fused multiply-add differs from the multiply then the add."""
    import guide_truth as gt
    rng = np.random.default_rng(3)
    vis = rng.random(4096).astype(F)
    floor = F(0.3)
    fused = gt.fmaf(F(1.0) - floor, vis, floor)
    m = (floor + ((F(1.0) - floor) * vis).astype(F)).astype(F)
    assert (fused != m).any()
    alb = np.ones((4096, 3), dtype=F)
    got = spt.light_shade_host(alb, vis, float(floor))
    assert np.array_equal(_bits(got[:, 0]), _bits(m))


@pytest.mark.parametrize("floor", [0.0, -0.0, -0.25, 1.0000001, 2.0, float("inf"), float("-inf"), float("nan")])
def test_shade_host_refuses_a_floor_outside_its_range(spt, floor):
    alb, vis = np.full((4, 3), 0.5, dtype=F), np.full(4, 0.5, dtype=F)
    out = np.full((4, 3), -7.0, dtype=F)
    with pytest.raises(spt.SptError):
        spt.light_shade_host(alb, vis, floor, out=out)
    assert (out == -7.0).all()
    assert b"shade_floor" in spt.load_library().spt_last_error()


def test_create_refuses_unknown_flags_before_it_looks_for_a_device(spt):
    lib = spt.load_library()
    p = spt.default_params(width=8, height=4, spp=4, seed=SEED)
    for flags in (2, 3, 0x80000000, 0xFFFFFFFE):
        out = ctypes.c_void_p(0x1234)
        assert lib.spt_light_guide_create(0, ctypes.byref(p), flags, ctypes.byref(out)) == 1, flags
        assert out.value == 0x1234
        assert b"flags" in lib.spt_last_error()
    assert lib.spt_light_guide_create(0, ctypes.byref(p), 1, None) == 1  # a null out
    assert lib.spt_light_guide_create(0, None, 1, ctypes.byref(ctypes.c_void_p())) == 1


def test_create_refuses_more_than_2_to_24_samples_and_bad_shapes(spt):
    lib = spt.load_library()
    for kw, text in (({"spp": (1 << 24) + 1}, b"2^24"), ({"width": 0}, b"positive"), ({"spp": 0}, b"positive"),
                     ({"shard_index": 2, "shard_count": 2}, b"shard")):
        q = spt.default_params(**{**dict(width=8, height=4, spp=4, seed=SEED), **kw})
        out = ctypes.c_void_p(0x1234)
        for flags in (0, 1):
            assert lib.spt_light_guide_create(0, ctypes.byref(q), flags, ctypes.byref(out)) == 1, kw
            assert out.value == 0x1234 and text in lib.spt_last_error(), (kw, lib.spt_last_error())


def test_guide_create_ex_still_refuses_the_other_flags(spt):
    """A light guide is its own object: spt_guide_create_ex takes no new flag."""
    lib = spt.load_library()
    p = spt.default_params(width=8, height=4, spp=4, seed=SEED)
    for flags in (2, 3):
        out = ctypes.c_void_p(0x1234)
        assert lib.spt_guide_create_ex(0, ctypes.byref(p), flags, ctypes.byref(out)) == 1
        assert out.value == 0x1234


def test_null_objects_are_refused(spt):
    lib = spt.load_library()
    info = spt.spt_guide_info()
    assert lib.spt_light_guide_info_get(None, ctypes.byref(info)) == 1
    assert lib.spt_light_guide_clear(None, None) == 1
    assert lib.spt_light_guide_resolve(None, None, None, None, None) == 1
    assert lib.spt_light_guide_download(None, None, None) == 1
    assert lib.spt_light_guide_destroy(None) == 0
    p = spt.default_params(width=8, height=4, spp=4, seed=SEED)
    assert lib.spt_light_guide_render_async(None, None, None, 0, None, ctypes.byref(p), 0, 4, None) == 1


def test_the_header_announces_the_light_guide(spt):
    text = open(os.path.join(ROOT, "include", "spt.h")).read()
    assert re.search(r"^#define SPT_HAS_GUIDE_LIGHT 1\b", text, re.M)
    assert re.search(r"^#define SPT_ABI_VERSION 6\b", text, re.M)
    assert spt.load_library().spt_abi_version() == 6
    assert (spt.SPT_HAS_GUIDE_LIGHT, spt.LIGHT_GUIDE_SLOTS) == (1, 4)
    for name in ("spt_light_guide_create", "spt_light_guide_render_async", "spt_light_guide_resolve_host",
                 "spt_light_shade_async", "spt_light_shade_host"):
        assert name in spt.EXPORTS and hasattr(spt.load_library(), name)
    for rel in ("csrc/spt_guide_light.hip", "csrc/spt_guide_light_host.cpp", "csrc/spt_guide_light.h",
                "csrc/spt_guide_device.h"):
        assert rel in spt.KERNEL_SOURCES  # a change to them makes the build identity stale
    mk = open(os.path.join(ROOT, "small-pathtracer_amd", "csrc", "Makefile")).read()
    hashed = mk[mk.index("HASHED"):mk.index("SRC_SHA16")]
    for name in ("spt_guide_light.hip", "spt_guide_light_host.cpp", "spt_guide_light.h", "spt_guide_device.h"):
        assert name in hashed
    assert spt.build_sources_sha16() == spt.kernel_sources_sha16()


# ---- the truth helper itself -----------------------------------------------------------------------
def test_truth_on_head_is_the_count_the_contract_was_written_with(spt, oracle):
    prims = gct.scene(spt, "head")
    for (w, h, spp), want in (((31, 24, 8), (5738, 3990)), ((8, 4, 96), (3046, 2413))):
        p = spt.default_params(width=w, height=h, spp=spp, seed=SEED)
        cam = spt.Camera(aspect=float(F(w) / F(h)))
        rec, det = glt.light_truth(oracle, prims, cam._c, p, return_detail=True)
        assert (int(rec[..., 0].sum()), int(rec[..., 1].sum())) == want
        assert (rec[..., 3] == 0).all() and (rec[..., 1] <= rec[..., 0]).all() and (rec[..., 0] <= spp).all()
        assert np.isfinite(det["weight"]).all() and 0 < det["weight"].max() < 0.14
        assert not (det["vertex"][det["tested"]] == p.light_id).any()
        # the chain kind of a scene without specular primitives holds the same bits
        assert np.array_equal(glt.light_truth(oracle, prims, cam._c, p, chain=True), rec)


def test_truth_windows_and_rows_add_up(spt, oracle):
    prims = gct.scene(spt, "specular")
    w, h, spp = 12, 8, 6
    p = spt.default_params(width=w, height=h, spp=spp, seed=SEED)
    cam = spt.Camera(aspect=float(F(w) / F(h)))
    for chain in (False, True):
        whole = glt.light_truth(oracle, prims, cam._c, p, chain=chain)
        parts = glt.light_truth(oracle, prims, cam._c, p, chain, 0, 2) + glt.light_truth(oracle, prims, cam._c, p, chain, 2, 4)
        assert np.array_equal(whole, parts)
        assert np.array_equal(glt.light_truth(oracle, prims, cam._c, p, chain, rows=[5, 2]), whole[[5, 2]])


def test_truth_first_hit_mirror_is_not_tested_and_the_chain_sees_through_it(spt, oracle):
    prims = gct.scene(spt, "one_mirror_wall")
    w, h, spp = 16, 12, 8
    p = spt.default_params(width=w, height=h, spp=spp, seed=SEED)
    cam = spt.Camera(aspect=float(F(w) / F(h)))
    first, d1 = glt.light_truth(oracle, prims, cam._c, p, chain=False, return_detail=True)
    chain, d2 = glt.light_truth(oracle, prims, cam._c, p, chain=True, return_detail=True)
    mirror = d1["vertex"] == 0
    assert mirror.any() and not d1["tested"][mirror].any()
    assert d2["tested"][mirror].any() and (d2["segments"][mirror] == 2).all()
    assert np.array_equal(d1["tested"][~mirror], d2["tested"][~mirror])
    assert chain[..., 0].sum() > first[..., 0].sum()

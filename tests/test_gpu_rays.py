"""The edge rays of tests/test_contract_rays.py (families F2-F6: exactly zero direction components,
origins on planes, grazes of edges, corners, rims and tangents, roots at the sphere epsilon) through
every render-kernel family on the GPU, bit for bit against the oracle.

A camera is four raw vectors, so ray_camera() aims single rays (horizontal = vertical = 0: every
pixel and sample traces origin, llc - origin) and narrow fans exactly where a trace can go wrong.
Each case names the variant it was written for: a dispatch change cannot quietly empty the coverage.
A zero direction component makes rcp_nr a NaN whose bits no rule fixes (measured: 0xFFC00000 on the
host and on gfx950 alike); the slabs compare keys as signed integers, and whatever the NaN it must
end in 'no hit' on both sides.
"""
import numpy as np
import pytest

import ray_truth as rt

pytestmark = pytest.mark.gpu
LEAKS = 4  # SPT_FLAG_REFERENCE_LEAKS
NEE, COS = dict(nee_prob=1.0), dict(nee_prob=0.0)
SPH = dict(max_depth=12)

# (scene, camera class, params, level, the variant the case is written for)
CASES = [
    ("head", "axis", NEE, "auto", "const_nee"),
    ("head", "axis", COS, "auto", "const_cos"),
    ("head", "axis", dict(flags=LEAKS, **NEE), "auto", "const_nee_ref"),
    ("head", "axis", dict(flags=LEAKS, **COS), "auto", "const_cos_ref"),
    ("head", "raw", NEE, "auto", "const_nee_cam"),
    ("head", "raw", COS, "auto", "const_cos_cam"),
    ("head", "raw", dict(flags=LEAKS, **NEE), "auto", "const"),
    ("head", "axis", NEE, "const", "const"),
    ("head", "raw", NEE, "cornell", "cornell"),
    ("head", "axis", dict(flags=LEAKS, **NEE), "cornell", "cornell"),
    ("head", "raw", NEE, "generic", "generic"),
    ("head", "axis", dict(flags=LEAKS, **COS), "generic", "generic"),
    ("movebox", "axis", NEE, "auto", "upbox_nee"),
    ("movebox", "raw", NEE, "auto", "upbox_nee_cam"),
    ("movebox", "raw", dict(flags=LEAKS, **NEE), "auto", "cornell"),
    ("editlight", "axis", NEE, "auto", "uplight_nee"),
    ("editlight", "raw", NEE, "auto", "uplight_nee_cam"),
    ("editroom", "axis", NEE, "auto", "cornell_nee"),
    ("editroom", "axis", COS, "auto", "cornell_cos"),
    ("editroom", "raw", NEE, "auto", "cornell"),
    ("negzero2", "axis", NEE, "auto", "cornell_nee"),
    ("negzero2", "raw", NEE, "auto", "cornell"),
    ("dropbox", "axis", NEE, "auto", "rectdiff_nee"),
    ("dropbox", "raw", NEE, "auto", "rectdiff"),
    ("dropbox", "axis", dict(flags=LEAKS, **NEE), "auto", "rectdiff"),
    ("spheres32", "axis", dict(**SPH, **NEE), "auto", "sphdiff_nee"),
    ("spheres32", "raw", dict(**SPH, **NEE), "auto", "sphdiff_nee"),
    ("spheres32", "raw", dict(flags=LEAKS, **SPH, **NEE), "auto", "sphdiff_nee_ref"),
    ("spheres32", "raw", dict(**SPH, **COS), "auto", "sphdiff"),
    ("three_spheres", "raw", dict(**SPH, **NEE), "auto", "sphdiff_nee"),
    ("three_spheres", "axis", dict(**SPH, **COS), "auto", "sphdiff"),
    ("three_spheres", "raw", dict(**SPH, **NEE), "generic", "generic"),
    ("classic", "raw", COS, "auto", "wide"),
    ("classic", "axis", dict(flags=LEAKS, **COS), "auto", "wide"),
]
REQUIRED = {"const_nee", "const_cos", "const_nee_cam", "const_cos_cam", "const_nee_ref", "const",
            "cornell", "generic", "upbox_nee", "upbox_nee_cam", "uplight_nee", "uplight_nee_cam",
            "cornell_nee", "rectdiff_nee", "rectdiff", "sphdiff_nee", "sphdiff", "wide"}


def ray_camera(spt, origin, L, hor=(0, 0, 0), ver=(0, 0, 0)):
    """A camera from raw vectors: origin, lower_left_corner = origin + L, horizontal, vertical."""
    cam = spt.Camera()
    for i in range(3):
        cam._c.origin[i] = float(origin[i])
        cam._c.lower_left_corner[i] = float(origin[i]) + float(L[i])
        cam._c.horizontal[i] = float(hor[i])
        cam._c.vertical[i] = float(ver[i])
    return cam


def case_params(spt, kw, level, w, h, spp=8, seed=5):
    kw = dict(kw)
    flags = kw.pop("flags", 0) | spt.kernel_flag(level)
    return spt.default_params(width=w, height=h, spp=spp, seed=seed, flags=flags, **kw)


def _case_id(c):
    return "-".join([c[0], c[1]] + [f"{k}={v}" for k, v in c[2].items()] + [c[3], c[4]])


def test_cases_cover_the_required_variants():
    assert REQUIRED <= {c[4] for c in CASES}


def _compare(spt, oracle, prims, cam, p, want, label):
    gpu, gst = spt.render(prims, cam, p, return_stats=True)
    assert gst["kernel"] == want, (label, gst["kernel"], want)
    cpu, cst = oracle.counter_render(prims, cam._c, p)
    diff = np.argwhere(gpu != cpu)
    assert diff.size == 0, f"{label}: {len(diff)} values differ, first {diff[:4].tolist()}"
    assert {k: gst[k] for k in spt.STAT_KEYS} == cst, label
    return cst


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_edge_rays_bit_exact(spt, oracle, case):
    name, cls, kw, level, want = case
    prims = rt.scene(spt, name)
    views = rt.views(spt, oracle, name, cls)
    assert len(views) >= 5
    first_misses = 0
    for label, o, L, hor, ver, w, h in views:
        cam = ray_camera(spt, o, L, hor, ver)
        p = case_params(spt, kw, level, w, h)
        cst = _compare(spt, oracle, prims, cam, p, want, label)
        if label.startswith("F2_o0") and prims[0].kind != rt.SPHERE:
            # mid-room, a zero component: every sample misses the closed room at its first vertex
            # (with SPT_FLAG_REFERENCE_LEAKS the path goes on from there and may miss again)
            assert cst["samples"] == w * h * 8 and cst["misses"] >= cst["samples"], (label, cst)
            first_misses += cst["samples"]
    if cls == "raw" and prims[0].kind != rt.SPHERE:
        assert first_misses == 7 * 4 * 4 * 8


AXIS_CASES = [c for c in CASES if c[1] == "axis" and c[3] == "auto" and c[0] != "classic"]


@pytest.mark.parametrize("case", AXIS_CASES, ids=_case_id)
def test_zero_component_on_the_jitter_lattice(spt, oracle, case):
    """The axis-camera kernels cannot take a degenerate camera, but the jitter lattice can hold the
    zero: w = 1, hor = (4, 0, 0), L.x = -1 gives d.x = -1 + 4 (-0.5 + j 2^-16), exactly 0 for the
    16-bit draw j = 49152, one sample in 2^16. 16 rows @ 32768 spp hold 2^19 samples; the seed is
    the first whose render has at least 8 of them (counted here from the Philox words, the low bytes
    of vertex 1's call)."""
    name, cls, kw, level, want = case
    prims = rt.scene(spt, name)
    h, spp = 16, 32768
    pix, s = np.meshgrid(np.arange(h, dtype=np.uint32), np.arange(spp, dtype=np.uint32), indexing="ij")
    for seed in range(1, 40):
        ctr = np.stack([pix.ravel(), s.ravel(), np.ones(h * spp, np.uint32),
                        np.full(h * spp, seed, np.uint32)], axis=1)
        r = oracle.map_words("philox", ctr)
        zeros = int((oracle.map_words("u16i", r[:, :2])[:, 0] == 49152).sum())
        if zeros >= 8:
            break
    assert zeros >= 8
    cam = ray_camera(spt, (50, 40, 100), (-1, -.45, -.8), (4, 0, 0), (0, .3, 0))
    p = case_params(spt, kw, level, 1, h, spp=spp, seed=seed)
    # those samples' rays are (0, y, z) with y in [-.45, -.15]: a miss at vertex 1 (F2)
    _, ids = oracle.intersect_batch(prims, p, [(50, 40, 100)] * 2, [(0, -.45, -.8), (0, -.15, -.8)])
    assert ids.tolist() == [-1, -1]
    cst = _compare(spt, oracle, prims, cam, p, want, f"lattice seed {seed}")
    assert cst["misses"] >= zeros >= 1


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("label", [v[0] for v in rt.ID_VIEWS])
def test_first_hit_id_image(spt, oracle, label, seed):
    """The id scene (every prim black, emitting its index) at 64 x 48 @ 1 spp: the GPU's image is the
    oracle's bit for bit, and every pixel whose nine-ray fp64 footprint has one id shows that id
    (tests/test_contract_rays.py checks the oracle's half of this without a GPU)."""
    prims, cam, p, want = rt.id_view(spt, label, seed)
    gpu, gst = spt.render(prims, cam, p, return_stats=True)
    assert gst["kernel"] == want
    cpu, cst = oracle.counter_render(prims, cam._c, p)
    assert np.array_equal(gpu, cpu)
    assert {k: gst[k] for k in spt.STAT_KEYS} == cst
    got = rt.decode_ids(gpu)
    want_ids = rt.footprint_ids(rt.Truth(oracle, prims), cam, rt.ID_W, rt.ID_H)
    keep = want_ids != -2
    assert np.mean(~keep) <= (0.15 if label.startswith("head") else 0.20)
    assert np.array_equal(got[keep], want_ids[keep]), np.argwhere((got != want_ids) & keep)[:5].tolist()

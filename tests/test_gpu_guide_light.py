"""The light guide on the GPU (include/spt.h SPT_HAS_GUIDE_LIGHT; light_guide_kernel<TP, CHAIN> in
spt_guide_light.hip): the downloaded int64[4] records, exact, against tests/guide_light_truth.py (the
header's rule restated from the oracle's pieces); lanes, windows and shards; rejections; the device
resolve and shade against the host statements; a context's neighbours; two geometric properties; the
denoise path and the drop-in program with a light guide.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import guide_chain_truth as gct
import guide_light_truth as glt
from test_gpu_guide import _frame, _read_pfm

pytestmark = pytest.mark.gpu
SEED = 5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "small-pathtracer_amd", "smallpt_amd")
BOXES = ("mirror_glass", "classic")  # no light rectangle in the scene: nee_prob = 0, as their renders have
F = np.float32


def _aspect(w, h):
    return float(F(w) / F(h))


def _params(spt, name, w, h, spp, **kw):
    if name in BOXES:
        kw.setdefault("nee_prob", 0.0)
    return glt.light_params(spt, name, spt.default_params(width=w, height=h, spp=spp, seed=SEED, **kw))


def _light(spt, prims, cam, p, chain=False, windows=None, renderer=None):
    """-> (records, info) of a fresh light guide filled with `windows` (default: the full one)."""
    r = renderer or spt.Renderer(p.device)
    g = spt.LightGuide(p, p.device, through_specular=chain)
    try:
        for base, count in windows or [(0, p.spp)]:
            g.render(r, prims, cam, p, base, count)
        return g.to_numpy(), g.info()
    finally:
        g.close()
        if renderer is None:
            r.close()


def _same(got, want, label):
    diff = np.argwhere(got != want)
    assert diff.size == 0, f"{label}: {len(diff)} slots differ, first {diff[:4].tolist()}: " \
                           f"{[(int(got[tuple(i)]), int(want[tuple(i)])) for i in diff[:4]]}"


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


# ---- 1. the truth, per scene class -----------------------------------------------------------------
# (label, scene, w, h, spp, the wide instantiation?, the kinds, the light edited?). Which instantiation
# a pass launches is the scene's: the wide one iff the scene has a wide sphere.
TRUTH_CASES = [("head", "head", 31, 24, 8, False, (False,), False),
               ("specular", "specular", 31, 24, 8, False, (False, True), False),
               ("mirror_glass", "mirror_glass", 16, 12, 8, True, (False, True), False),
               ("spheres32", "spheres32", 16, 12, 8, False, (False,), False),
               ("one_mirror_wall", "one_mirror_wall", 16, 12, 8, False, (False, True), False),
               ("head_edited_light", "head", 16, 12, 8, False, (False,), True)]


def _case(spt, name, w, h, spp, edited):
    prims = gct.scene(spt, name)
    p = _params(spt, name, w, h, spp)
    if edited:
        prims = glt.edited_light(spt, prims, p)
    return prims, spt.Camera(aspect=_aspect(w, h)), p


@pytest.mark.parametrize("label,name,w,h,spp,wide,kinds,edited", TRUTH_CASES, ids=[c[0] for c in TRUTH_CASES])
def test_records_equal_the_truth(spt, oracle, label, name, w, h, spp, wide, kinds, edited):
    prims, cam, p = _case(spt, name, w, h, spp, edited)
    assert (spt.select_kernel(prims, cam, p)["name"] == "wide") == wide
    assert any(q.refl != gct.DIFF for q in prims) == (True in kinds)
    if edited:
        assert (p.light_x0, p.light_dz, p.light_area) == (34.0, 24.0, 36.0 * 24.0)
        assert list(prims[6].geom)[:5] == [34.0, 70.0, 63.0, 87.0, 81.5]
    got = {}
    for chain in kinds:
        want, det = glt.light_truth(oracle, prims, cam._c, p, chain=chain, return_detail=True)
        tested, lit = int(want[..., 0].sum()), int(want[..., 1].sum())
        # the case's coverage, on the truth: a scene edit cannot empty it
        assert tested > 0 and 10 * lit >= tested and 10 * (tested - lit) >= tested, (label, chain, tested, lit)
        assert np.isfinite(det["weight"]).all() and (want[..., 2] > 0).any()
        if chain:
            assert det["segments"].max() >= 2
        rec, info = _light(spt, prims, cam, p, chain=chain)
        assert info["samples_done"] == spp and info["flags"] == (spt.GUIDE_THROUGH_SPECULAR if chain else 0)
        assert (info["width"], info["rows"], info["spp_total"]) == (w, h, spp)
        _same(rec, want, f"{label} chain={chain}")
        got[chain] = rec
    if len(kinds) == 2:  # ... and the two kinds differ where the scene has specular primitives
        assert not np.array_equal(got[False], got[True])
    if label == "head":
        assert (int(got[False][..., 0].sum()), int(got[False][..., 1].sum())) == (5738, 3990)


def test_every_instantiation_is_covered():
    assert {(c[5], k) for c in TRUTH_CASES for k in c[6]} == {(False, False), (False, True), (True, False), (True, True)}


# ---- 2. lanes, windows, shards ---------------------------------------------------------------------
# K = 64 at 8x4 @ 96 (the cap), 8 at its window of 5 samples, 1 or 2 at 256x192 @ 2 (the resident lanes
# of the device), as tests/test_gpu_guide.py's LANE_CASES.
LANE_CASES = [("8x4_spp96", 8, 4, 96, (0, 96)), ("8x4_window5", 8, 4, 96, (0, 5)), ("256x192_spp2", 256, 192, 2, (0, 2))]
_lanes = {}


@pytest.mark.parametrize("label,w,h,spp,window", LANE_CASES, ids=[c[0] for c in LANE_CASES])
def test_lane_groups(spt, oracle, label, w, h, spp, window):
    prims = gct.scene(spt, "specular")
    cam = spt.Camera(aspect=_aspect(w, h))
    p = _params(spt, "specular", w, h, spp)
    rec, info = _light(spt, prims, cam, p, chain=True, windows=[window])
    _lanes[label] = info["lanes_per_pixel"]
    if w * h <= 64:
        _same(rec, glt.light_truth(oracle, prims, cam._c, p, True, *window), label)
    else:  # (the truth of 98304 rays is slow in numpy) the same records whatever the lanes per pixel
        parts, _ = _light(spt, prims, cam, p, chain=True, windows=[(1, 1), (0, 1)])  # K = 1 twice
        _same(rec, parts, label)
        rows = [0, 120, 150, 191]  # two of them cross the balls
        want, det = glt.light_truth(oracle, prims, cam._c, p, True, *window, rows=rows, return_detail=True)
        assert det["segments"].max() >= 2 and 0 < want[..., 1].sum() < want[..., 0].sum()
        _same(rec[rows], want, label + " rows")


def test_lane_groups_covered_every_width():
    assert len(_lanes) == len(LANE_CASES), "runs after test_lane_groups"
    ks = set(_lanes.values())
    assert _lanes["8x4_spp96"] == 64, _lanes
    assert ks & {1, 2} and ks & {4, 8, 16, 32} and 64 in ks, _lanes


def test_windows_in_any_order_and_two_shards(spt, oracle):
    w, h, spp = 8, 4, 96
    prims = gct.scene(spt, "head")
    cam = spt.Camera(aspect=_aspect(w, h))
    p = _params(spt, "head", w, h, spp, tile_rows=2)
    one, _ = _light(spt, prims, cam, p)
    assert (int(one[..., 0].sum()), int(one[..., 1].sum())) == (3046, 2413)
    _same(one, glt.light_truth(oracle, prims, cam._c, p), "the truth")
    q8 = _params(spt, "head", w, h, 8, tile_rows=2)
    whole, _ = _light(spt, prims, cam, q8, windows=[(0, 8)])
    ab, ia = _light(spt, prims, cam, q8, windows=[(0, 3), (3, 5)])
    ba, ib = _light(spt, prims, cam, q8, windows=[(3, 5), (0, 3)])
    assert ia["samples_done"] == ib["samples_done"] == 8
    _same(ab, whole, "windows (0, 3) + (3, 5)")
    _same(ba, whole, "windows reversed")
    seen = []
    for k in range(2):
        q = _params(spt, "head", w, h, spp, tile_rows=2, shard_index=k, shard_count=2)
        rows = spt.shard_rows(q)
        rec, info = _light(spt, prims, cam, q)
        assert info["rows"] == len(rows) > 0
        _same(rec, one[rows], f"shard {k}")
        seen += list(rows)
    assert sorted(seen) == list(range(h))
    # a shard without rows only counts
    q = _params(spt, "head", w, h, spp, tile_rows=8, shard_index=1, shard_count=2)
    rec, info = _light(spt, prims, cam, q, windows=[(0, 7)])
    assert rec.shape == (0, w, 4) and info["rows"] == 0 and info["samples_done"] == 7


# ---- 3. rejections ---------------------------------------------------------------------------------
def test_rejected_calls_leave_the_light_guide_untouched(spt):
    import torch
    prims = gct.scene(spt, "head")
    cam = spt.Camera(aspect=_aspect(32, 24))
    p = _params(spt, "head", 32, 24, 8)
    r, g = spt.Renderer(0), spt.LightGuide(p, 0)
    try:
        g.render(r, prims, cam, p, 0, 5)
        before, info = g.to_numpy(), g.info()
        assert before[..., 0].sum() > 0
        bad = [(_params(spt, "head", 31, 24, 8), 5, 1), (p, 7, 2), (p, 8, 1), (p, 0, 4), (p, 5, 0),
               (_params(spt, "head", 32, 24, 9), 5, 1), (_params(spt, "head", 32, 24, 8, shard_count=2), 5, 1)]
        for q, base, count in bad:
            with pytest.raises(spt.SptError) as e:
                g.render(r, prims, cam, q, base, count)
            assert e.value.status == 1, (base, count)
            assert g.info() == info
            assert np.array_equal(g.to_numpy(), before)
        if torch.cuda.device_count() > 1:
            other = spt.Renderer(1)
            try:
                with pytest.raises(spt.SptError) as e:
                    g.render(other, prims, cam, p, 5, 1)
                assert e.value.status == 1 and np.array_equal(g.to_numpy(), before)
            finally:
                other.close()
        g.render(r, prims, cam, p, 5, 3)  # still usable
        assert g.info()["samples_done"] == 8
        g.clear()
        assert g.info()["samples_done"] == 0 and not g.to_numpy().any()
    finally:
        g.close()
        r.close()
    with pytest.raises(spt.SptError):
        spt.LightGuide(_params(spt, "head", 4, 4, (1 << 24) + 1), 0)


# ---- 4. resolve and shade --------------------------------------------------------------------------
@pytest.mark.parametrize("window", [(0, 8), (2, 3)], ids=["full", "partial"])
def test_device_resolve_equals_the_host_statement(spt, window):
    import torch
    w, h = 31, 24
    prims = gct.scene(spt, "specular")
    cam = spt.Camera(aspect=_aspect(w, h))
    p = _params(spt, "specular", w, h, 8)
    r, g = spt.Renderer(0), spt.LightGuide(p, 0)
    try:
        g.render(r, prims, cam, p, *window)
        rec = g.to_numpy()
        assert (rec[..., 0] == 0).any() and (rec[..., 1] < rec[..., 0]).any() and (rec[..., 1] > 0).any()
        host = spt.light_guide_resolve_host(rec, w, h, 8, window[1])
        want = glt.resolve_numpy(rec, 8, window[1])
        dev = g.resolve()
        for k in spt.LIGHT_GUIDE_PLANES:
            assert np.array_equal(_bits(dev[k]), _bits(host[k])), k
            assert np.array_equal(_bits(host[k]), _bits(want[k])), k
        some = g.resolve(planes=("direct",))
        assert set(some) == {"direct"} and np.array_equal(_bits(some["direct"]), _bits(host["direct"]))
        # the planes left NULL are not written: one buffer, sentinels around the two planes asked for
        n = w * h
        buf = torch.full((2 * n + 48,), -7.0, dtype=torch.float32, device="cuda:0")
        lib = spt.load_library()
        assert lib.spt_light_guide_resolve(g._g, ctypes.c_void_p(buf.data_ptr() + 4 * 16), None,
                                           ctypes.c_void_p(buf.data_ptr() + 4 * (32 + n)), None) == 0
        torch.cuda.synchronize(0)
        out = buf.cpu().numpy()
        assert np.array_equal(_bits(out[16:16 + n]), _bits(host["visibility"]).reshape(-1))
        assert np.array_equal(_bits(out[32 + n:32 + 2 * n]), _bits(host["tested"]).reshape(-1))
        assert (out[:16] == -7).all() and (out[16 + n:32 + n] == -7).all() and (out[32 + 2 * n:] == -7).all()
        # before any sample: zeros
        g.clear()
        assert all((v == 0).all() for v in g.resolve().values())
    finally:
        g.close()
        r.close()


@pytest.mark.parametrize("w,h", [(31, 24), (37, 7), (16, 16)], ids=["31x24", "259_pixels", "one_block"])
@pytest.mark.parametrize("floor", [0.25, 0.1, 1.0])
def test_device_shade_equals_the_host_statement(spt, w, h, floor):
    rng = np.random.default_rng(w * h)
    alb = rng.random((h, w, 3)).astype(F)
    vis = rng.random((h, w)).astype(F)
    vis.reshape(-1)[:4] = (0.0, 1.0, 0.375, F(2.0 / 7.0))
    host = spt.light_shade_host(alb, vis, floor)
    assert np.array_equal(_bits(host), _bits(glt.shade_numpy(alb, vis, floor)))
    assert np.array_equal(_bits(spt.light_shade(alb, vis, floor)), _bits(host))
    assert np.array_equal(_bits(spt.light_shade(alb, vis, floor, in_place=True)), _bits(host))


def test_device_shade_rejections_and_bounds(spt):
    import torch
    lib = spt.load_library()
    n = 259
    buf = torch.full((3 * n + 32,), -7.0, dtype=torch.float32, device="cuda:0")
    alb = torch.full((3 * n,), 0.5, dtype=torch.float32, device="cuda:0")
    vis = torch.full((n,), 1.0, dtype=torch.float32, device="cuda:0")
    V = ctypes.c_void_p
    out = V(buf.data_ptr() + 4 * 16)
    for floor in (0.0, -0.25, 1.0000001, float("inf"), float("nan")):
        assert lib.spt_light_shade_async(V(alb.data_ptr()), V(vis.data_ptr()), n, floor, out, None) == 1
    assert lib.spt_light_shade_async(V(alb.data_ptr()), V(vis.data_ptr()), -1, 0.25, out, None) == 1
    assert lib.spt_light_shade_async(None, V(vis.data_ptr()), n, 0.25, out, None) == 1
    assert lib.spt_light_shade_async(None, None, 0, 0.25, None, None) == 0
    torch.cuda.synchronize(0)
    assert (buf.cpu().numpy() == -7).all()
    assert lib.spt_light_shade_async(V(alb.data_ptr()), V(vis.data_ptr()), n, 0.25, out, None) == 0
    torch.cuda.synchronize(0)
    got = buf.cpu().numpy()
    assert (got[:16] == -7).all() and (got[16 + 3 * n:] == -7).all() and (got[16:16 + 3 * n] == 0.5).all()


# ---- 5. neighbours are untouched -------------------------------------------------------------------
def test_a_light_guide_pass_leaves_the_context_and_a_guide_alone(spt, oracle):
    w, h = 31, 24
    a, b = gct.scene(spt, "head"), gct.scene(spt, "specular")
    cam = spt.Camera(aspect=_aspect(w, h))
    pa, pb = _params(spt, "head", w, h, 8), _params(spt, "specular", w, h, 4)

    def frame(r):
        return _frame(spt, r, a, cam, pa)

    fresh = spt.Renderer(0)
    alone = spt.Guide(pb, 0, True)
    try:  # the image and the guide's records of the calls alone
        img0, st0, k0 = frame(fresh)
        alone.render(fresh, b, cam, pb, 0, 4)
        guide0 = alone.to_numpy()
    finally:
        alone.close()
        fresh.close()
    want_light = glt.light_truth(oracle, b, cam._c, pb, chain=True)
    r = spt.Renderer(0)
    g, lg = spt.Guide(pb, 0, True), spt.LightGuide(pb, 0, True)
    try:
        img1, st1, k1 = frame(r)
        g.render(r, b, cam, pb, 0, 2)
        lg.render(r, b, cam, pb, 0, 2)
        assert r.kernel() == k0 and {k: r.stats()[k] for k in st0} == st0
        img2, st2, k2 = frame(r)
        lg.render(r, b, cam, pb, 2, 2)
        g.render(r, b, cam, pb, 2, 2)
        assert r.kernel() == k0 and {k: r.stats()[k] for k in st0} == st0
        img3, st3, k3 = frame(r)
        _same(g.to_numpy(), guide0, "the guide beside a light guide")
        _same(lg.to_numpy(), want_light, "the light guide between frames")
        assert k0 == k1 == k2 == k3 and st0 == st1 == st2 == st3
        assert np.array_equal(img0, img1) and np.array_equal(img0, img2) and np.array_equal(img0, img3)
    finally:
        lg.close()
        g.close()
        r.close()


# ---- 6. two geometric properties -------------------------------------------------------------------
def test_an_open_floor_is_lit(spt, oracle):
    """`head` without the two boxes, the parameters' rectangle set to the light primitive itself (HEAD's
    parameters sample z in [63, 99) at y = 81.6, its primitive ends at z = 96 at y = 81.5: a twelfth of the
    light points lie on the ceiling). Nothing then stands between the floor and a light point, so every
    tested sample on the floor is lit -- but for the contract's own self-hits: a vertex whose y the hit
    point's rounding left below the floor plane (x.y = -2^-18 from the camera's height 40) sends its
    shadow ray up through the floor, which is then the nearest hit. So: lit iff the vertex is not below
    the plane, sample by sample, and the device's sums are those."""
    w, h, spp = 16, 12, 8
    cam = spt.Camera(aspect=_aspect(w, h))
    p = _params(spt, "head", w, h, spp)
    p.light_dz, p.light_y, p.light_area = 33.0, 81.5, 36.0 * 33.0
    room = [spt.spt_prim.from_buffer_copy(q) for q in gct.scene(spt, "head")[:7]]  # without the two boxes
    g = list(room[p.light_id].geom)[:5]
    assert g == [p.light_x0, p.light_x0 + p.light_dx, p.light_z0, p.light_z0 + p.light_dz, p.light_y]
    want, det = glt.light_truth(oracle, room, cam._c, p, return_detail=True)
    on_floor = (det["vertex"] == 4) & det["tested"]
    above = on_floor & (det["x"][..., 1] >= 0)
    assert on_floor.sum() >= 300 and 10 * above.sum() >= 9 * on_floor.sum()
    assert np.array_equal(det["lit"][on_floor], above[on_floor])
    rec, _ = _light(spt, room, cam, p)
    _same(rec, want, "open floor")
    only_floor = (det["vertex"] == 4).all(axis=2)  # pixels whose every sample sees the floor
    assert only_floor.sum() >= 20
    assert np.array_equal(rec[only_floor][:, 0], np.full(only_floor.sum(), spp))
    assert np.array_equal(rec[only_floor][:, 1], above.sum(axis=2)[only_floor])
    assert (rec[only_floor][:, 2] > 0).all()


def test_a_covered_light_lights_nothing(spt, oracle):
    """`head` with a DIFF rectangle at y = 80 that covers the sample rectangle from below -- the whole room's
    cross-section, so that no surface above it is seen -- and a second one at y = 79, its underside: a
    single sheet has no thickness, and a vertex on it would send its shadow ray up from the sheet itself."""
    w, h, spp = 16, 12, 8
    cam = spt.Camera(aspect=_aspect(w, h))
    p = _params(spt, "head", w, h, spp)
    covered = gct.scene(spt, "head") + [spt.Rectangle_xz(1.0, 99.0, 0.0, 170.0, 80.0, 0, (0.5, 0.5, 0.5)),
                                        spt.Rectangle_xz(1.0, 99.0, 0.0, 170.0, 79.0, 0, (0.5, 0.5, 0.5))]
    rec, _ = _light(spt, covered, cam, p)
    assert rec[..., 0].sum() >= w * h * spp * 9 // 10
    assert not rec[..., 1].any() and not rec[..., 2].any()  # lit == 0 everywhere
    want, det = glt.light_truth(oracle, covered, cam._c, p, return_detail=True)
    _same(rec, want, "covered light")
    assert (det["vertex"] == 18).any() and not (det["vertex"] == 17).any()  # the underside is seen, the sheet is not


# ---- 7. denoising ----------------------------------------------------------------------------------
W, H, SPP, GUIDE_SPP = 31, 24, 32, 16


def test_render_denoised_with_a_light_guide_equals_the_manual_sequence(spt):
    prims = gct.scene(spt, "head")
    cam = spt.Camera(aspect=_aspect(W, H))
    p = spt.default_params(width=W, height=H, spp=SPP, seed=1)
    batch = SPP // 8
    r, film, guide, lg = spt.Renderer(0), spt.Film(p, 0), spt.Guide(p, 0), spt.LightGuide(p, 0)
    dn = spt.Denoiser(W, H, 0)
    try:
        film.enable_noise(batch)
        for k in range(8):
            film.render(r, prims, cam, p, k * batch, batch)
            r.stats()
        guide.render(r, prims, cam, p, 0, GUIDE_SPP)
        lg.render(r, prims, cam, p, 0, GUIDE_SPP)
        planes = guide.resolve()
        vis = lg.resolve()["visibility"]
        assert (vis == 0).any() and (vis == 1).any() and ((vis > 0) & (vis < 1)).any()
        rgb, se = film.resolve(), film.noise_map()
        manual = {}
        for floor in (0.25, 0.5):
            shaded = spt.light_shade(planes["albedo"], vis, floor)
            assert np.array_equal(_bits(shaded), _bits(spt.light_shade_host(planes["albedo"], vis, floor)))
            manual[floor] = dn.denoise(rgb, se, shaded, planes["normal"], planes["depth"], return_se=True)
        off, off_se = dn.denoise_film(film, guide, return_se=True)  # today's path: spt_film_denoise
    finally:
        dn.close()
        lg.close()
        guide.close()
        film.close()
        r.close()
    for floor in (0.25, 0.5):
        got, info = spt.render_denoised(prims, cam, p, guide_spp=GUIDE_SPP, return_info=True, light_guide=True,
                                        shade_floor=floor)
        assert np.array_equal(_bits(got), _bits(manual[floor][0])), floor
        assert np.array_equal(_bits(info["se"]), _bits(manual[floor][1])), floor
        assert np.array_equal(_bits(info["guides"]["visibility"]), _bits(vis))
        assert np.array_equal(_bits(info["guides"]["albedo_unshaded"]), _bits(planes["albedo"]))
        assert np.array_equal(_bits(info["noisy"]), _bits(rgb))
    assert not np.array_equal(manual[0.25][0], manual[0.5][0]) and not np.array_equal(manual[0.25][0], off)
    assert np.array_equal(_bits(spt.render_denoised(prims, cam, p, guide_spp=GUIDE_SPP, light_guide=True)),
                          _bits(manual[0.25][0]))  # the default floor
    got, info = spt.render_denoised(prims, cam, p, guide_spp=GUIDE_SPP, return_info=True)  # the default: off
    assert np.array_equal(_bits(got), _bits(off)) and np.array_equal(_bits(info["se"]), _bits(off_se))
    assert "visibility" not in info["guides"]
    got = spt.render_denoised(prims, cam, p, guide_spp=GUIDE_SPP, light_guide=False)
    assert np.array_equal(_bits(got), _bits(off))


def test_render_denoised_pair_with_a_light_guide_equals_the_manual_sequence(spt):
    prims = gct.scene(spt, "specular")
    cam = spt.Camera(aspect=_aspect(W, H))
    p = spt.default_params(width=W, height=H, spp=SPP, seed=1)
    batch = SPP // 8
    r, fa, fb = spt.Renderer(0), spt.Film(p, 0), spt.Film(p, 0)
    guide, lg = spt.Guide(p, 0, True), spt.LightGuide(p, 0, True)
    dn = spt.Denoiser(W, H, 0)
    try:
        for f in (fa, fb):
            f.enable_noise(batch)
        for k in range(8):
            (fb if k & 1 else fa).render(r, prims, cam, p, k * batch, batch)
            r.stats()
        guide.render(r, prims, cam, p, 0, GUIDE_SPP)
        lg.render(r, prims, cam, p, 0, GUIDE_SPP)
        planes = guide.resolve()
        shaded = spt.light_shade(planes["albedo"], lg.resolve()["visibility"], 0.25)
        want = dn.denoise_pair(fa.resolve(), fa.noise_map(), fb.resolve(), fb.noise_map(), shaded,
                               planes["normal"], planes["depth"])
        off = dn.denoise_film_pair(fa, fb, guide)
    finally:
        dn.close()
        lg.close()
        guide.close()
        fb.close()
        fa.close()
        r.close()
    got, info = spt.render_denoised_pair(prims, cam, p, guide_spp=GUIDE_SPP, through_specular=True,
                                         return_info=True, light_guide=True)
    for a, b, name in zip((got, info["se"], info["diff"]), want, ("out", "se", "diff")):
        assert np.array_equal(_bits(a), _bits(b)), name
    assert not np.array_equal(got, off[0])
    plain = spt.render_denoised_pair(prims, cam, p, guide_spp=GUIDE_SPP, through_specular=True)
    assert np.array_equal(_bits(plain), _bits(off[0]))


# ---- 8. the drop-in program ------------------------------------------------------------------------
def test_dropin_writes_the_light_planes_and_denoises_with_a_light_guide(spt, tmp_path):
    w, h, spp = 48, 32, 16
    plain, with_light = tmp_path / "plain.ppm", tmp_path / "out.ppm"
    prefix = str(tmp_path / "g")
    for args in ([str(plain)], [str(with_light), "--guides", prefix, "--light"]):
        run = subprocess.run([EXE, str(w), str(h), str(spp), "5"] + args, capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stdout + run.stderr
    assert plain.read_bytes() == with_light.read_bytes()
    prims, cam = spt.cornell_scene(), spt.Camera(aspect=_aspect(w, h))
    p = spt.default_params(width=w, height=h, spp=spp, seed=5)
    want = spt.render_light_guides(prims, cam, p)
    assert set(want) == {"visibility", "direct", "tested"} and 0 < want["visibility"].mean() < 1
    for k in ("visibility", "direct"):
        got = _read_pfm(prefix + f"_{k}.pfm")
        for c in range(3):
            assert np.array_equal(_bits(got[..., c]), _bits(want[k])), k
    albedo = _read_pfm(prefix + "_albedo.pfm")  # the guide's planes are there as before
    assert np.array_equal(_bits(albedo), _bits(spt.render_guides(prims, cam, p)["albedo"]))
    p1 = spt.default_params(width=w, height=h, spp=spp, seed=1)
    out = tmp_path / "d.pfm"
    for extra, kw in ((["--shade-floor", "0.5"], dict(shade_floor=0.5)), ([], {})):
        run = subprocess.run([EXE, str(w), str(h), str(spp), "1", str(out), "--pfm", "--denoise", "--light-guide"]
                             + extra, capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stdout + run.stderr
        raw = out.read_bytes()
        data = np.frombuffer(raw[len(raw) - w * h * 12:], dtype="<f4").reshape(h, w, 3)[::-1]
        assert np.array_equal(_bits(data), _bits(spt.render_denoised(prims, cam, p1, guide_spp=spp, light_guide=True, **kw)))
    run = subprocess.run([EXE, str(w), str(h), str(spp), "1", str(out), "--pfm", "--denoise", "--pair", "--light-guide"],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "PAIR :" in run.stdout, run.stdout + run.stderr
    raw = out.read_bytes()
    data = np.frombuffer(raw[len(raw) - w * h * 12:], dtype="<f4").reshape(h, w, 3)[::-1]
    assert np.array_equal(_bits(data), _bits(spt.render_denoised_pair(prims, cam, p1, guide_spp=spp, light_guide=True)))
    for args in (["--light"], ["--light-guide"], ["--denoise", "--shade-floor", "0.5"],
                 ["--denoise", "--light-guide", "--shade-floor", "0"],
                 ["--denoise", "--pair", "--bank", "2,4", "--light-guide"]):
        bad = subprocess.run([EXE, str(w), str(h), str(spp), "1", str(out)] + args, capture_output=True, text=True,
                             timeout=120)
        assert bad.returncode != 0, args
    usage = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert all(f in usage for f in ("--light ", "--light-guide", "--shade-floor"))

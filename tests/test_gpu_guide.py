"""The guide planes on the GPU (include/spt.h SPT_HAS_GUIDE; guide_kernel in spt_guide.hip): every
comparison is on the downloaded int64 records, exact, against tests/guide_truth.py (the contract
restated from the oracle's pieces) or against the render kernels themselves.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import guide_chain_truth as gct
import guide_truth as gt
import ray_truth as rt
from test_gpu_rays import ray_camera

pytestmark = pytest.mark.gpu
SEED = 5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _aspect(w, h):
    return float(np.float32(w) / np.float32(h))


def _scene(spt, name):
    if name in ("specular", "mirror_glass", "hall"):
        return gct.scene(spt, name)
    return rt.scene(spt, name)


def _params(spt, w, h, spp, **kw):
    return spt.default_params(width=w, height=h, spp=spp, seed=SEED, **kw)


def _guide(spt, prims, cam, p, windows=None, renderer=None):
    """-> (records, info) of a fresh guide filled with `windows` (default: the full one)."""
    r = renderer or spt.Renderer(p.device)
    g = spt.Guide(p, p.device)
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


# ---- 1. the truth, per scene class -----------------------------------------------------------------
TRUTH_CASES = [("head_ref", "head", {}, 64, 48, 8), ("head_tilted", "head", rt.TILTED, 64, 48, 8),
               ("spheres32", "spheres32", {}, 64, 48, 8), ("specular", "specular", {}, 48, 32, 4),
               ("classic", "classic", {}, 32, 24, 4),
               # first hits mostly specular: a first-hit pass must stop there, not step on as a chain does
               # (mirror_glass: the wide instantiation; hall: mirror rectangles, free-scale directions)
               ("mirror_glass", "mirror_glass", {}, 32, 24, 4), ("hall", "hall", gct.HALL_CAM, 32, 24, 4)]


@pytest.mark.parametrize("label,name,camkw,w,h,spp", TRUTH_CASES, ids=[c[0] for c in TRUTH_CASES])
def test_records_equal_the_truth(spt, oracle, label, name, camkw, w, h, spp):
    prims = _scene(spt, name)
    cam = spt.Camera(aspect=_aspect(w, h), **camkw)
    # (a Camera is its four raw vectors: the tilted one has no zero component among them)
    # (the classic boxes have no light rectangle: their params carry nee_prob = 0, as their renders do)
    p = _params(spt, w, h, spp, **(dict(nee_prob=0.0) if name in ("classic", "mirror_glass") else {}))
    if name in ("classic", "mirror_glass"):
        assert spt.select_kernel(prims, cam, p)["name"] == "wide"  # the guide's instantiation follows it
    rec, info = _guide(spt, prims, cam, p)
    assert info["samples_done"] == spp and info["width"] == w and info["rows"] == h
    want = gt.guide_truth(oracle, prims, cam._c, p)
    assert want[..., 7].sum() > 0
    _same(rec, want, label)


# ---- 2. against the render kernels, independently of the truth helper -------------------------------
# With every primitive emitting its colour, max_depth = 1 and nee_prob = 0 a render is the first hit's
# colour in the same 1.31 sums. The depth cap takes the HEAD scene off the estimator-specialised
# variants (they are compiled for max_depth == 0), so the literal-geometry kernel "const" runs it; the
# classic box runs "wide". Either way a specialised render variant against the generic guide kernel.
@pytest.mark.parametrize("name,w,h,spp,variant", [("head", 64, 48, 8, "const"), ("classic", 32, 24, 4, "wide")])
def test_albedo_slots_equal_a_film_of_the_albedo_scene(spt, name, w, h, spp, variant):
    prims = _scene(spt, name)
    cam = spt.Camera(aspect=_aspect(w, h))
    p = _params(spt, w, h, spp, max_depth=1, nee_prob=0.0)
    r, film = spt.Renderer(0), spt.Film(p, 0)
    try:
        film.render(r, gt.albedo_scene(spt, prims), cam, p, 0, spp)
        st = r.stats()
        assert st["misses"] == 0 and st["samples"] == w * h * spp
        assert r.kernel() == variant
        sums = film.to_numpy()
        rec, _ = _guide(spt, prims, cam, p, renderer=r)
        assert r.kernel() == variant  # the guide pass is no render
    finally:
        film.close()
        r.close()
    _same(rec[..., 0:3].astype(np.uint64), sums, name)
    assert (rec[..., 7] == spp).all()


# ---- 3. windows ------------------------------------------------------------------------------------
def test_windows_add_up_in_any_order(spt, oracle):
    prims = _scene(spt, "head")
    cam = spt.Camera(aspect=_aspect(64, 48))
    p = _params(spt, 64, 48, 8)
    one, _ = _guide(spt, prims, cam, p)
    ab, ia = _guide(spt, prims, cam, p, [(0, 3), (3, 5)])
    ba, ib = _guide(spt, prims, cam, p, [(3, 5), (0, 3)])
    assert ia["samples_done"] == ib["samples_done"] == 8
    _same(ab, one, "[0,3)+[3,8)")
    _same(ba, one, "[3,8)+[0,3)")
    part, ip = _guide(spt, prims, cam, p, [(1, 3)])
    assert ip["samples_done"] == 3
    _same(part, gt.guide_truth(oracle, prims, cam._c, p, 1, 3), "[1,4)")


# ---- 4. lane groups --------------------------------------------------------------------------------
# K = the smallest power of two that fills the device's resident lanes (256 CUs x 8 blocks x 256 lanes
# on an MI355X: 2^19), capped by the window's sample count rounded up: 8x4 pixels always hit the cap.
LANE_CASES = [("8x4_spp96", 8, 4, 96, (0, 96)), ("8x4_window5", 8, 4, 96, (0, 5)),
              ("256x192_spp2", 256, 192, 2, (0, 2))]
_lane_results = {}


def _lane_case(spt, oracle, label):
    """Render one of LANE_CASES (once per session) -> (records, truth, lanes per pixel)."""
    if label not in _lane_results:
        _, w, h, spp, window = next(c for c in LANE_CASES if c[0] == label)
        prims = _scene(spt, "head")
        cam = spt.Camera(aspect=_aspect(w, h))
        p = _params(spt, w, h, spp)
        rec, info = _guide(spt, prims, cam, p, [window])
        _lane_results[label] = (rec, gt.guide_truth(oracle, prims, cam._c, p, *window),
                                info["lanes_per_pixel"])
    return _lane_results[label]


@pytest.mark.parametrize("label", [c[0] for c in LANE_CASES])
def test_lane_groups(spt, oracle, label):
    rec, want, k = _lane_case(spt, oracle, label)
    assert k in (1, 2, 4, 8, 16, 32, 64)
    _same(rec, want, label)


def test_lane_groups_covered_every_width(spt, oracle):
    seen = {c[0]: _lane_case(spt, oracle, c[0])[2] for c in LANE_CASES}
    ks = set(seen.values())
    assert seen["8x4_spp96"] == 64, seen
    assert ks & {1, 2} and ks & {4, 8, 16, 32} and 64 in ks, seen


# ---- 5. shards -------------------------------------------------------------------------------------
def test_shards_hold_their_rows(spt, oracle):
    prims = _scene(spt, "head")
    w, h, spp = 64, 44, 8  # a ragged last tile
    cam = spt.Camera(aspect=_aspect(w, h))
    whole, _ = _guide(spt, prims, cam, _params(spt, w, h, spp, tile_rows=8))
    seen = []
    for k in range(3):
        p = _params(spt, w, h, spp, tile_rows=8, shard_index=k, shard_count=3)
        rows = spt.shard_rows(p)
        rec, info = _guide(spt, prims, cam, p)
        assert info["rows"] == len(rows)
        _same(rec, whole[rows], f"shard {k}")
        seen += list(rows)
    assert sorted(seen) == list(range(h))
    p = _params(spt, w, h, spp, tile_rows=8, shard_index=7, shard_count=8)  # 6 tiles: no rows
    assert len(spt.shard_rows(p)) == 0
    rec, info = _guide(spt, prims, cam, p, [(0, 3)])
    assert rec.shape == (0, w, 8) and info["samples_done"] == 3 and info["rows"] == 0


# ---- 6. edge rays ----------------------------------------------------------------------------------
def _edge_views(spt, oracle):
    """A handful of the F2-F6 views of tests/ray_truth.py: a zero direction component, a rectangle
    edge graze, a box corner, a sphere tangent, roots at the sphere epsilon."""
    picks = {"head": ("F2_o0_d2", "F2_o2_d5", "F4_box16_edge_mid", "F4_box11_top_corner", "F4_room_corner0",
                      "F3_0_ray"),
             "three_spheres": ("F4_s7_tangent", "F5_s7_front2e-3", "F5_s7_front1e-3", "F5_s9_surface_out",
                               "F2_o1_d0")}
    out = []
    for name, labels in picks.items():
        views = {v[0]: v for v in rt.views(spt, oracle, name, "raw")}
        missing = [lb for lb in labels if lb not in views]
        assert not missing, (name, missing, sorted(views))
        out += [(name, views[lb]) for lb in labels]
    return out


def test_edge_rays(spt, oracle):
    n_single = n_miss = 0
    for name, (label, o, L, hor, ver, w, h) in _edge_views(spt, oracle):
        prims = rt.scene(spt, name)
        cam = ray_camera(spt, o, L, hor, ver)
        p = _params(spt, w, h, 8)
        rec, _ = _guide(spt, prims, cam, p)
        want = gt.guide_truth(oracle, prims, cam._c, p)
        _same(rec, want, label)
        if not any(hor) and not any(ver):  # every sample is one known ray: the oracle's verdict on it
            o32, d = gt.camera_rays(oracle, cam._c, p, [0], 0, 1, gt.unit_dirs(prims))
            one = gt.ray_records(oracle, prims, p, o32, d.reshape(-1, 3)[:1])[0]
            t, ids = oracle.intersect_batch(prims, p, o32[None, :], d.reshape(-1, 3)[:1])
            assert one[7] == (1 if ids[0] >= 0 else 0)
            assert (rec == 8 * one[None, None, :]).all(), label
            n_single += 1
            n_miss += int(ids[0] < 0)
    assert n_single >= 5 and n_miss >= 1  # (a zero component in the closed room is a miss)


# ---- 7. a context between frames -------------------------------------------------------------------
def _frame(spt, r, prims, cam, p):
    import torch
    buf = torch.empty(p.height * p.width * 3, dtype=torch.float32, device="cuda:0")
    r.render_async(prims, cam, p, buf.data_ptr())
    st = r.stats()
    torch.cuda.synchronize(0)
    keys = spt.STAT_KEYS + ["shadow_proven"]
    return buf.cpu().numpy(), {k: st[k] for k in keys}, r.kernel()


def test_a_guide_pass_between_frames_leaves_the_context_alone(spt, oracle):
    a = _scene(spt, "head")
    b = _scene(spt, "spheres32")
    cam = spt.Camera(aspect=_aspect(64, 48))
    pa = _params(spt, 64, 48, 8)
    pb = _params(spt, 64, 48, 4)
    fresh = spt.Renderer(0)
    img0, st0, k0 = _frame(spt, fresh, a, cam, pa)
    fresh.close()
    truth_b = gt.guide_truth(oracle, b, cam._c, pb)
    r = spt.Renderer(0)
    g = spt.Guide(pb, 0)
    film = spt.Film(pa, 0)
    film0 = spt.Film(pa, 0)
    try:
        img1, st1, k1 = _frame(spt, r, a, cam, pa)
        g.render(r, b, cam, pb, 0, 4)
        assert r.kernel() == k0 and {k: r.stats()[k] for k in st0} == st0
        img2, st2, k2 = _frame(spt, r, a, cam, pa)
        _same(g.to_numpy(), truth_b, "guide of B between frames of A")
        assert k0 == k1 == k2 and st0 == st1 == st2
        assert np.array_equal(img0, img1) and np.array_equal(img0, img2)
        # ... and with a film pass in place of the second frame
        g.clear()
        g.render(r, b, cam, pb, 0, 4)
        film.render(r, a, cam, pa, 0, 8)
        st3 = {k: r.stats()[k] for k in st0}
        fresh = spt.Renderer(0)
        film0.render(fresh, a, cam, pa, 0, 8)
        fresh.stats()
        assert st3 == st0 and r.kernel() == k0
        assert np.array_equal(film.to_numpy(), film0.to_numpy())
        fresh.close()
        _same(g.to_numpy(), truth_b, "guide of B before a film pass of A")
    finally:
        film.close()
        film0.close()
        g.close()
        r.close()


# ---- 8. rejections ---------------------------------------------------------------------------------
def test_rejected_calls_leave_the_guide_untouched(spt):
    import torch
    prims = _scene(spt, "head")
    cam = spt.Camera(aspect=_aspect(32, 24))
    p = _params(spt, 32, 24, 8)
    r, g = spt.Renderer(0), spt.Guide(p, 0)
    try:
        g.render(r, prims, cam, p, 0, 5)
        before, info = g.to_numpy(), g.info()
        bad = [(_params(spt, 31, 24, 8), 5, 1), (p, 7, 2), (p, 8, 1), (p, 0, 4), (p, 5, 0),
               (_params(spt, 32, 24, 9), 5, 1), (_params(spt, 32, 24, 8, shard_count=2), 5, 1)]
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
    finally:
        g.close()
        r.close()
    with pytest.raises(spt.SptError):
        spt.Guide(_params(spt, 4, 4, (1 << 24) + 1), 0)


# ---- 9. resolve ------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [(0, 8), (2, 3)], ids=["full", "partial"])
def test_device_resolve_equals_the_host_statement(spt, window):
    import torch
    prims = _scene(spt, "three_spheres")
    w, h = 40, 24
    # from outside the room, wider than its back wall: hits, misses and pixels with both
    cam = ray_camera(spt, (50, 40, 300), (-100, -75, -100), (200, 0, 0), (0, 150, 0))
    p = _params(spt, w, h, 8)
    r, g = spt.Renderer(0), spt.Guide(p, 0)
    try:
        g.render(r, prims, cam, p, *window)
        rec = g.to_numpy()
        assert 0 < rec[..., 7].sum() < w * h * window[1]  # hits and misses both
        host = spt.guide_resolve_host(rec, w, h, 8, window[1])
        dev = g.resolve()
        for k in spt.GUIDE_PLANES:
            assert np.array_equal(dev[k].view(np.uint32), host[k].view(np.uint32)), k
        some = g.resolve(planes=("normal", "coverage"))
        assert set(some) == {"normal", "coverage"}
        for k in some:
            assert np.array_equal(some[k].view(np.uint32), host[k].view(np.uint32)), k
        # the planes left NULL are not written: one buffer, sentinels around the two planes asked for
        n = w * h
        buf = torch.full((n * 5 + 64,), -7.0, dtype=torch.float32, device="cuda:0")
        lib = spt.load_library()
        assert lib.spt_guide_resolve(g._g, None, ctypes.c_void_p(buf.data_ptr() + 4 * 16), None,
                                     ctypes.c_void_p(buf.data_ptr() + 4 * (32 + 3 * n)), None) == 0
        torch.cuda.synchronize(0)
        out = buf.cpu().numpy()
        assert np.array_equal(out[16:16 + 3 * n].view(np.uint32), host["normal"].reshape(-1).view(np.uint32))
        assert np.array_equal(out[32 + 3 * n:32 + 4 * n].view(np.uint32),
                              host["coverage"].reshape(-1).view(np.uint32))
        assert (out[:16] == -7).all() and (out[16 + 3 * n:32 + 3 * n] == -7).all() and (out[32 + 4 * n:] == -7).all()
    finally:
        g.close()
        r.close()


# ---- 10. the drop-in program -----------------------------------------------------------------------
def _read_pfm(path):
    data = open(path, "rb").read()
    assert data[:3] == b"PF\n"
    w, h = (int(x) for x in data[3:].split(b"\n", 1)[0].split())
    a = np.frombuffer(data[len(data) - 12 * w * h:], dtype="<f4").reshape(h, w, 3)
    return a[::-1]  # scanlines bottom to top


def test_dropin_writes_the_guide_planes(spt, tmp_path):
    exe = os.path.join(ROOT, "small-pathtracer_amd", "smallpt_amd")
    plain, with_guides = tmp_path / "plain.ppm", tmp_path / "out.ppm"
    prefix = str(tmp_path / "g")
    for args in ([str(plain)], [str(with_guides), "--guides", prefix]):
        r = subprocess.run([exe, "64", "48", "8", "5"] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
    assert plain.read_bytes() == with_guides.read_bytes()
    p = _params(spt, 64, 48, 8)
    want = spt.render_guides(spt.cornell_scene(), spt.Camera(aspect=_aspect(64, 48)), p)
    assert want["coverage"].min() == 1.0
    for k in ("albedo", "normal"):
        got = _read_pfm(prefix + f"_{k}.pfm")
        assert np.array_equal(got.view(np.uint32), want[k].view(np.uint32)), k
    got = _read_pfm(prefix + "_depth.pfm")
    for c in range(3):
        assert np.array_equal(got[..., c].view(np.uint32), want["depth"].view(np.uint32))
    assert (want["normal"] < 0).any()  # signed normals survive the PFM encoder

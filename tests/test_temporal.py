"""Temporal accumulation (include/spt.h SPT_HAS_TEMPORAL) on the CPU: the host statement
spt_temporal_accumulate_host against tests/temporal_truth.py (the header's text restated in numpy
float32), bit for bit on every output and every state plane, and the properties the header's rules imply.
"""
import ctypes

import numpy as np
import pytest

import temporal_truth as tt

SIZES = [(1, 1), (3, 2), (5, 1), (1, 5), (17, 13), (40, 56)]
PLANES = ("rgb", "se", "n", "hist")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want, label):
    for k in PLANES:
        assert np.array_equal(bits(got[k]), bits(want[k])), f"{label}: {k} differs"
    for k in tt.STATE_PLANES:
        assert np.array_equal(bits(got["state"][k]), bits(want["state"][k])), f"{label}: state {k} differs"


def host(spt, f, cam, prev=None, prev_cam=None, **kw):
    return spt.temporal_accumulate_host(*tt.planes_of(f), tt.to_struct(spt, cam), spt.default_temporal_params(**kw),
                                        prev, tt.to_struct(spt, prev_cam) if prev_cam is not None else None)


def both(spt, f, cam, prev, prev_cam, label, **kw):
    """One frame by the host statement and by the restatement, compared; -> the host's result."""
    got = host(spt, f, cam, prev, prev_cam, **kw)
    want = tt.accumulate_truth(*tt.planes_of(f), cam, prev, prev_cam, **kw)
    same(got, want, label)
    return got


@pytest.mark.parametrize("n_max", [1.0, 2.0, 32.0])
@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_host_statement_equals_the_truth(spt, w, h, flags, n_max):
    kw = dict(flags=flags, n_max=n_max)
    cam0 = tt.camera(w, h)
    frames = [tt.frame(cam0, w, h, seed) for seed in (1, 2, 3)]
    r1 = both(spt, frames[0], cam0, None, None, "first frame", **kw)
    assert np.all(r1["n"] == (frames[0]["depth"] != 0)), "a first frame has n = 1, 0 at a miss"
    r2 = both(spt, frames[1], cam0, r1["state"], cam0, "same camera, second frame", **kw)
    r3 = both(spt, frames[2], cam0, r2["state"], cam0, "same camera, third frame", **kw)
    cam1 = tt.camera(w, h, origin=(1.3, -0.7, 0.5))
    r4 = both(spt, tt.frame(cam1, w, h, 4), cam1, r3["state"], cam0, "shifted camera", **kw)
    if w * h >= 17 * 13:  # the shifted camera does reproject, and through all four taps
        took = np.any(r4["hist"] != r4["rgb"], axis=-1)
        assert took.mean() > 0.3 and np.all(r4["n"][took] <= min(4.0, n_max)) and np.all(r4["n"][~took] <= 1)
    # the previous camera looks at the scene from behind it: C <= 0 at every pixel
    behind = tt.camera(w, h, origin=(0.0, 0.0, -200.0))
    r5 = both(spt, frames[0], cam0, r3["state"], behind, "behind the previous camera", **kw)
    assert np.array_equal(bits(r5["n"]), bits(r1["n"])) and np.array_equal(bits(r5["hist"]), bits(frames[0]["rgb"]))
    # the previous camera stood so far to the side that every tap lies outside its image
    far = tt.camera(w, h, origin=(1000.0, 0.0, 0.0))
    r6 = both(spt, frames[0], cam0, r3["state"], far, "every tap outside", **kw)
    assert np.array_equal(bits(r6["n"]), bits(r1["n"])) and np.array_equal(bits(r6["rgb"]), bits(r1["rgb"]))


def test_host_statement_equals_the_truth_with_other_parameters(spt):
    w, h = 17, 13
    kw = dict(n_max=5.5, normal_min=0.3, plane_tol=0.2, albedo_floor=0.3)
    cam0, cam1 = tt.camera(w, h), tt.camera(w, h, origin=(-2.0, 1.0, -3.0))
    r1 = both(spt, tt.frame(cam0, w, h, 7), cam0, None, None, "first", **kw)
    r2 = both(spt, tt.frame(cam1, w, h, 8), cam1, r1["state"], cam0, "moved", **kw)
    assert np.any(r2["n"] == 2) and np.any(r2["n"] == 1)


def test_inputs_that_are_not_finite_agree_too(spt):
    w, h = 17, 13
    cam0, cam1 = tt.camera(w, h), tt.camera(w, h, origin=(1.3, -0.7, 0.5))
    f0, f1 = tt.frame(cam0, w, h, 1), tt.frame(cam1, w, h, 2)
    rng = np.random.default_rng(5)
    for f in (f0, f1):
        for k in ("rgb", "se", "albedo", "normal", "depth"):
            a = f[k].reshape(-1)
            a[rng.integers(0, a.size, 6)] = [np.nan, np.inf, -np.inf, -1.0, 3e38, -0.0]
    r1 = host(spt, f0, cam0)
    w1 = tt.accumulate_truth(*tt.planes_of(f0), cam0)
    r2 = host(spt, f1, cam1, r1["state"], cam0)
    w2 = tt.accumulate_truth(*tt.planes_of(f1), cam1, w1["state"], cam0)
    for got, want in ((r1, w1), (r2, w2)):
        for k in PLANES:  # NaN payloads are unspecified: compare the values
            assert np.array_equal(got[k], want[k], equal_nan=True), k


# ---- (a) the same camera: the history's length and the error estimate -----------------------------
@pytest.mark.parametrize("n_max", [4.0, 32.0])
def test_same_camera_counts_frames_and_divides_the_variance(spt, n_max):
    w, h, se = 17, 13, 0.04
    cam = tt.camera(w, h)
    hit = tt.frame(cam, w, h, 0)["depth"] != 0
    prev, v = None, 0.0
    for k in range(1, int(n_max) + 9):
        f = tt.frame(cam, w, h, k, se=se, short_normals=False)
        r = host(spt, f, cam, prev, cam if prev is not None else None, n_max=n_max,
                 flags=spt.TEMPORAL_NO_DEMODULATE)
        prev = r["state"]
        n = min(k, int(n_max))
        assert np.all(r["n"][hit] == n) and np.all(r["n"][~hit] == 0), k
        # the header's recurrence in fp64: var / k while the length grows, the exponential average after
        alpha = 1.0 / n
        v = (1.0 - alpha) ** 2 * v + alpha ** 2 * float(np.float32(se)) ** 2
        if k <= n_max:
            assert abs(v - float(np.float32(se)) ** 2 / k) <= 1e-15
        rel = np.abs(r["se"][hit].astype(np.float64) / np.sqrt(v) - 1.0).max()
        # at most n_max = 32 blends of a few roundings each, halved by the square root
        assert rel <= 2.0 ** -20, (k, rel)
        assert np.array_equal(bits(r["se"][~hit]), bits(f["se"][~hit])), "a miss keeps its own se"


# ---- (b) a fronto-parallel wall, the camera moved sideways by whole pixels ------------------------
@pytest.mark.parametrize("k", [1, -3])
def test_sideways_move_shifts_the_history_by_whole_pixels(spt, k):
    w, h, depth, a = 40, 24, 64.0, 0.5
    wall = [(-1e4, 1e4, -1e4, 1e4, -depth, (0.7, 0.6, 0.5))]
    move = k * 2.0 * a * depth / w  # a pixel's footprint on the wall is 2 a depth / w wide
    cam0, cam1 = tt.camera(w, h, half_width=a), tt.camera(w, h, origin=(move, 0.0, 0.0), half_width=a)
    f0 = tt.frame(cam0, w, h, 1, rects=wall)
    f1 = tt.frame(cam1, w, h, 2, rects=wall)
    r0 = host(spt, f0, cam0)
    r1 = host(spt, f1, cam1, r0["state"], cam0)
    # where the fp64 caster's world point lands in the previous image, in fp64
    _, _, X = tt.cast(cam1, w, h, wall)
    o, llc, hor, ver = cam0
    M = np.linalg.inv(np.stack([hor / w, ver / h, llc - o], axis=1))
    A, B, C = np.moveaxis((X - o) @ M.T, -1, 0)
    fx, fy = A / C, (h - 1) - B / C
    gy, gx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    lx, ly = np.rint(fx).astype(int), np.rint(fy).astype(int)
    assert np.all(lx == gx + k) and np.all(ly == gy), "the move is not k whole pixels"
    # the statement's own landing point is an fp32 one: the world point (three roundings of a value near
    # depth), q and M q (three products and two sums each) and two divisions put it within
    # 32 * 2^-24 * (depth / footprint) = 2^-19 * w / (2 a) pixels of the fp64 one
    slack = 2.0 ** -19 * w / (2.0 * a)
    off = (np.abs(fx - lx) + slack) + (np.abs(fy - ly) + slack)
    inside = (lx >= 1) & (lx < w - 1) & (ly >= 1) & (ly < h - 1)
    assert inside.sum() >= (w - 2 - abs(k)) * (h - 2)
    prev = f0["rgb"].astype(np.float64)
    pad = np.pad(prev, ((1, 1), (1, 1), (0, 0)), mode="edge")
    nb = np.stack([pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    spread = np.abs(nb - prev[None]).max(axis=0)  # the largest neighbour difference at every pixel
    assert np.all(r1["n"][inside] == 2)
    want = prev[ly[inside], lx[inside]]
    # the offset times the neighbour difference, and the roundings of rgb / a, the blend of taps and * a
    bound = off[inside][:, None] * spread[ly[inside], lx[inside]] + 8 * 2.0 ** -24 * np.abs(want)
    err = np.abs(r1["hist"][inside].astype(np.float64) - want)
    assert np.all(err <= bound), (err.max(), bound[err > bound][:3])


# ---- (c) disocclusion -----------------------------------------------------------------------------
def test_disocclusion_resets_the_history(spt):
    w, h, a = 64, 48, 0.5
    # a wall at depth 100 and a square at depth 50 over the central 16 x 12 pixels (columns 24..39, rows
    # 18..29); the camera moves so that the wall moves 2 pixels and the square 4
    scene = [(-1e4, 1e4, -1e4, 1e4, -100.0, (0.7, 0.6, 0.5)), (-6.4, 5.6, -5.0, 4.3, -50.0, (0.2, 0.5, 0.8))]
    move = 2 * 2.0 * a * 100.0 / w
    cam0, cam1 = tt.camera(w, h, half_width=a), tt.camera(w, h, origin=(move, 0.0, 0.0), half_width=a)
    f0 = tt.frame(cam0, w, h, 1, rects=scene, short_normals=False)
    f1 = tt.frame(cam1, w, h, 2, rects=scene, short_normals=False)
    sq0 = np.argwhere(f0["id"] == 1)
    assert (sq0.min(0).tolist(), sq0.max(0).tolist()) == ([18, 24], [29, 39])
    sq1 = np.argwhere(f1["id"] == 1)
    assert (sq1.min(0).tolist(), sq1.max(0).tolist()) == ([18, 20], [29, 35]), "the square moves 4 pixels"
    r0 = host(spt, f0, cam0)
    r1 = host(spt, f1, cam1, r0["state"], cam0)
    # wall points the square hid from the previous camera: the fp64 caster's ray from there hits the square
    _, pid1, X1 = tt.cast(cam1, w, h, scene)
    d = X1 - cam0[0]
    dist = np.linalg.norm(d, axis=-1)
    t_prev, pid_prev, _ = tt.cast_rays(cam0[0], d / dist[..., None], scene)
    hidden = (pid1 == 0) & (pid_prev == 1)
    assert hidden.sum() == 2 * 12, "a strip two pixels wide beside the square"
    assert np.all(r1["n"][hidden] == 1)

    def band(pid):  # a pixel of another depth lies within 2 pixels (on either side of a depth edge)
        p = np.pad(pid, 2, mode="edge")
        return np.any([p[2 + dy:2 + dy + h, 2 + dx:2 + dx + w] != pid for dy in range(-2, 3) for dx in range(-2, 3)],
                      axis=0)

    border = np.ones((h, w), bool)
    border[2:-2, 2:-2] = False
    left_out = band(f0["id"]) | band(f1["id"]) | border
    assert left_out.mean() <= 0.30, left_out.mean()
    assert np.all(r1["n"][~left_out] == r0["n"][~left_out] + 1)
    assert np.all(r0["n"] == 1)


# ---- the Python mirror ----------------------------------------------------------------------------
def test_python_mirror(spt):
    assert spt.SPT_HAS_TEMPORAL == 1
    assert ctypes.sizeof(spt.spt_temporal_params) == 24
    assert ctypes.sizeof(spt.spt_temporal_state) == 40
    assert ctypes.sizeof(spt.spt_temporal_info) == 24
    p = spt.default_temporal_params()
    assert (p.n_max, p.flags, p.reserved) == (32.0, 0, 0)
    assert [np.float32(v) for v in (p.normal_min, p.plane_tol, p.albedo_floor)] == \
        [np.float32(0.9), np.float32(0.01), np.float32(0.01)]
    assert spt.default_temporal_params(n_max=4).n_max == 4.0
    with pytest.raises(TypeError):
        spt.default_temporal_params(sigma=1)
    w, h = 5, 3
    cam = tt.camera(w, h)
    f = tt.frame(cam, w, h, 1, short_normals=False)
    r1 = spt.temporal_accumulate_host(*tt.planes_of(f), tt.to_struct(spt, cam))
    assert {k: r1["state"][k].shape for k in r1["state"]} == \
        {"c": (h, w, 3), "v": (h, w, 3), "n": (h, w), "X": (h, w, 3), "N": (h, w, 3)}
    # the state round-trips: copies of its planes give the same next frame as the planes themselves
    copy = {k: v.copy() for k, v in r1["state"].items()}
    r2 = spt.temporal_accumulate_host(*tt.planes_of(f), tt.to_struct(spt, cam), None, r1["state"],
                                      tt.to_struct(spt, cam))
    r2c = spt.temporal_accumulate_host(*tt.planes_of(f), tt.to_struct(spt, cam), None, copy, tt.to_struct(spt, cam))
    same(r2, r2c, "round trip")
    assert np.all(r2["n"][f["depth"] != 0] == 2)
    # a Camera is taken as well as an spt_camera
    c = spt.Camera(aspect=w / h)
    ra = spt.temporal_accumulate_host(*tt.planes_of(f), c)
    rb = spt.temporal_accumulate_host(*tt.planes_of(f), c._c)
    same(ra, rb, "Camera")


def test_refused_arguments(spt):
    w, h = 5, 3
    cam = tt.camera(w, h)
    f = tt.frame(cam, w, h, 1)
    cs = tt.to_struct(spt, cam)
    for kw in (dict(n_max=0.5), dict(n_max=float("nan")), dict(normal_min=2.0), dict(plane_tol=-1.0),
               dict(plane_tol=float("inf")), dict(albedo_floor=0.0), dict(flags=2), dict(reserved=1)):
        with pytest.raises(spt.SptError):
            spt.temporal_accumulate_host(*tt.planes_of(f), cs, spt.default_temporal_params(**kw))
    flat = cam.copy()
    flat[3] = flat[2]  # vertical parallel to horizontal: no volume
    with pytest.raises(spt.SptError):
        spt.temporal_accumulate_host(*tt.planes_of(f), tt.to_struct(spt, flat))
    r1 = spt.temporal_accumulate_host(*tt.planes_of(f), cs)
    with pytest.raises(spt.SptError):  # a state without its camera
        spt.temporal_accumulate_host(*tt.planes_of(f), cs, None, r1["state"], None)
    with pytest.raises(spt.SptError):  # a singular previous camera
        spt.temporal_accumulate_host(*tt.planes_of(f), cs, None, r1["state"], tt.to_struct(spt, flat))

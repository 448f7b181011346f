"""Progressive rendering on the GPU: sample windows added into a film reproduce the one-shot render
bit for bit -- for any split, order, chunk, kernel family, shard, launch shape, context -- and the
film's resolve, merge, checkpoint and rejections behave as include/spt.h states.

Every image comparison is bitwise (np.array_equal): the windows' samples are converted with the
one-shot's scale 2^31 / spp and summed in uint64, so there is nothing to tolerate."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "small-pathtracer_amd", "smallpt_amd")
INT_STATS = ["samples", "path_rays", "shadow_rays", "vertices", "nee_events", "nee_light_hits",
             "cosine_samples", "misses", "shadow_traced", "sphere_vertices", "shadow_proven"]
TILTED = dict(lookfrom=(40, 55, 160), lookat=(55, 35, 10), vup=(0.1, 1, 0))


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available()
    return torch


def numpy_resolve(sums, spp_total, samples_done):
    f = sums.astype(np.float32) * np.float32(2.0 ** -31)
    if samples_done == 0:
        return np.zeros(sums.shape, np.float32)
    if samples_done != spp_total:
        f = f * np.float32(np.float64(spp_total) / np.float64(samples_done))
    return np.minimum(f, np.float32(1.0)).astype(np.float32)


def film_passes(spt, prims, cam, p, windows):
    """Render the windows into a new film on a new context -> (film, renderer, per-pass stats,
    per-pass kernel names). The caller closes both."""
    r, film = spt.Renderer(p.device), spt.Film(p, p.device)
    stats, names = [], []
    for base, count in windows:
        film.render(r, prims, cam, p, base, count)
        stats.append(r.stats())
        names.append(r.kernel())
    return film, r, stats, names


def film_image(spt, prims, cam, p, windows):
    film, r, stats, names = film_passes(spt, prims, cam, p, windows)
    try:
        assert film.info()["samples_done"] == sum(c for _, c in windows)
        return film.resolve(), stats, names
    finally:
        film.close()
        r.close()


@pytest.fixture(scope="module")
def head(spt):
    """HEAD NEE at 64x48 @ 16, seed 1: scene, camera, params and the one-shot render with stats."""
    p = spt.default_params(width=64, height=48, spp=16, seed=1, device=0)
    cam = spt.Camera(aspect=64 / 48)
    prims = spt.cornell_scene()
    img, st = spt.render(prims, cam, p, return_stats=True)
    img.setflags(write=False)
    return prims, cam, p, img, st


def test_split_equals_one_shot_and_oracle(spt, oracle, head):
    prims, cam, p, one, st1 = head
    img, stats, names = film_image(spt, prims, cam, p, [(0, 5), (5, 11)])
    assert np.array_equal(img, one)
    cpu, _ = oracle.counter_render(prims, cam._c, p)
    assert np.array_equal(img, cpu)
    for k in INT_STATS:
        assert sum(s[k] for s in stats) == st1[k], k
    assert [s["samples"] for s in stats] == [64 * 48 * 5, 64 * 48 * 11]
    assert names == [st1["kernel"]] * 2


@pytest.mark.parametrize("windows,chunk", [
    ([(5, 11), (0, 5)], 0),                    # the same windows in reverse order
    ([(s, 1) for s in range(16)], 0),          # 16 windows of one sample
    ([(0, 6), (6, 10)], 4),                    # explicit chunk 4: a base that is no multiple of it
    ([(6, 10), (0, 6)], 4),
    ([(11, 5), (3, 8), (0, 3)], 3),            # ragged last chunks in every window
], ids=["reverse", "singles", "chunk4", "chunk4_reverse", "chunk3_ragged"])
def test_order_and_granularity(spt, head, windows, chunk):
    prims, cam, p, one, _ = head
    q = spt.spt_params.from_buffer_copy(p)
    q.chunk = chunk
    img, _, _ = film_image(spt, prims, cam, q, windows)
    assert np.array_equal(img, one)


def _family(spt, name):
    """-> (prims, camera kwargs, params kwargs) of one kernel family."""
    c = spt.cornell_scene
    return {
        "head_nee": lambda: (c(), {}, {}),
        "cosine": lambda: (c(), {}, dict(nee_prob=0.0)),
        "tilted": lambda: (c(), TILTED, {}),
        "move_short_box": lambda: (spt.move_short_box(c(), 1.0), {}, {}),
        "edit_light": lambda: (spt.edit_light(c(), x=(30, 66), z=(65, 99)), {}, {}),
        "edit_room": lambda: (spt.edit_room(c(), depth=150.0, width=(2.0, 98.0)), {}, {}),
        "reference_leaks": lambda: (c(), {}, dict(flags=spt.FLAG_REFERENCE_LEAKS)),
        "nee_half": lambda: (c(), {}, dict(nee_prob=0.5)),
        "spheres32": lambda: (spt.spheres32_scene(), {}, dict(max_depth=16)),
        "specular": lambda: (spt.cornell_specular_scene(), {}, dict(max_depth=16)),
        "uniform_scatter": lambda: (c(), {}, dict(flags=spt.FLAG_UNIFORM_SCATTER)),
    }[name]()


FAMILIES = ["head_nee", "cosine", "tilted", "move_short_box", "edit_light", "edit_room",
            "reference_leaks", "nee_half", "spheres32", "specular", "uniform_scatter"]


@pytest.mark.parametrize("name", FAMILIES)
def test_every_kernel_family(spt, name):
    """The window reaches every Topo x Cfg x CAMAX form of the render kernel, and does not change
    the dispatch."""
    prims, camkw, pkw = _family(spt, name)
    p = spt.default_params(width=32, height=24, spp=12, seed=7, device=0, **pkw)
    cam = spt.Camera(aspect=32 / 24, **camkw)
    one, st1 = spt.render(prims, cam, p, return_stats=True)
    img, stats, names = film_image(spt, prims, cam, p, [(0, 5), (5, 7)])
    assert np.array_equal(img, one)
    want = spt.select_kernel(prims, cam, p)["name"]
    assert names == [want, want] and st1["kernel"] == want
    for k in INT_STATS:
        assert stats[0][k] + stats[1][k] == st1[k], k


def test_families_reach_distinct_kernels(spt):
    """The family list is worth its name: it launches at least 9 different variants."""
    seen = set()
    for name in FAMILIES:
        prims, camkw, pkw = _family(spt, name)
        p = spt.default_params(width=32, height=24, spp=12, seed=7, **pkw)
        seen.add(spt.select_kernel(prims, spt.Camera(aspect=32 / 24, **camkw), p)["name"])
    assert len(seen) >= 9, seen


def test_shard_film_holds_the_compact_rows(spt):
    p = spt.default_params(width=64, height=48, spp=16, seed=1, device=0, tile_rows=8,
                           shard_index=1, shard_count=3)
    cam = spt.Camera(aspect=64 / 48)
    prims = spt.cornell_scene()
    one = spt.render(prims, cam, p)
    assert one.shape == (16, 64, 3)  # tiles 1 and 4 of six
    film, r, _, _ = film_passes(spt, prims, cam, p, [(0, 7), (7, 9)])
    try:
        assert film.info() == {"width": 64, "rows": 16, "spp_total": 16, "samples_done": 16}
        assert np.array_equal(film.resolve(), one)
    finally:
        film.close()
        r.close()


def test_odd_sizes_take_the_unaligned_paths(spt):
    """Pixel counts that are no multiple of 4, of 8 or of the block (the film kernels' scalar heads
    and tails, a pixel spread K < 8 with an odd run length), more than one block."""
    prims = spt.cornell_scene()
    for w, h in [(37, 11), (24, 3), (33, 28), (1, 1), (50, 27)]:
        p = spt.default_params(width=w, height=h, spp=6, seed=3, device=0)
        cam = spt.Camera(aspect=w / h)
        one = spt.render(prims, cam, p)
        img, _, _ = film_image(spt, prims, cam, p, [(4, 2), (0, 4)])
        assert np.array_equal(img, one), (w, h)


def test_short_and_long_launch_in_one_image(spt, torch_dev):
    """1024x768 @ 512 as 200 + 312: by the host's own rule (lane-iterations per resident lane below
    SPT_SMALL_ITERS = 2000 -> a short launch: other chunking, guided grabs, 4 blocks per CU) the
    first window is a short launch and the second a long one; together they are the one-shot."""
    w, h, spp = 1024, 768, 512
    n_cu = torch_dev.cuda.get_device_properties(0).multi_processor_count
    # plan_launch (spt_dispatch.cpp): pixels * samples * 5.3 rays per NEE sample / (CUs * 8 blocks * 256 lanes)
    iters = lambda count: w * h * count * 5.3 / (n_cu * 8 * 256)  # noqa: E731
    assert iters(200) < 2000.0 <= iters(312), (n_cu, iters(200), iters(312))
    p = spt.default_params(width=w, height=h, spp=spp, seed=1, device=0)
    cam = spt.Camera(aspect=w / h)
    prims = spt.cornell_scene()
    one = spt.render(prims, cam, p)
    img, stats, names = film_image(spt, prims, cam, p, [(0, 200), (200, 312)])
    assert names == ["const_nee", "const_nee"]
    assert [s["samples"] for s in stats] == [w * h * 200, w * h * 312]
    assert np.array_equal(img, one)
    # the film kernels at this size (thousands of blocks): the fused preview, the merge, the resolve
    torch = torch_dev
    buf = torch.empty(w * h * 3, dtype=torch.float32, device="cuda:0")
    a, ra = spt.Film(p, 0), spt.Renderer(0)
    b, rb, _, _ = film_passes(spt, prims, cam, p, [(0, 200)])
    try:
        a.render(ra, prims, cam, p, 200, 312, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy().reshape(h, w, 3), numpy_resolve(a.to_numpy(), 512, 312))
        a.merge(b)
        assert a.info()["samples_done"] == 512
        assert np.array_equal(a.resolve(), one)
    finally:
        a.close()
        b.close()
        ra.close()
        rb.close()


def test_preview_and_full_resolve(spt, head):
    prims, cam, p, one, _ = head
    film, r, _, _ = film_passes(spt, prims, cam, p, [(0, 5)])
    try:
        sums = film.to_numpy()
        assert sums.dtype == np.uint64 and sums.shape == (48, 64, 3) and sums.any()
        prev = film.resolve()
        assert np.array_equal(prev, numpy_resolve(sums, 16, 5))
        assert np.array_equal(prev, spt.film_resolve_host(sums, 64, 48, 16, 5))
        assert not np.array_equal(prev, one)
        film.render(r, prims, cam, p, 5, 11)
        assert np.array_equal(film.resolve(), one)
        assert np.array_equal(numpy_resolve(film.to_numpy(), 16, 16), one)
        film.clear()
        assert film.info()["samples_done"] == 0 and not film.to_numpy().any()
        assert not film.resolve().any()
    finally:
        film.close()
        r.close()


def test_merge_of_two_films(spt, head):
    prims, cam, p, one, _ = head
    a, ra, _, _ = film_passes(spt, prims, cam, p, [(0, 8)])
    b, rb, _, _ = film_passes(spt, prims, cam, p, [(8, 8)])
    try:
        sa, sb = a.to_numpy(), b.to_numpy()
        a.merge(b)
        assert a.info()["samples_done"] == 16 and b.info()["samples_done"] == 8
        assert np.array_equal(a.to_numpy(), sa + sb) and np.array_equal(b.to_numpy(), sb)
        assert np.array_equal(a.resolve(), one)
    finally:
        a.close()
        b.close()
        ra.close()
        rb.close()


def test_checkpoint_and_resume_on_a_new_context(spt, head, tmp_path):
    prims, cam, p, one, _ = head
    film, r, _, _ = film_passes(spt, prims, cam, p, [(0, 8)])
    path = str(tmp_path / "ck.film")
    film.save(path)
    film.close()
    r.close()
    sums, info = spt.read_film_file(path)
    assert info == {"width": 64, "rows": 48, "spp_total": 16, "samples_done": 8}
    r2, film2 = spt.Renderer(0), spt.Film(p, 0)
    try:
        film2.from_numpy(sums, info["samples_done"])
        film2.render(r2, prims, cam, p, 8, 8)
        assert film2.info()["samples_done"] == 16
        assert np.array_equal(film2.resolve(), one)
    finally:
        film2.close()
        r2.close()


def test_fused_output_equals_separate_resolve(spt, head, torch_dev):
    prims, cam, p, one, _ = head
    torch = torch_dev
    r, film = spt.Renderer(0), spt.Film(p, 0)
    try:
        buf = torch.full((48 * 64 * 3 + 1,), -1.0, dtype=torch.float32, device="cuda:0")
        stream = torch.cuda.current_stream().cuda_stream
        film.render(r, prims, cam, p, 0, 5, buf.data_ptr(), stream)  # a preview, fused
        torch.cuda.synchronize()
        fused = buf[:-1].cpu().numpy().reshape(48, 64, 3)
        assert np.array_equal(fused, film.resolve())
        assert float(buf[-1]) == -1.0
        # ... and into a buffer off the 16-byte grid, the full film
        film.render(r, prims, cam, p, 5, 11, buf.data_ptr() + 4, stream)
        torch.cuda.synchronize()
        assert np.array_equal(buf[1:].cpu().numpy().reshape(48, 64, 3), one)
        buf.fill_(-1.0)
        film.resolve(buf.data_ptr() + 4, stream)
        torch.cuda.synchronize()
        assert np.array_equal(buf[1:].cpu().numpy().reshape(48, 64, 3), one) and float(buf[0]) == -1.0
    finally:
        film.close()
        r.close()


def test_render_progressive(spt, head):
    prims, cam, p, one, st1 = head
    img, st = spt.render_progressive(prims, cam, p, 3, return_stats=True)
    assert np.array_equal(img, one)
    for k in INT_STATS:
        assert st[k] == st1[k], k
    assert np.array_equal(spt.render_progressive(prims, cam, p, [(10, 6), (0, 10)]), one)


def test_rejections_leave_the_film_untouched(spt, head):
    prims, cam, p, _, _ = head
    film, r, _, _ = film_passes(spt, prims, cam, p, [(0, 6)])
    other = spt.Film(spt.default_params(width=64, height=48, spp=12), 0)
    narrow = spt.Film(spt.default_params(width=32, height=48, spp=16), 0)
    try:
        before = film.to_numpy()

        def rejected(call):
            with pytest.raises(spt.SptError) as e:
                call()
            assert e.value.status == 1
            assert film.info()["samples_done"] == 6
            assert np.array_equal(film.to_numpy(), before)

        def with_p(**kw):
            q = spt.spt_params.from_buffer_copy(p)
            for k, v in kw.items():
                setattr(q, k, v)
            return q

        rejected(lambda: film.render(r, prims, cam, p, 10, 7))       # base + count > spp
        rejected(lambda: film.render(r, prims, cam, p, 6, 0))        # count = 0
        rejected(lambda: film.render(r, prims, cam, p, -1, 2))       # base < 0
        rejected(lambda: film.render(r, prims, cam, with_p(spp=12), 6, 2))
        rejected(lambda: film.render(r, prims, cam, with_p(width=32), 6, 2))
        rejected(lambda: film.render(r, prims, cam, with_p(height=24), 6, 2))
        rejected(lambda: film.render(r, prims, cam, with_p(shard_count=2), 6, 2))
        rejected(lambda: film.render(r, prims, cam, with_p(shard_count=2, shard_index=1), 6, 2))
        rejected(lambda: film.render(r, prims, cam, with_p(tile_rows=4), 6, 2))
        rejected(lambda: film.render(r, prims, cam, p, 0, 11))       # samples_done would overshoot
        rejected(lambda: film.merge(other))                          # unequal spp
        rejected(lambda: film.merge(narrow))                         # unequal width
        rejected(lambda: film.merge(film))
        rejected(lambda: film.from_numpy(before, 17))
        full, rf, _, _ = film_passes(spt, prims, cam, p, [(0, 11)])
        try:
            rejected(lambda: film.merge(full))                       # 6 + 11 > 16
        finally:
            full.close()
            rf.close()
        # the film still works: the remaining samples complete it
        film.render(r, prims, cam, p, 6, 10)
        assert film.info()["samples_done"] == 16
    finally:
        film.close()
        other.close()
        narrow.close()
        r.close()


def _prog(tmp_path, *args):
    r = subprocess.run([PROG, *[str(a) for a in args]], capture_output=True, text=True, timeout=120,
                       cwd=tmp_path)
    return r.returncode, r.stdout + r.stderr


def test_smallpt_amd_passes_and_film(tmp_path):
    rc, out = _prog(tmp_path, 64, 48, 16, 1, "b.ppm")
    assert rc == 0, out[-2000:]
    plain = (tmp_path / "b.ppm").read_bytes()
    rc, out = _prog(tmp_path, 64, 48, 16, 1, "a.ppm", "--passes", 3)
    assert rc == 0 and "DURATION" in out, out[-2000:]
    assert (tmp_path / "a.ppm").read_bytes() == plain
    # two runs of 8 samples through a film file, then a third against the full film
    rc, out = _prog(tmp_path, 64, 48, 16, 1, "f1.ppm", "--film", "f.bin", "--add", 8)
    assert rc == 0 and "FILM : 8 / 16" in out, out[-2000:]
    assert (tmp_path / "f1.ppm").read_bytes() != plain  # a preview
    half = (tmp_path / "f.bin").read_bytes()
    assert half[:8] == b"SPTFILM1" and len(half) == 32 + 64 * 48 * 3 * 8
    rc, out = _prog(tmp_path, 64, 48, 16, 1, "f2.ppm", "--film", "f.bin", "--add", 8)
    assert rc == 0 and "FILM : 16 / 16" in out, out[-2000:]
    assert (tmp_path / "f2.ppm").read_bytes() == plain
    full = (tmp_path / "f.bin").read_bytes()
    rc, out = _prog(tmp_path, 64, 48, 16, 1, "f3.ppm", "--film", "f.bin", "--add", 8)
    assert rc == 1 and "film is full" in out, out[-2000:]
    assert not (tmp_path / "f3.ppm").exists() and (tmp_path / "f.bin").read_bytes() == full
    # a film of another size is refused
    rc, out = _prog(tmp_path, 32, 48, 16, 1, "f4.ppm", "--film", "f.bin")
    assert rc == 1 and "not W H SPP" in out, out[-2000:]

"""The noise-aware film on the GPU: the moment plane M2 is the exact sum of the squared batch sums,
whatever the order, size, shard or kernel family; its carries; the error map and the image figures
against their host statements; the calibration of the RMSE estimate; render_until; the rejections;
smallpt_amd --noise.

M2 comparisons are exact (Python integers or a 128-bit restatement in uint64 pairs). The map and the
summary are compared with the tolerances of tests/test_film_noise.py."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "small-pathtracer_amd", "smallpt_amd")
REL_F32 = 2.0 ** -21
REL_SUM = 1e-9
MASK32 = np.uint64(0xFFFFFFFF)


def m2_ints(m2):
    """(…, 2) uint64 pairs (lo, hi) -> Python integers (object array)."""
    return m2[..., 0].astype(object) + m2[..., 1].astype(object) * (1 << 64)


def square128(p):
    """uint64 p < 2^63 -> (lo, hi) of p^2 as uint64 arrays (numpy wraps modulo 2^64)."""
    a, b = p >> np.uint64(32), p & MASK32
    bb, ab = b * b, a * b                      # b^2 < 2^64; a b < 2^63
    cross_lo, cross_hi = ab << np.uint64(33), ab >> np.uint64(31)  # 2 a b 2^32
    lo = bb + cross_lo
    hi = a * a + cross_hi + (lo < bb).astype(np.uint64)
    return lo, hi


def add128(lo, hi, lo2, hi2):
    s = lo + lo2
    return s, hi + hi2 + (s < lo2).astype(np.uint64)


def window_sums(spt, prims, cam, p, base, count):
    """The window alone in a plain film -> its sums (rows, w, 3) uint64."""
    r, film = spt.Renderer(p.device), spt.Film(p, p.device)
    try:
        film.render(r, prims, cam, p, base, count)
        r.stats()
        return film.to_numpy()
    finally:
        film.close()
        r.close()


def noise_film(spt, prims, cam, p, batch, order):
    """Batches `order` (indices) into a new noise film -> (film, renderer); the caller closes both."""
    r, film = spt.Renderer(p.device), spt.Film(p, p.device)
    film.enable_noise(batch)
    for k in order:
        film.render(r, prims, cam, p, k * batch, batch)
        r.stats()
    return film, r


def check_moments(spt, prims, cam, p, batch, orders):
    """M2 == sum of S_k^2 exactly, the sums == the plain film's, the resolve == the one-shot render."""
    nb = p.spp // batch
    S = [window_sums(spt, prims, cam, p, k * batch, batch) for k in range(nb)]
    want_m2 = sum(s.astype(object) ** 2 for s in S)
    want_sums = sum(S[1:], S[0].copy())
    one = spt.render(prims, cam, p)
    for order in orders:
        film, r = noise_film(spt, prims, cam, p, batch, order)
        try:
            assert film.noise_info() == {"enabled": 1, "batch": batch, "batches_done": nb}
            assert film.info()["samples_done"] == p.spp
            m2 = film.noise_to_numpy()
            assert m2.shape == S[0].shape + (2,)
            assert np.array_equal(m2_ints(m2), want_m2), order
            assert np.array_equal(film.to_numpy(), want_sums), order
            assert np.array_equal(film.resolve(), one), order
        finally:
            film.close()
            r.close()
    return S


@pytest.fixture(scope="module")
def head(spt):
    """HEAD NEE at 64x48 @ 16, seed 1: scene, camera, params and the one-shot render."""
    p = spt.default_params(width=64, height=48, spp=16, seed=1, device=0)
    cam = spt.Camera(aspect=64 / 48)
    prims = spt.cornell_scene()
    img = spt.render(prims, cam, p)
    img.setflags(write=False)
    return prims, cam, p, img


def test_exact_moments_in_any_order(spt, head):
    prims, cam, p, _ = head
    S = check_moments(spt, prims, cam, p, 4, [[0, 1, 2, 3], [2, 0, 3, 1]])
    assert any(int(s.max()) ** 2 >= 1 << 64 for s in S)  # the hi word is in use (the light's pixels)
    # the numpy 128-bit restatement (used at 1024x768 below) is the Python-integer one
    lo, hi = square128(S[0])
    assert np.array_equal(m2_ints(np.stack([lo, hi], axis=-1)), S[0].astype(object) ** 2)
    # clear takes the moments and the batch count along
    film, r = noise_film(spt, prims, cam, p, 4, [0, 1])
    try:
        assert film.noise_to_numpy().any()
        film.clear()
        assert film.noise_info() == {"enabled": 1, "batch": 4, "batches_done": 0}
        assert film.info()["samples_done"] == 0
        assert not film.noise_to_numpy().any() and not film.to_numpy().any()
    finally:
        film.close()
        r.close()


@pytest.mark.parametrize("w,h", [(37, 11), (24, 3), (33, 28), (1, 1), (50, 27)])
def test_odd_sizes_take_the_unaligned_paths(spt, w, h):
    p = spt.default_params(width=w, height=h, spp=6, seed=3, device=0)
    check_moments(spt, spt.cornell_scene(), spt.Camera(aspect=w / h), p, 2, [[0, 1, 2], [2, 0, 1]])


def test_shard_film(spt):
    p = spt.default_params(width=64, height=48, spp=6, seed=1, device=0, tile_rows=8, shard_index=1,
                           shard_count=3)
    S = check_moments(spt, spt.cornell_scene(), spt.Camera(aspect=64 / 48), p, 2, [[1, 2, 0]])
    assert S[0].shape == (16, 64, 3)


@pytest.mark.parametrize("name", ["cosine", "specular"])
def test_other_kernel_families(spt, name):
    prims, pkw = {"cosine": (spt.cornell_scene(), dict(nee_prob=0.0)),
                  "specular": (spt.cornell_specular_scene(), dict(max_depth=16))}[name]
    p = spt.default_params(width=32, height=24, spp=12, seed=7, device=0, **pkw)
    cam = spt.Camera(aspect=32 / 24)
    if name == "specular":
        assert spt.select_kernel(prims, cam, p)["name"] == "generic"
    check_moments(spt, prims, cam, p, 4, [[0, 1, 2]])


def test_carries_through_merge_and_pass(spt):
    """lo words at 2^64 - 1: the merge's and the accumulate's carries reach the hi words. Whatever
    the scene renders, the expected value is built from the film's own downloads."""
    w, h, batch = 37, 11, 4
    p = spt.default_params(width=w, height=h, spp=16, seed=2, device=0)
    cam, prims = spt.Camera(aspect=w / h), spt.cornell_scene()
    top = np.uint64(2 ** 64 - 1)
    n = h * w * 3
    a_m2 = np.empty((h, w, 3, 2), np.uint64)
    a_m2[..., 0], a_m2[..., 1] = top, 5
    b_m2 = np.empty((h, w, 3, 2), np.uint64)
    b_m2[..., 0] = np.where(np.arange(n).reshape(h, w, 3) % 3 == 0, top, np.uint64(1))
    b_m2[..., 1] = np.arange(n, dtype=np.uint64).reshape(h, w, 3) * np.uint64(2 ** 40)
    zeros = np.zeros((h, w, 3), np.uint64)
    a, b, r = spt.Film(p, 0), spt.Film(p, 0), spt.Renderer(0)
    try:
        for film, m2 in ((a, a_m2), (b, b_m2)):
            film.enable_noise(batch)
            film.from_numpy(zeros, batch)
            film.noise_from_numpy(m2, 1)
            assert np.array_equal(film.noise_to_numpy(), m2)
        a.merge(b)
        merged = m2_ints(a_m2) + m2_ints(b_m2)
        assert np.array_equal(m2_ints(a.noise_to_numpy()), merged)
        assert np.array_equal(b.noise_to_numpy(), b_m2)
        assert a.noise_info()["batches_done"] == 2 and a.info()["samples_done"] == 8
        a.render(r, prims, cam, p, 8, batch)
        r.stats()
        P = a.to_numpy().astype(object)  # the film held zeros: its sums are the pass's
        assert P.any()
        got = m2_ints(a.noise_to_numpy())
        assert np.array_equal(got, merged + P ** 2)
        assert np.array_equal(a.noise_to_numpy()[..., 1].astype(object), (merged + P ** 2) >> 64)
        assert a.noise_info()["batches_done"] == 3
    finally:
        a.close()
        b.close()
        r.close()


def test_moments_at_1024x768(spt):
    """The size at which the resolve kernel's load/wait problem showed: after every pass M2 is the
    running sum of (film after - film before)^2, from downloads."""
    w, h, batch = 1024, 768, 4
    p = spt.default_params(width=w, height=h, spp=16, seed=1, device=0)
    cam, prims = spt.Camera(aspect=w / h), spt.cornell_scene()
    r, film = spt.Renderer(0), spt.Film(p, 0)
    try:
        film.enable_noise(batch)
        before = film.to_numpy()
        lo, hi = np.zeros_like(before), np.zeros_like(before)
        for k in range(4):
            film.render(r, prims, cam, p, k * batch, batch)
            r.stats()
            after = film.to_numpy()
            lo, hi = add128(lo, hi, *square128(after - before))
            m2 = film.noise_to_numpy()
            bad = (m2[..., 0] != lo) | (m2[..., 1] != hi)
            assert not bad.any(), (k, int(bad.sum()), np.argwhere(bad)[:4].tolist())
            before = after
        assert hi.any()
        assert np.array_equal(film.resolve(), spt.render(prims, cam, p))
    finally:
        film.close()
        r.close()


def _close(got, want, rel):
    return abs(got - want) <= rel * abs(want)


@pytest.mark.parametrize("batches", [4, 2], ids=["full", "preview"])
def test_map_and_summary_match_the_host_statements(spt, head, batches):
    prims, cam, p, _ = head
    film, r = noise_film(spt, prims, cam, p, 4, range(batches))
    try:
        sums, m2 = film.to_numpy(), film.noise_to_numpy()
        done = 4 * batches
        args = (sums, m2, 64, 48, 16, done, 4, batches)
        se = film.noise_map()
        want = spt.film_noise_map_host(*args)
        assert se.dtype == np.float32 and se.shape == (48, 64, 3)
        assert np.array_equal(se == 0, want == 0)
        assert np.all(np.abs(se.astype(np.float64) - want) <= REL_F32 * want)
        assert (se > 0).any()
        s1, s2 = film.noise_summary(), film.noise_summary()
        assert s1 == s2  # Python floats compare by value: the same bits
        hs = spt.film_noise_summary_host(*args)
        for c in range(3):
            assert _close(s1["rmse"][c], hs["rmse"][c], REL_SUM), (c, s1, hs)
        assert _close(s1["rmse_all"], hs["rmse_all"], REL_SUM)
        assert _close(s1["se_max"], hs["se_max"], REL_F32) and s1["se_max"] == float(se.max())
        assert s1["clamped"] == hs["clamped"] and s1["batches_done"] == batches
        # the light's pixels: resolved to the clamp, no error by rule, counted
        res = film.resolve()
        light = res == np.float32(1.0)
        assert light.all(axis=-1).any(), "the light is in view"
        assert not se[light].any()
        assert s1["clamped"] == int(light.sum()) > 0
        # an error map into a caller's device buffer, enqueued
        import torch
        buf = torch.full((48 * 64 * 3 + 1,), -1.0, dtype=torch.float32, device="cuda:0")
        film.noise_map(buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(buf[:-1].cpu().numpy().reshape(48, 64, 3), se) and float(buf[-1]) == -1.0
    finally:
        film.close()
        r.close()


def test_calibration_against_a_converged_render(spt):
    """The estimate sqrt(mean SE^2) against the actual RMSE to a one-shot 8192-spp render of another
    seed, the truth's own noise taken out by sqrt(1 + 256 / 8192). The light's emission is divided
    by 16 so that no channel is clamped. The CPU oracle gave 0.965-1.03 for this construction; the
    band [0.90, 1.10] is about three times that spread. Measured on an MI355X: see DESIGN.md §3."""
    prims = [spt.spt_prim.from_buffer_copy(q) for q in spt.cornell_scene()]
    for i in range(3):
        prims[6].e[i] /= 16.0
    cam = spt.Camera(aspect=64 / 48)
    p = spt.default_params(width=64, height=48, spp=256, seed=1, device=0)
    truth = spt.render(prims, cam, spt.default_params(width=64, height=48, spp=8192, seed=999,
                                                      device=0)).astype(np.float64)
    film, r = noise_film(spt, prims, cam, p, 16, range(16))
    try:
        img = film.resolve().astype(np.float64)
        s = film.noise_summary()
    finally:
        film.close()
        r.close()
    actual = np.sqrt(((img - truth) ** 2).mean(axis=(0, 1)))
    ratios = [float(actual[c] / (s["rmse"][c] * np.sqrt(1.0 + 256.0 / 8192.0))) for c in range(3)]
    print("calibration ratios (actual / estimate):", ratios, "estimate:", s["rmse"])
    assert s["clamped"] == 0
    for c in range(3):
        assert 0.90 <= ratios[c] <= 1.10, ratios


def test_render_until(spt, head):
    prims, cam, p, one = head
    img, info = spt.render_until(prims, cam, p, 0.0, return_info=True)  # batch = 16 / 8
    assert np.array_equal(img, one)
    assert info["samples_done"] == 16 and info["batches_done"] == 8 and max(info["rmse"]) > 0
    img, info = spt.render_until(prims, cam, p, 1e9, batch=4, return_info=True)
    assert info["samples_done"] == 8 and info["batches_done"] == 2
    r, film = spt.Renderer(0), spt.Film(p, 0)
    try:
        film.render(r, prims, cam, p, 0, 4)
        film.render(r, prims, cam, p, 4, 4)
        assert np.array_equal(img, film.resolve())
    finally:
        film.close()
        r.close()
    assert not np.array_equal(img, one)
    again, info2 = spt.render_until(prims, cam, p, 1e9, batch=4, return_info=True)
    assert np.array_equal(again, img) and info2 == info
    img3, info3 = spt.render_until(prims, cam, p, 1e9, batch=2, min_batches=3, return_info=True)
    assert info3["samples_done"] == 6 and info3["batches_done"] == 3
    with pytest.raises(ValueError):
        spt.render_until(prims, cam, spt.default_params(width=64, height=48, spp=12, device=0), 0.1)


def test_rejections_leave_sums_moments_and_counts_untouched(spt, head):
    prims, cam, p, _ = head
    film, r = noise_film(spt, prims, cam, p, 4, [0])
    plain, rp = spt.Film(p, 0), spt.Renderer(0)
    other = spt.Film(p, 0)
    empty = spt.Film(p, 0)
    try:
        plain.render(rp, prims, cam, p, 4, 4)
        rp.stats()
        other.enable_noise(2)
        state = lambda f: (f.info(), f.noise_info(), f.to_numpy(),  # noqa: E731
                           f.noise_to_numpy() if f.noise_info()["enabled"] else None)

        def rejected(call, *films):
            before = [state(f) for f in films]
            with pytest.raises(spt.SptError) as e:
                call()
            assert e.value.status == 1
            for f, b in zip(films, before):
                a = state(f)
                assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])
                assert (a[3] is None and b[3] is None) or np.array_equal(a[3], b[3])

        rejected(lambda: plain.enable_noise(4), plain)               # a film that holds samples
        assert plain.noise_info() == {"enabled": 0, "batch": 0, "batches_done": 0}
        for bad in (0, -4, 5, 16, 32):                               # 16: one batch only
            rejected(lambda: empty.enable_noise(bad), empty)
        assert empty.noise_info()["enabled"] == 0
        rejected(lambda: film.enable_noise(4), film)                 # twice
        rejected(lambda: film.render(r, prims, cam, p, 4, 2), film)  # not a whole batch
        rejected(lambda: film.render(r, prims, cam, p, 4, 8), film)
        rejected(lambda: film.render(r, prims, cam, p, 2, 4), film)  # a base off the batch grid
        rejected(lambda: film.merge(plain), film, plain)             # mixed, both ways
        rejected(lambda: plain.merge(film), film, plain)
        rejected(lambda: film.merge(other), film, other)             # unequal batch
        rejected(lambda: film.noise_map(), film)                     # one batch: no error yet
        rejected(lambda: film.noise_summary(), film)
        rejected(lambda: film.from_numpy(film.to_numpy(), 6), film)  # no whole batches
        rejected(lambda: film.noise_from_numpy(film.noise_to_numpy(), 5), film)
        rejected(lambda: plain.noise_to_numpy(), plain)
        rejected(lambda: plain.noise_map(), plain)
        rejected(lambda: plain.noise_summary(), plain)
        # both films still work
        film.render(r, prims, cam, p, 4, 4)
        assert film.noise_info()["batches_done"] == 2 and film.noise_summary()["batches_done"] == 2
        plain.render(rp, prims, cam, p, 0, 3)
        assert plain.info()["samples_done"] == 7
    finally:
        for f in (film, plain, other, empty):
            f.close()
        r.close()
        rp.close()


def _prog(tmp_path, *args):
    r = subprocess.run([PROG, *[str(a) for a in args]], capture_output=True, text=True, timeout=120,
                       cwd=tmp_path)
    return r.returncode, r.stdout + r.stderr


def test_smallpt_amd_noise(spt, tmp_path):
    rc, out = _prog(tmp_path, 64, 48, 64, 1, "out.ppm", "--noise", "1e9", "--batch", 8)
    assert rc == 0, out[-2000:]
    line = [ln for ln in out.splitlines() if ln.startswith("NOISE : ")]
    assert len(line) == 1 and line[0].endswith(" after 16 / 64"), out[-2000:]
    assert all(float(x) > 0 for x in line[0].split()[2:5])
    rc, out = _prog(tmp_path, 64, 48, 64, 1, "plain.ppm")
    assert rc == 0, out[-2000:]
    rc, out = _prog(tmp_path, 64, 48, 64, 1, "full.ppm", "--noise", 0)
    assert rc == 0 and " after 64 / 64" in out, out[-2000:]
    assert (tmp_path / "full.ppm").read_bytes() == (tmp_path / "plain.ppm").read_bytes()
    assert (tmp_path / "out.ppm").read_bytes() != (tmp_path / "plain.ppm").read_bytes()
    # with a checkpoint: a noise film's file, resumed by a second run
    rc, out = _prog(tmp_path, 64, 48, 64, 1, "f1.ppm", "--noise", "1e9", "--batch", 8, "--film", "f.bin")
    assert rc == 0 and " after 16 / 64" in out and "FILM : 16 / 64" in out, out[-2000:]
    assert (tmp_path / "f1.ppm").read_bytes() == (tmp_path / "out.ppm").read_bytes()
    data = (tmp_path / "f.bin").read_bytes()
    assert data[:8] == b"SPTFILM2" and len(data) == 48 + 72 * 64 * 48
    rc, out = _prog(tmp_path, 64, 48, 64, 1, "f2.ppm", "--noise", "1e9", "--batch", 8, "--film", "f.bin")
    assert rc == 0 and " after 24 / 64" in out, out[-2000:]
    sums, m2, info = spt.read_film_file(str(tmp_path / "f.bin"), with_noise=True)
    assert info == {"width": 64, "rows": 48, "spp_total": 64, "samples_done": 24, "batch": 8,
                    "batches_done": 3}
    assert m2.any() and sums.any()
    # a plain run refuses the noise film, and the other way round
    rc, out = _prog(tmp_path, 64, 48, 64, 1, "f3.ppm", "--film", "f.bin")
    assert rc == 1 and "noise film" in out, out[-2000:]
    rc, out = _prog(tmp_path, 64, 48, 64, 1, "f4.ppm", "--noise", "1e9", "--batch", 16, "--film", "f.bin")
    assert rc == 1 and "another --batch" in out, out[-2000:]

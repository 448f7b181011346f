"""The pooled error on the GPU: spt_film_noise_pool_map and spt_film_adaptive_select_pooled against
their host statements (spt_film_host.cpp, themselves compared with Python floats in
tests/test_film_pool.py).

Every film here is the HEAD scene (NEE) at 64 spp in batches of 8. Keep masks leave retired pixels at
2, 3 and 4 batches, the rest is active at the front, 5; the planes are downloaded once per shape and
the device film is set back to them (a checkpoint upload) before every call under test. The selection
(counts plane, n_active, and the list through the next pass's statistics and sums) equals the host
statement's exactly; the map lies within relative 2^-21 of it (one float rounding and the square
root; the tolerance of tests/test_film_noise.py for the same kind of quantity) and is 0 exactly where
the statement is. Thresholds: the median over the active pixels of the host's pooled se, at which the
host statement alone retires 20-80 % -- except where every active pixel has the same window (a 1x1
film; 5x3 at R = 16 with the centre in), where no threshold can split them.
Shapes: 70x11 (a row wider than a wave, no multiple of the tile, fewer rows than a window at R = 16),
300x5 (several blocks per row: halos cross block edges), 5x3, 1x1, and shard 1 of 3 of a 70x40 image
in tiles of 8 rows (16 compact rows, two bands: no window crosses compact row 8).
Every test needs symbols the parent commit does not have."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "small-pathtracer_amd", "smallpt_amd")
REL_F32 = 2.0 ** -21
RETIRED, MASK = np.uint32(0x80000000), np.uint32(0x7FFFFFFF)
SPP, BATCH, FRONT = 64, 8, 5
SHAPES = {"70x11": dict(width=70, height=11), "300x5": dict(width=300, height=5),
          "5x3": dict(width=5, height=3), "1x1": dict(width=1, height=1),
          "shard": dict(width=70, height=40, tile_rows=8, shard_index=1, shard_count=3)}
RADII = (1, 2, 16)


def uniform_reference(spt, prims, cam, p, batch, upto):
    """One uniform noise film filled in order -> U[b] = (sums, m2) after b batches, b = 0..upto."""
    r, film = spt.Renderer(p.device), spt.Film(p, p.device)
    try:
        film.enable_noise(batch)
        U = [(film.to_numpy(), film.noise_to_numpy())]
        for k in range(upto):
            film.render(r, prims, cam, p, k * batch, batch)
            r.stats()
            U.append((film.to_numpy(), film.noise_to_numpy()))
    finally:
        film.close()
        r.close()
    for s, m in U:
        s.setflags(write=False)
        m.setflags(write=False)
    return U


def planes_at(U, batches):
    """The sums and moments of a film whose pixel p holds batches[p] batches."""
    S = np.stack([u[0] for u in U])
    M = np.stack([u[1] for u in U])
    b = batches.astype(np.int64)
    return (np.take_along_axis(S, b[None, :, :, None], axis=0)[0],
            np.take_along_axis(M, b[None, :, :, None, None], axis=0)[0])


class Case:
    """One shape: the scene, the uniform reference U[0..6], an adaptive film with retired pixels at 2,
    3 and 4 batches and the front at 5, and its planes on the host."""

    def __init__(self, spt, name):
        kw = SHAPES[name]
        self.spt, self.name = spt, name
        self.p = spt.default_params(spp=SPP, seed=1, device=0, **kw)
        self.w = kw["width"]
        self.band = kw.get("tile_rows", 0)
        self.prims, self.cam = spt.cornell_scene(), spt.Camera(aspect=kw["width"] / kw["height"])
        self.U = uniform_reference(spt, self.prims, self.cam, self.p, BATCH, FRONT + 1)
        self.rows = self.U[0][0].shape[0]
        self.r, self.film = spt.Renderer(0), spt.Film(self.p, 0)
        self.film.enable_noise(BATCH)
        self.film.enable_adaptive()
        idx = np.arange(self.rows * self.w).reshape(self.rows, self.w)
        for k in range(FRONT):
            if k >= 2:  # before pass 3, 4, 5: the pixels with index % 7 == 1, 3, 5 retire at 2, 3, 4
                self.film.adaptive_select(-1.0, (idx % 7 != 2 * k - 3).astype(np.uint8))
            self.film.render(self.r, self.prims, self.cam, self.p, k * BATCH, BATCH)
            self.r.stats()
        self.sums, self.m2 = self.film.to_numpy(), self.film.noise_to_numpy()
        self.counts = self.film.counts_to_numpy()
        for a in (self.sums, self.m2, self.counts):
            a.setflags(write=False)
        self.active = (self.counts & RETIRED) == 0
        want = np.full((self.rows, self.w), FRONT, np.uint32)
        for k, b in ((1, 2), (3, 3), (5, 4)):
            want[idx % 7 == k] = np.uint32(b) | RETIRED
        assert np.array_equal(self.counts, want)
        s, m = planes_at(self.U, self.counts & MASK)
        assert np.array_equal(self.sums, s) and np.array_equal(self.m2, m)

    def restore(self):
        """The film back at the downloaded planes: a checkpoint's three uploads, the counts last."""
        self.film.from_numpy(self.sums, FRONT * BATCH)
        self.film.noise_from_numpy(self.m2, FRONT)
        self.film.counts_from_numpy(self.counts)
        assert self.film.adaptive_info()["n_active"] == int(self.active.sum())

    def host_map(self, R, loo):
        return self.spt.film_noise_pool_map_host(self.sums, self.m2, self.counts, self.w, self.rows, SPP,
                                                 BATCH, FRONT, R, loo, self.band)

    def host_select(self, thr, R, loo, keep=None):
        return self.spt.film_adaptive_select_pooled_host(self.sums, self.m2, self.counts, self.w, self.rows,
                                                         SPP, BATCH, FRONT, thr, R, loo, keep, self.band)

    def median_threshold(self, R, loo):
        """The CPU file's rule: the median over the active pixels of the host's pooled se, at which
        the host statement alone retires 20-80 % of them (where the windows differ at all)."""
        se = self.host_map(R, loo).max(axis=-1)[self.active]
        thr = float(np.sort(se)[se.size // 2])
        _, lst = self.host_select(thr, R, loo)
        gone = se.size - lst.size
        one_window = se.size == 1 or (not loo and self.w <= R + 1 and self.rows <= R + 1)
        print(f"{self.name} R={R} loo={loo}: threshold {thr:.6g}, {gone} of {se.size} active retire")
        if one_window:
            assert gone in (0, se.size)
        else:
            assert 0.2 * se.size <= gone <= 0.8 * se.size, (gone, se.size)
        return thr

    def close(self):
        self.film.close()
        self.r.close()


@pytest.fixture(scope="module")
def cases(spt):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(spt, name)
        return made[name]

    yield get
    for c in made.values():
        c.close()


def close_to(got, want):
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.array_equal(got == 0, want == 0)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print("largest relative error", float((err / np.where(want == 0, 1, want)).max()))
    assert np.all(err <= REL_F32 * want)


@pytest.mark.parametrize("loo", [False, True])
@pytest.mark.parametrize("R", RADII)
@pytest.mark.parametrize("name", list(SHAPES))
def test_pooled_selection_is_the_host_statement(spt, cases, name, R, loo):
    c = cases(name)
    thr = c.median_threshold(R, loo)
    want_c, want_l = c.host_select(thr, R, loo)
    got = []
    for _ in range(2):  # the same call on equal films: equal bits
        c.restore()
        n = c.film.adaptive_select(thr, None, 0, R, loo)
        got.append((n, c.film.counts_to_numpy()))
        assert c.film.adaptive_info()["n_active"] == n
        assert c.film.adaptive_info()["front"] == FRONT
    assert got[0][0] == got[1][0] == want_l.size
    assert np.array_equal(got[0][1], want_c) and np.array_equal(got[1][1], want_c)
    # the selection changed no sample
    assert np.array_equal(c.film.to_numpy(), c.sums) and np.array_equal(c.film.noise_to_numpy(), c.m2)


@pytest.mark.parametrize("name", list(SHAPES))
def test_keep_mask_and_no_threshold(spt, cases, name):
    c = cases(name)
    keep = (np.random.default_rng(5).random((c.rows, c.w)) < 0.7).astype(np.uint8)
    thr = c.median_threshold(2, True)
    for t in (thr, -1.0):
        want_c, want_l = c.host_select(t, 2, True, keep)
        c.restore()
        assert c.film.adaptive_select(t, keep, 0, 2, True) == want_l.size
        assert np.array_equal(c.film.counts_to_numpy(), want_c)
    c.restore()  # threshold < 0 without a mask: nothing retires
    assert c.film.adaptive_select(-1.0, None, 0, 2, False) == int(c.active.sum())
    assert np.array_equal(c.film.counts_to_numpy(), c.counts)


@pytest.mark.parametrize("loo", [False, True])
@pytest.mark.parametrize("R", RADII)
@pytest.mark.parametrize("name", list(SHAPES))
def test_pool_map_on_an_adaptive_film(spt, cases, name, R, loo):
    c = cases(name)
    c.restore()
    a, b = c.film.noise_pool_map(R, loo), c.film.noise_pool_map(R, loo)
    assert a.tobytes() == b.tobytes()
    close_to(a, c.host_map(R, loo))
    if name != "1x1":
        assert np.count_nonzero(a) > a.size // 2
    assert np.array_equal(c.film.counts_to_numpy(), c.counts)  # a map marks nothing


@pytest.mark.parametrize("R,loo", [(1, False), (2, True), (16, False), (16, True)])
@pytest.mark.parametrize("name", list(SHAPES))
def test_pool_map_on_a_uniform_noise_film(spt, cases, name, R, loo):
    c = cases(name)
    film = spt.Film(c.p, 0)
    try:
        film.enable_noise(BATCH)
        film.from_numpy(c.U[3][0], 3 * BATCH)
        film.noise_from_numpy(c.U[3][1], 3)
        a, b = film.noise_pool_map(R, loo), film.noise_pool_map(R, loo)
        assert a.tobytes() == b.tobytes()
        close_to(a, spt.film_noise_pool_map_host(c.U[3][0], c.U[3][1], None, c.w, c.rows, SPP, BATCH, 3, R,
                                                 loo, c.band))
    finally:
        film.close()


@pytest.mark.parametrize("name", list(SHAPES))
def test_pass_after_a_pooled_selection_keeps_the_invariant(spt, cases, name):
    """Every pixel holds a uniform noise film's sums and moments at its own count, bit for bit; the
    pass renders the selection's list (its statistics count the list's pixels)."""
    c = cases(name)
    thr = c.median_threshold(2, True)
    want_c, want_l = c.host_select(thr, 2, True)
    c.restore()
    n = c.film.adaptive_select(thr, None, 0, 2, True)
    assert n == want_l.size
    before = c.film.adaptive_info()
    if n == 0:  # the one-pixel film: nothing left to render
        with pytest.raises(spt.SptError) as e:
            c.film.render(c.r, c.prims, c.cam, c.p, FRONT * BATCH, BATCH)
        assert e.value.status == 1
        return
    c.film.render(c.r, c.prims, c.cam, c.p, FRONT * BATCH, BATCH)
    assert c.r.stats()["samples"] == n * BATCH
    a = c.film.adaptive_info()
    assert a["front"] == FRONT + 1 and a["n_active"] == n
    assert a["samples_total"] == before["samples_total"] + n * BATCH
    stay = (want_c & RETIRED) == 0
    assert int(stay.sum()) == n
    counts = np.where(stay, np.uint32(FRONT + 1), want_c)
    assert np.array_equal(c.film.counts_to_numpy(), counts)
    s, m = planes_at(c.U, counts & MASK)
    assert np.array_equal(c.film.to_numpy(), s) and np.array_equal(c.film.noise_to_numpy(), m)
    assert np.array_equal(c.film.resolve(),
                          spt.film_adaptive_resolve_host(s, counts, c.w, c.rows, SPP, BATCH))


def test_rejections_leave_the_film_unchanged(spt, cases):
    c = cases("70x11")
    c.restore()
    plain, noise, young = spt.Film(c.p, 0), spt.Film(c.p, 0), spt.Film(c.p, 0)
    empty_p = spt.default_params(width=70, height=8, spp=SPP, seed=1, device=0, tile_rows=8, shard_index=1,
                                 shard_count=3)
    empty = spt.Film(empty_p, 0)
    try:
        def rejected(call, film):
            info, a = film.info(), film.adaptive_info()
            cnt = film.counts_to_numpy() if a["enabled"] else None
            with pytest.raises(spt.SptError) as e:
                call()
            assert e.value.status == 1
            assert film.info() == info and film.adaptive_info() == a
            if cnt is not None:
                assert np.array_equal(film.counts_to_numpy(), cnt)

        for R in (-1, 17, 1 << 20):
            rejected(lambda: c.film.adaptive_select(0.01, None, 0, R, False), c.film)
            rejected(lambda: c.film.noise_pool_map(R), c.film)
        rejected(lambda: c.film.noise_pool_map(0), c.film)
        rejected(lambda: c.film.adaptive_select(float("nan"), None, 0, 2, True), c.film)
        lib, n = spt.load_library(), ctypes.c_int64(-3)
        assert lib.spt_film_adaptive_select_pooled(c.film._f, 0.01, 2, 2, None, ctypes.byref(n), None) == 1
        assert lib.spt_film_adaptive_select_pooled(c.film._f, 0.01, 0, 0, None, ctypes.byref(n), None) == 1
        assert lib.spt_film_adaptive_select_pooled(c.film._f, 0.01, 2, 0, None, None, None) == 1
        assert lib.spt_film_noise_pool_map(c.film._f, 2, 4, None, None) == 1
        assert lib.spt_film_noise_pool_map(c.film._f, 2, 0, None, None) == 1  # no output buffer
        assert n.value == -3 and np.array_equal(c.film.counts_to_numpy(), c.counts)
        rejected(lambda: plain.adaptive_select(0.01, None, 0, 2, False), plain)
        rejected(lambda: plain.noise_pool_map(2), plain)
        noise.enable_noise(BATCH)
        rejected(lambda: noise.adaptive_select(0.01, None, 0, 2, False), noise)
        rejected(lambda: noise.noise_pool_map(2), noise)          # no batch yet
        young.enable_noise(BATCH)
        young.enable_adaptive()
        young.render(c.r, c.prims, c.cam, c.p, 0, BATCH)
        c.r.stats()
        rejected(lambda: young.adaptive_select(0.01, None, 0, 2, False), young)  # front < 2
        rejected(lambda: young.noise_pool_map(2), young)
        # a shard without rows: nothing to select, and that is no error
        assert empty.info()["rows"] == 0
        empty.enable_noise(BATCH)
        empty.enable_adaptive()
        for k in range(2):
            empty.render(c.r, c.prims, c.cam, empty_p, k * BATCH, BATCH)
        assert empty.adaptive_select(0.01, None, 0, 2, True) == 0
        assert empty.noise_pool_map(2).shape == (0, 70, 3)
        # the film under test still works
        assert c.film.adaptive_select(-1.0, None, 0, 2, False) == int(c.active.sum())
    finally:
        for f in (plain, noise, young, empty):
            f.close()


@pytest.fixture(scope="module")
def head(spt):
    """HEAD NEE at 64x48 @ 64 in batches of 8 and its uniform reference U[0..8]."""
    p = spt.default_params(width=64, height=48, spp=SPP, seed=1, device=0)
    cam, prims = spt.Camera(aspect=64 / 48), spt.cornell_scene()
    return prims, cam, p, uniform_reference(spt, prims, cam, p, BATCH, SPP // BATCH)


def pooled_target(spt, head):
    """A target below the estimate at four batches: the run selects and goes on."""
    prims, cam, p, _ = head
    _, loose = spt.render_adaptive(prims, cam, p, 1e9, return_info=True)
    assert loose["front"] == 4 and loose["pool_radius"] == 0 and loose["pool_exclude_center"] is False
    return 0.7 * max(loose["rmse"])


@pytest.mark.parametrize("loo", [False, True])
def test_render_adaptive_pooled(spt, head, loo):
    prims, cam, p, U = head
    target = pooled_target(spt, head)
    img, info = spt.render_adaptive(prims, cam, p, target, return_info=True, pool_radius=2,
                                    pool_exclude_center=loo)
    assert info["pool_radius"] == 2 and info["pool_exclude_center"] is loo
    cnt = info["counts"]
    batches = cnt & MASK
    assert info["front"] > 4 and info["samples_total"] == int(batches.sum()) * BATCH
    assert info["samples_total"] < 64 * 48 * BATCH * info["front"]  # something retired
    assert (batches >= 4).all() and ((cnt[batches < info["front"]] & RETIRED) != 0).all()
    # the image is the adaptive host resolve of the film's planes: every pixel a uniform film's at its count
    sums, _ = planes_at(U, batches)
    assert np.array_equal(img, spt.film_adaptive_resolve_host(sums, cnt, 64, 48, SPP, BATCH))
    # the first selection is the host statement's on the uniform film after four batches
    four = np.full((48, 64), 4, np.uint32)
    want_c, _ = spt.film_adaptive_select_pooled_host(U[4][0], U[4][1], four, 64, 48, SPP, BATCH, 4, target,
                                                     2, loo)
    assert np.array_equal(batches == 4, (want_c & RETIRED) != 0)
    own, _ = spt.render_adaptive(prims, cam, p, target, return_info=True)
    assert not np.array_equal(own, img)  # the unpooled rule retires other pixels


def test_smallpt_amd_pool(spt, head, tmp_path):
    prims, cam, p, _ = head
    target = pooled_target(spt, head)

    def prog(*args):
        q = subprocess.run([PROG, *[str(a) for a in args]], capture_output=True, text=True, timeout=120,
                           cwd=tmp_path)
        return q.returncode, q.stdout + q.stderr

    for loo, extra in ((False, []), (True, ["--pool-loo"])):
        img, info = spt.render_adaptive(prims, cam, p, target, return_info=True, pool_radius=2,
                                        pool_exclude_center=loo)
        spt.write_image(str(tmp_path / "py.ppm"), img, "p3")
        rc, out = prog(64, 48, SPP, 1, "out.ppm", "--noise", repr(target), "--adaptive", "--pool", 2, *extra)
        assert rc == 0, out[-2000:]
        assert (tmp_path / "out.ppm").read_bytes() == (tmp_path / "py.ppm").read_bytes()
        line = [ln for ln in out.splitlines() if ln.startswith("SAMPLES_TOTAL : ")]
        assert len(line) == 1 and int(line[0].split()[-1]) == info["samples_total"], out[-2000:]
    rc, out = prog(64, 48, SPP, 1, "a.ppm", "--noise", repr(target), "--pool", 2)
    assert rc == 1 and "--pool" in out, out[-2000:]
    rc, out = prog(64, 48, SPP, 1, "b.ppm", "--noise", repr(target), "--adaptive", "--pool", 17)
    assert rc == 1 and "--pool" in out, out[-2000:]
    rc, out = prog(64, 48, SPP, 1, "c.ppm", "--noise", repr(target), "--adaptive", "--pool-loo")
    assert rc == 1 and "--pool" in out, out[-2000:]

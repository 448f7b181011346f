"""The adaptive film on the GPU: passes over a pixel list and per-pixel batch counts.

The yardstick is the uniform noise film: a pixel that holds b batches carries the sums and the
moments of a uniform noise film after b batches, bit for bit, whichever launches rendered them (the
unlisted passes while nothing has retired, the passes over the compacted list afterwards). The
selection is compared with its host statement exactly, the resolve bit for bit, the map and the
summary with the tolerances of tests/test_film_noise.py. Every test here needs symbols the parent
commit does not have."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "small-pathtracer_amd", "smallpt_amd")
REL_F32 = 2.0 ** -21
REL_SUM = 1e-9
RETIRED, MASK = np.uint32(0x80000000), np.uint32(0x7FFFFFFF)
MASK32 = np.uint64(0xFFFFFFFF)
TILTED = dict(lookfrom=(40, 55, 160), lookat=(55, 35, 10), vup=(0.1, 1, 0))


def square128(p):
    """uint64 p < 2^63 -> (lo, hi) of p^2 as uint64 arrays (numpy wraps modulo 2^64)."""
    a, b = p >> np.uint64(32), p & MASK32
    bb, ab = b * b, a * b
    cross_lo, cross_hi = ab << np.uint64(33), ab >> np.uint64(31)
    lo = bb + cross_lo
    hi = a * a + cross_hi + (lo < bb).astype(np.uint64)
    return lo, hi


def add128(lo, hi, lo2, hi2):
    s = lo + lo2
    return s, hi + hi2 + (s < lo2).astype(np.uint64)


def uniform_reference(spt, prims, cam, p, batch, upto=None):
    """One uniform noise film filled in order -> U[b] = (sums, m2) after b batches, b = 0..upto."""
    nb = upto or p.spp // batch
    r, film = spt.Renderer(p.device), spt.Film(p, p.device)
    try:
        film.enable_noise(batch)
        U = [(film.to_numpy(), film.noise_to_numpy())]
        for k in range(nb):
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


def shrinking_masks(rng, rows, w, n):
    """n keep masks for n selections in a row: a checkerboard, whole rows removed, seeded random
    ones, and a last one that leaves exactly one of the pixels still active."""
    yy, xx = np.mgrid[0:rows, 0:w]
    masks = [((yy + xx) % 2 == 0), (yy % 3 != 1) | (rows < 3)]
    while len(masks) < n - 1:
        masks.append(rng.random((rows, w)) < 0.6)
    masks = masks[: max(0, n - 1)]
    active = np.ones((rows, w), bool)
    for m in masks:
        if not (active & m).any():  # never empty before the last selection
            m |= active
        active &= m
    last = np.zeros((rows, w), bool)
    idx = np.flatnonzero(active)
    last.reshape(-1)[idx[int(rng.integers(0, idx.size))]] = True
    return [m.astype(np.uint8) for m in masks + [last]]


class Tracker:
    """The counts the masks imply, kept on the host beside the film."""

    def __init__(self, rows, w, batch):
        self.batches = np.zeros((rows, w), np.uint32)
        self.active = np.ones((rows, w), bool)
        self.batch, self.total = batch, 0

    def rendered(self):
        self.batches[self.active] += 1
        self.total += int(self.active.sum()) * self.batch

    def select(self, keep):
        self.active &= keep.astype(bool)

    def counts(self):
        return self.batches | np.where(self.active, np.uint32(0), RETIRED)


def one_pass(spt, film, r, prims, cam, p, batch, trk):
    """The next window; its statistics count the active pixels only."""
    front = film.adaptive_info()["front"]
    n_active = film.adaptive_info()["n_active"]
    assert n_active == int(trk.active.sum())
    film.render(r, prims, cam, p, front * batch, batch)
    assert r.stats()["samples"] == n_active * batch
    trk.rendered()
    a = film.adaptive_info()
    assert a == {"enabled": 1, "front": front + 1, "n_active": n_active, "samples_total": trk.total}
    assert film.info()["samples_done"] == (front + 1) * batch


def drive(spt, film, r, prims, cam, p, batch, masks, trk, first=True):
    """Two full passes (first), then a selection by keep mask before each further pass."""
    if first:
        one_pass(spt, film, r, prims, cam, p, batch, trk)
        one_pass(spt, film, r, prims, cam, p, batch, trk)
    for keep in masks:
        trk.select(keep)
        assert film.adaptive_select(-1.0, keep) == int(trk.active.sum())
        one_pass(spt, film, r, prims, cam, p, batch, trk)


def _close(got, want, rel):
    return abs(got - want) <= rel * abs(want)


def check_film(spt, film, p, batch, U, trk, one=None, statements=True):
    """The film against the uniform reference at every pixel's own count, and against the host
    statements."""
    i = film.info()
    rows, w = i["rows"], i["width"]
    cnt = film.counts_to_numpy()
    assert cnt.dtype == np.uint32 and cnt.shape == (rows, w)
    assert np.array_equal(cnt, trk.counts())
    sums, m2 = film.to_numpy(), film.noise_to_numpy()
    want_s, want_m = planes_at(U, trk.batches)
    assert np.array_equal(sums, want_s)
    assert np.array_equal(m2, want_m)
    if not statements:
        return
    front = film.adaptive_info()["front"]
    res = film.resolve()
    assert np.array_equal(res, spt.film_adaptive_resolve_host(sums, cnt, w, rows, p.spp, batch))
    if one is not None:  # pixels that hold every batch carry the one-shot render's bits
        full = trk.batches == p.spp // batch
        assert np.array_equal(res[full], one[full])
    se = film.noise_map()
    want = spt.film_adaptive_noise_map_host(sums, m2, cnt, w, rows, p.spp, batch)
    assert np.array_equal(se == 0, want == 0)
    assert np.all(np.abs(se.astype(np.float64) - want) <= REL_F32 * want)
    s1, s2 = film.noise_summary(), film.noise_summary()
    assert s1 == s2
    hs = spt.film_adaptive_noise_summary_host(sums, m2, cnt, w, rows, p.spp, batch, front)
    for c in range(3):
        assert _close(s1["rmse"][c], hs["rmse"][c], REL_SUM), (c, s1, hs)
    assert _close(s1["rmse_all"], hs["rmse_all"], REL_SUM)
    assert _close(s1["se_max"], hs["se_max"], REL_F32) and s1["se_max"] == float(se.max())
    assert s1["clamped"] == hs["clamped"] and s1["batches_done"] == front


def adaptive_film(spt, p, batch):
    r, film = spt.Renderer(p.device), spt.Film(p, p.device)
    film.enable_noise(batch)
    film.enable_adaptive()
    return film, r


@pytest.fixture(scope="module")
def head(spt):
    """HEAD NEE at 64x48 @ 16, batch 2, seed 1: scene, camera, params, the one-shot render and the
    uniform reference U[0..8]."""
    p = spt.default_params(width=64, height=48, spp=16, seed=1, device=0)
    cam, prims = spt.Camera(aspect=64 / 48), spt.cornell_scene()
    one = spt.render(prims, cam, p)
    one.setflags(write=False)
    return prims, cam, p, one, uniform_reference(spt, prims, cam, p, 2)


def test_exact_by_depth(spt, head):
    prims, cam, p, one, U = head
    masks = shrinking_masks(np.random.default_rng(11), 48, 64, 6)
    assert int(masks[-1].sum()) == 1
    film, r = adaptive_film(spt, p, 2)
    try:
        trk = Tracker(48, 64, 2)
        drive(spt, film, r, prims, cam, p, 2, masks, trk)
        assert film.adaptive_info()["front"] == 8 and film.adaptive_info()["n_active"] == 1
        assert sorted(set(trk.batches.reshape(-1).tolist())) == [2, 3, 4, 5, 6, 7, 8]
        check_film(spt, film, p, 2, U, trk, one)
        assert trk.total < 64 * 48 * 16
        film.clear()  # counts, list and totals go back
        assert film.adaptive_info() == {"enabled": 1, "front": 0, "n_active": 64 * 48, "samples_total": 0}
        assert not film.counts_to_numpy().any() and not film.to_numpy().any()
        trk = Tracker(48, 64, 2)
        drive(spt, film, r, prims, cam, p, 2, masks[:1], trk)
        check_film(spt, film, p, 2, U, trk, statements=False)
    finally:
        film.close()
        r.close()


def small_case(spt, prims, cam, p, batch=2, extra_masks=()):
    """The check of test_exact_by_depth at a small size: two full passes, then a selection before
    each further pass; extra_masks: further films whose single selection keeps just that mask."""
    U = uniform_reference(spt, prims, cam, p, batch)
    rows, w = U[0][0].shape[:2]
    nb = p.spp // batch
    runs = [shrinking_masks(np.random.default_rng(5), rows, w, nb - 2)] + [[m] for m in extra_masks]
    for masks in runs:
        film, r = adaptive_film(spt, p, batch)
        try:
            trk = Tracker(rows, w, batch)
            drive(spt, film, r, prims, cam, p, batch, masks, trk)
            check_film(spt, film, p, batch, U, trk)
        finally:
            film.close()
            r.close()
    return rows, w


@pytest.mark.parametrize("name", ["cosine", "tilted", "spheres32", "specular", "edited_box", "generic"])
def test_every_unit_setup_path(spt, name):
    kw, camkw, want = {}, {}, None
    prims = spt.cornell_scene()
    if name == "cosine":
        kw, want = dict(nee_prob=0.0), "const_cos"
    elif name == "tilted":
        camkw, want = TILTED, "const_nee_cam"
    elif name == "spheres32":
        prims, want = spt.spheres32_scene(), "sphdiff_nee"
    elif name == "specular":
        prims, kw, want = spt.cornell_specular_scene(), dict(max_depth=16), "generic"
    elif name == "edited_box":
        prims, want = spt.move_short_box(spt.cornell_scene(), 3.0), "upbox_nee"
    elif name == "generic":
        kw, want = dict(flags=spt.kernel_flag("generic")), "generic"
    p = spt.default_params(width=32, height=24, spp=8, seed=7, device=0, **kw)
    cam = spt.Camera(aspect=32 / 24, **camkw)
    assert spt.select_kernel(prims, cam, p)["name"] == want
    small_case(spt, prims, cam, p)


def test_shard_and_the_ends_of_its_list(spt):
    p = spt.default_params(width=32, height=24, spp=8, seed=7, device=0, tile_rows=2, shard_index=1,
                           shard_count=3)
    rows = len(spt.shard_rows(p))
    first, last = np.zeros((rows, 32), np.uint8), np.zeros((rows, 32), np.uint8)
    first.reshape(-1)[0] = 1
    last.reshape(-1)[-1] = 1
    assert small_case(spt, spt.cornell_scene(), spt.Camera(aspect=32 / 24), p,
                      extra_masks=(first, last)) == (8, 32)


@pytest.mark.parametrize("w,h", [(37, 11), (24, 3), (1, 1), (50, 27)])
def test_odd_sizes_and_list_lengths(spt, w, h):
    p = spt.default_params(width=w, height=h, spp=6, seed=3, device=0)
    prims, cam = spt.cornell_scene(), spt.Camera(aspect=w / h)
    U = uniform_reference(spt, prims, cam, p, 2)
    n = w * h
    rng = np.random.default_rng(w * 100 + h)
    for length in sorted({x for x in (1, 3, 255, 257, n - 1, n) if 1 <= x <= n}):
        keep = np.zeros(n, np.uint8)
        keep[rng.choice(n, size=length, replace=False)] = 1
        film, r = adaptive_film(spt, p, 2)
        try:
            trk = Tracker(h, w, 2)
            drive(spt, film, r, prims, cam, p, 2, [keep.reshape(h, w)], trk)
            assert film.adaptive_info()["n_active"] == length
            check_film(spt, film, p, 2, U, trk, statements=length in (1, 257, n - 1))
        finally:
            film.close()
            r.close()


def test_threshold_selection(spt, head):
    prims, cam, p, _, U = head
    film, r = adaptive_film(spt, p, 2)
    try:
        trk = Tracker(48, 64, 2)
        for _ in range(3):
            one_pass(spt, film, r, prims, cam, p, 2, trk)
        se = film.noise_map().max(axis=-1)
        thresholds = [float(np.median(se)), float(np.percentile(se, 90)), float(se.max()) * 1.5]
        assert 0 < thresholds[0] < thresholds[1] < thresholds[2]
        sums, m2 = film.to_numpy(), film.noise_to_numpy()
        counts = film.counts_to_numpy()
        assert np.array_equal(counts, np.full((48, 64), 3, np.uint32))
        left = []
        for t in thresholds:
            want_c, want_l = spt.film_adaptive_select_host(sums, m2, counts, 64, 48, 16, 2, 3, t)
            n = film.adaptive_select(t)
            counts = film.counts_to_numpy()
            assert n == want_l.size and np.array_equal(counts, want_c), t
            assert film.adaptive_info()["n_active"] == n
            left.append(n)
        assert 64 * 48 > left[0] > left[1] > left[2] == 0
        # the selection changed no sample; the next pass has nothing to render
        assert np.array_equal(film.to_numpy(), sums) and np.array_equal(film.noise_to_numpy(), m2)
        info, ainfo = film.info(), film.adaptive_info()
        with pytest.raises(spt.SptError) as e:
            film.render(r, prims, cam, p, 6, 2)
        assert e.value.status == 1
        assert film.info() == info and film.adaptive_info() == ainfo
        assert np.array_equal(film.to_numpy(), sums) and np.array_equal(film.noise_to_numpy(), m2)
        assert np.array_equal(film.counts_to_numpy(), counts)
        # the list the second threshold left is the one a listed pass renders: redo it on a new film
        film.clear()
        trk = Tracker(48, 64, 2)
        for _ in range(3):
            one_pass(spt, film, r, prims, cam, p, 2, trk)
        film.adaptive_select(thresholds[0])
        n = film.adaptive_select(thresholds[1])
        want_c, want_l = spt.film_adaptive_select_host(sums, m2, np.full((48, 64), 3, np.uint32), 64, 48,
                                                       16, 2, 3, thresholds[1])
        assert n == want_l.size == left[1]
        trk.active = (want_c & RETIRED) == 0
        one_pass(spt, film, r, prims, cam, p, 2, trk)
        check_film(spt, film, p, 2, U, trk)
    finally:
        film.close()
        r.close()


def test_listed_pass_at_1024x768(spt):
    """The size at which spt_film.hip records its load hazard; the compaction runs over 3072 blocks."""
    w, h, batch = 1024, 768, 2
    p = spt.default_params(width=w, height=h, spp=8, seed=1, device=0)
    cam, prims = spt.Camera(aspect=w / h), spt.cornell_scene()
    U = uniform_reference(spt, prims, cam, p, batch, upto=3)
    # the uniform film's own moments restated in 128-bit numpy arithmetic from its sums
    lo, hi = np.zeros_like(U[0][0]), np.zeros_like(U[0][0])
    for b in range(1, 4):
        lo, hi = add128(lo, hi, *square128(U[b][0] - U[b - 1][0]))
        assert np.array_equal(U[b][1][..., 0], lo) and np.array_equal(U[b][1][..., 1], hi)
    keep = (np.random.default_rng(21).random((h, w)) < 0.5).astype(np.uint8)
    film, r = adaptive_film(spt, p, batch)
    try:
        trk = Tracker(h, w, batch)
        drive(spt, film, r, prims, cam, p, batch, [keep], trk)
        assert film.adaptive_info()["n_active"] == int(keep.sum())
        cnt = film.counts_to_numpy()
        assert np.array_equal(cnt, np.where(keep != 0, np.uint32(3), np.uint32(2) | RETIRED))
        sums, m2 = film.to_numpy(), film.noise_to_numpy()
        on = keep.astype(bool)
        bad = sums != np.where(on[..., None], U[3][0], U[2][0])
        assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4].tolist())
        bad = m2 != np.where(on[..., None, None], U[3][1], U[2][1])
        assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4].tolist())
        res = film.resolve()
        assert np.array_equal(res, spt.film_adaptive_resolve_host(sums, cnt, w, h, 8, batch))
    finally:
        film.close()
        r.close()


def test_checkpoint(spt, head):
    prims, cam, p, one, U = head
    masks = shrinking_masks(np.random.default_rng(11), 48, 64, 6)
    a, ra = adaptive_film(spt, p, 2)
    b, rb = adaptive_film(spt, p, 2)
    try:
        ta = Tracker(48, 64, 2)
        drive(spt, a, ra, prims, cam, p, 2, masks[:3], ta)
        sums, m2, counts = a.to_numpy(), a.noise_to_numpy(), a.counts_to_numpy()
        front = a.adaptive_info()["front"]
        assert front == 5
        b.from_numpy(sums, front * 2)
        b.noise_from_numpy(m2, front)
        b.counts_from_numpy(counts)
        assert b.adaptive_info() == a.adaptive_info() and b.info() == a.info()
        tb = Tracker(48, 64, 2)
        tb.batches, tb.active, tb.total = ta.batches.copy(), ta.active.copy(), ta.total
        drive(spt, a, ra, prims, cam, p, 2, masks[3:], ta, first=False)
        drive(spt, b, rb, prims, cam, p, 2, masks[3:], tb, first=False)
        assert np.array_equal(a.to_numpy(), b.to_numpy())
        assert np.array_equal(a.noise_to_numpy(), b.noise_to_numpy())
        assert np.array_equal(a.counts_to_numpy(), b.counts_to_numpy())
        assert a.adaptive_info() == b.adaptive_info()
        assert np.array_equal(a.resolve(), b.resolve())
        check_film(spt, b, p, 2, U, tb, one)
        with pytest.raises(spt.SptError):  # no file format for the counts
            b.save("/dev/null")
        bad = counts.copy()  # two active pixels at different counts
        act = np.flatnonzero((bad.reshape(-1) & RETIRED) == 0)
        bad.reshape(-1)[act[0]] -= 1
        with pytest.raises(spt.SptError) as e:
            b.counts_from_numpy(bad)
        assert e.value.status == 1
        assert np.array_equal(a.counts_to_numpy(), b.counts_to_numpy())
    finally:
        for f in (a, b):
            f.close()
        ra.close()
        rb.close()


def test_rejections_leave_the_film_unchanged(spt, head):
    prims, cam, p, _, _ = head
    film, r = adaptive_film(spt, p, 2)
    plain, noise, other = spt.Film(p, 0), spt.Film(p, 0), spt.Film(p, 0)
    long_p = spt.default_params(width=8, height=8, spp=8192, seed=1, device=0)
    long_film = spt.Film(long_p, 0)
    try:
        def state(f):
            n, a = f.noise_info(), f.adaptive_info()
            return (f.info(), n, a, f.to_numpy(), f.noise_to_numpy() if n["enabled"] else None,
                    f.counts_to_numpy() if a["enabled"] else None)

        def rejected(call, *films):
            before = [state(f) for f in films]
            with pytest.raises(spt.SptError) as e:
                call()
            assert e.value.status == 1
            for f, b in zip(films, before):
                a = state(f)
                assert a[:3] == b[:3] and np.array_equal(a[3], b[3])
                for x, y in zip(a[4:], b[4:]):
                    assert (x is None and y is None) or np.array_equal(x, y)

        rejected(lambda: plain.enable_adaptive(), plain)            # a plain film
        noise.enable_noise(2)
        noise.render(r, prims, cam, p, 0, 2)
        r.stats()
        rejected(lambda: noise.enable_adaptive(), noise)            # a film that holds samples
        long_film.enable_noise(1)
        rejected(lambda: long_film.enable_adaptive(), long_film)    # 8192 batches > 4096
        assert long_film.adaptive_info()["enabled"] == 0
        rejected(lambda: film.enable_adaptive(), film)              # twice
        rejected(lambda: film.render(r, prims, cam, p, 2, 2), film)  # not the next window
        film.render(r, prims, cam, p, 0, 2)
        r.stats()
        rejected(lambda: film.render(r, prims, cam, p, 0, 2), film)  # a window it holds
        rejected(lambda: film.render(r, prims, cam, p, 4, 2), film)  # a window ahead
        rejected(lambda: film.adaptive_select(0.1), film)           # one batch: no error yet
        film.render(r, prims, cam, p, 2, 2)
        r.stats()
        rejected(lambda: film.adaptive_select(float("nan")), film)  # a NaN threshold
        rejected(lambda: plain.adaptive_select(0.1), plain)
        rejected(lambda: noise.adaptive_select(0.1), noise)
        rejected(lambda: plain.counts_to_numpy(), plain)
        other.enable_noise(2)
        other.enable_adaptive()
        rejected(lambda: film.merge(other), film, other)            # adaptive on either side
        rejected(lambda: noise.merge(film), noise, film)
        rejected(lambda: film.merge(noise), noise, film)
        # every film still works
        assert film.adaptive_select(-1.0) == 64 * 48
        film.render(r, prims, cam, p, 4, 2)
        r.stats()
        assert film.adaptive_info()["front"] == 3
        noise.render(r, prims, cam, p, 2, 2)
        assert noise.noise_info()["batches_done"] == 2
    finally:
        for f in (film, plain, noise, other, long_film):
            f.close()
        r.close()


def test_render_adaptive(spt, head):
    prims, cam, p, one, U = head
    img, info = spt.render_adaptive(prims, cam, p, 1e9, return_info=True)  # batch = 16 / 8
    assert info["front"] == 4 and info["samples_total"] == 64 * 48 * 8
    assert np.array_equal(info["counts"], np.full((48, 64), 4, np.uint32))
    until, uinfo = spt.render_until(prims, cam, p, 1e9, min_batches=4, return_info=True)
    assert np.array_equal(img, until)
    assert all(_close(a, b, REL_SUM) for a, b in zip(info["rmse"], uinfo["rmse"]))
    img, info = spt.render_adaptive(prims, cam, p, 1e9, min_batches=2, return_info=True)
    assert info["front"] == 2
    # target 0: a pixel goes on to the last batch unless it has no error left to estimate
    img, info = spt.render_adaptive(prims, cam, p, 0.0, return_info=True)
    cnt = info["counts"]
    batches = cnt & MASK
    full = batches == 8
    assert info["front"] == 8 and full.any() and np.array_equal(img[full], one[full])
    early = ~full
    assert early.any(), "the light's pixels clamp: they retire at the first selection"
    assert ((cnt[early] & RETIRED) != 0).all() and (batches[early] >= 4).all()
    for b in sorted(set(batches[early].tolist())):
        se = spt.film_noise_map_host(U[b][0], U[b][1], 64, 48, 16, 2 * b, 2, b)
        assert not se[early & (batches == b)].any()
    assert info["samples_total"] == int(batches.sum()) * 2
    with pytest.raises(ValueError):
        spt.render_adaptive(prims, cam, spt.default_params(width=64, height=48, spp=12, device=0), 0.1)


def test_smallpt_amd_adaptive(spt, head, tmp_path):
    prims, cam, p, _, _ = head
    _, loose = spt.render_adaptive(prims, cam, p, 1e9, return_info=True)
    target = 0.7 * max(loose["rmse"])  # below the estimate at four batches: the run selects and goes on
    img, info = spt.render_adaptive(prims, cam, p, target, return_info=True)
    assert info["front"] > 4 and info["samples_total"] < 64 * 48 * 2 * info["front"]
    spt.write_image(str(tmp_path / "py.ppm"), img, "p3")

    def prog(*args):
        q = subprocess.run([PROG, *[str(a) for a in args]], capture_output=True, text=True, timeout=120,
                           cwd=tmp_path)
        return q.returncode, q.stdout + q.stderr

    rc, out = prog(64, 48, 16, 1, "c.ppm", "--noise", repr(target), "--adaptive")
    assert rc == 0, out[-2000:]
    assert (tmp_path / "c.ppm").read_bytes() == (tmp_path / "py.ppm").read_bytes()
    line = [ln for ln in out.splitlines() if ln.startswith("SAMPLES_TOTAL : ")]
    assert len(line) == 1 and int(line[0].split()[-1]) == info["samples_total"], out[-2000:]
    assert f" after {2 * info['front']} / 16" in out
    rc, out = prog(64, 48, 16, 1, "d.ppm", "--noise", repr(target), "--adaptive", "--film", "f.bin")
    assert rc == 1 and "--film" in out, out[-2000:]
    rc, out = prog(64, 48, 16, 1, "e.ppm", "--adaptive")
    assert rc == 1 and "--noise" in out, out[-2000:]

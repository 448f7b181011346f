"""The render loop's lane states and the masks made from them (spt_kernel.hip: LaneStates, the
generate guard, the traced shadow lanes' and the light compare's masks, the camera / cosine bit
select, the normal's sign from d_a's sign bit), on the GPU.

Every render is compared bit for bit with the oracle's counter mode: the image, every key of
spt.STAT_KEYS and through them every event count, no tolerance (the contract is exact), and the
variant that ran is the one the case means. tests/test_lane_states_cases.py shows on the CPU that the
cases hold idle lanes, stolen ranges, misses and every kind of shadow ray."""
import numpy as np
import pytest

import lane_states_cases as lc

pytestmark = pytest.mark.gpu


def _check(spt, oracle, prims, cam, p, kernel):
    gpu, st = spt.render(prims, cam, p, return_stats=True)
    cpu, cst = oracle.counter_render(prims, cam._c, p)
    assert st["kernel"] == kernel
    assert gpu.shape == cpu.shape == (p.height, p.width, 3)
    assert np.array_equal(gpu, cpu)
    for k in spt.STAT_KEYS:
        assert st[k] == cst[k], (k, st[k], cst[k])
    assert st["samples"] == p.width * p.height * p.spp
    return st


@pytest.mark.parametrize("family", list(lc.FAMILIES))
def test_kernel_family(spt, oracle, family):
    """64x48 @ 16: the literal NEE and cosine kernels, a moved box, an edited light, a tilted camera,
    SPEC/REFR materials (the generic kernel keeps the idle state at 0) and the sphere kernel."""
    prims, cam, p, kernel, _ = lc.family_case(spt, family)
    st = _check(spt, oracle, prims, cam, p, kernel)
    if lc.FAMILIES[family][4]:  # an early-resolve NEE kernel: proven and traced shadow rays
        assert 0 < st["shadow_proven"] < st["shadow_traced"]


@pytest.mark.parametrize("shape", list(lc.FEW_UNITS))
def test_fewer_units_than_lanes(spt, oracle, shape):
    """Most lanes are idle from the first iteration on; every wave leaves through the empty pass."""
    _check(spt, oracle, *lc.head_case(spt, lc.FEW_UNITS[shape])[:4])


def test_tail_steals(spt, oracle):
    """64x48 @ 64 in units of 64 samples: idle lanes take halves of busy lanes' ranges."""
    _check(spt, oracle, *lc.head_case(spt, lc.STEAL)[:4])


@pytest.fixture(scope="module")
def film_truth(spt, oracle):
    """The film case and the oracle's one-shot image of it."""
    prims, cam, p, kernel, _ = lc.head_case(spt, lc.FILM)
    one = oracle.counter_render(prims, cam._c, p)[0]
    one.setflags(write=False)
    return prims, cam, p, kernel, one


def test_two_window_film(spt, film_truth):
    """Windows of 8 + 8 samples, two launches: the one-shot image, bit for bit."""
    prims, cam, p, kernel, one = film_truth
    img, st = spt.render_progressive(prims, cam, p, [(0, lc.FILM_BATCH), (lc.FILM_BATCH, lc.FILM_BATCH)],
                                     return_stats=True)
    assert np.array_equal(img, one)
    assert st["samples"] == p.width * p.height * p.spp


def test_pixel_list_pass(spt, oracle, film_truth):
    """The second window over a pixel list (a checkerboard): the listed pixels carry the one-shot
    image's bits, and the pass's statistics are the oracle's of that window at those pixels."""
    prims, cam, p, kernel, one = film_truth
    b, half = lc.FILM_BATCH, lc.FILM_BATCH // 2  # (a selection needs two batches: each window is two)
    yy, xx = np.mgrid[0:p.height, 0:p.width]
    keep = ((yy + xx) % 2 == 0)
    r, film = spt.Renderer(p.device), spt.Film(p, p.device)
    try:
        film.enable_noise(half)
        film.enable_adaptive()
        for base in (0, half):
            film.render(r, prims, cam, p, base, half)
            assert r.kernel() == kernel and r.stats()["samples"] == p.width * p.height * half
        assert film.adaptive_select(-1.0, keep.astype(np.uint8)) == int(keep.sum())
        st = dict.fromkeys(spt.STAT_KEYS, 0)
        for base in (b, b + half):
            film.render(r, prims, cam, p, base, half)
            one_pass = r.stats()
            assert r.kernel() == kernel
            for k in st:
                st[k] += one_pass[k]
        assert st["samples"] == int(keep.sum()) * b
        res = film.resolve()
        assert np.array_equal(res[keep], one[keep])
        assert not np.array_equal(res[~keep], one[~keep])  # (half the samples there)
    finally:
        film.close()
        r.close()
    # A path's events do not depend on the sample count (it only scales the contributions), so the
    # list pass's counts are the oracle's of samples 0..15 less those of samples 0..7 at the listed
    # pixels.
    listed = (yy * p.width + xx)[keep].astype(np.uint32)
    _, c_all = oracle.counter_render_pixels(prims, cam._c, p, listed)
    _, c_first = oracle.counter_render_pixels(prims, cam._c, lc.params(spt, **dict(lc.FILM, spp=b)), listed)
    for k in spt.STAT_KEYS:
        assert st[k] == c_all[k] - c_first[k], (k, st[k], c_all[k], c_first[k])


def test_rays_parallel_to_planes(spt, oracle):
    """Raw cameras with an exactly zero direction component (a miss whose d_a is +-0) and fans from
    origins exactly on the moved box's and the room's planes."""
    cases = lc.zero_cases(spt, oracle)
    assert len(cases) >= len(lc.ZERO_VIEWS) + 3
    misses = 0
    for label, prims, cam, p, kernel in cases:
        misses += _check(spt, oracle, prims, cam, p, kernel)["misses"]
    assert misses > 0

"""The pool set-up through LDS (spt_kernel.hip, SPT_POOL_LDS): the wave that grabs a pool computes the
terms of all its units at once into its own region of LDS, and a lane that takes a unit reads its
entry. Every lane must end up holding what it used to compute for itself, so every render here is
compared bit for bit with the oracle's counter mode: the image, and the launch statistics.

The long-launch path (always full pools, the young cut, stealing) is pinned by the full-size C2/C3
row checks of test_gpu_parity.py; these cases are the ones the fill and the fetch can get wrong on
their own: a pool shorter than the wave, many pools per wave with guided grabs of any size and
start, the pixel mapping of a shard, each camera form, a sample window that does not start at 0."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILTED = dict(lookfrom=(40, 55, 160), lookat=(55, 35, 10), vup=(0.1, 1, 0))


def _check(spt, oracle, prims, cam, p, kernel=None):
    gpu, st = spt.render(prims, cam, p, return_stats=True)
    cpu, cst = oracle.counter_render(prims, cam._c, p, rows=spt.shard_rows(p))
    if kernel is not None:
        assert st["kernel"] == kernel
    assert gpu.shape == cpu.shape
    assert np.array_equal(gpu, cpu)
    for k in spt.STAT_KEYS:
        assert st[k] == cst[k], (k, st[k], cst[k])
    return st


def test_partial_pool(spt, oracle):
    """5x3 px @ 4 spp in units of one sample (the smallest chunk the host accepts; 0 asks for the
    default): 60 units in all, so the one pool that is ever filled is shorter than the wave and only
    the entries below pool_end may be read."""
    p = spt.default_params(width=5, height=3, spp=4, seed=2, device=0, chunk=1)
    st = _check(spt, oracle, spt.cornell_scene(), spt.Camera(aspect=5 / 3), p, "const_nee")
    assert st["samples"] == 60 < 64


def test_many_pools_per_wave_with_guided_grabs(spt, oracle):
    """256x192 @ 64 spp in units of 2 samples: a short launch (guided grabs, 4 blocks per CU) of
    1.57 M units, so every resident wave fills its region many times, and the guided grabs at the
    end give pools of every size from 64 down to 8 at starts that are no multiple of 64."""
    import torch
    w, h, spp, chunk = 256, 192, 64, 2
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    # plan_launch (spt_dispatch.cpp): a short launch below 2000 lane-iterations per resident lane,
    # 4 blocks per CU of 4 waves each
    assert w * h * spp * 5.3 / (n_cu * 8 * 256) < 2000.0
    waves = n_cu * 4 * 4
    n_units = w * h * (spp // chunk)
    assert n_units >= 2 * 2 * 64 * waves, (n_units, waves)  # two full pools each, twice over
    p = spt.default_params(width=w, height=h, spp=spp, seed=1, device=0, chunk=chunk)
    st = _check(spt, oracle, spt.cornell_scene(), spt.Camera(aspect=w / h), p, "const_nee")
    assert st["samples"] == w * h * spp


def test_pixel_mapping_of_a_shard(spt, oracle):
    """Width no multiple of 8 (the pixel spread takes a smaller K), height no multiple of tile_rows,
    the second of three shards: the fill's row / tile / shard arithmetic."""
    p = spt.default_params(width=41, height=36, spp=8, seed=5, device=0, tile_rows=8,
                           shard_index=1, shard_count=3)
    rows = spt.shard_rows(p)
    assert len(rows) == 12 and rows[0] == 8 and rows[-1] == 35  # tile 1, and the 4 rows of tile 4
    _check(spt, oracle, spt.cornell_scene(), spt.Camera(aspect=41 / 36), p, "const_nee")


@pytest.mark.parametrize("camkw,pkw,kernel", [
    ({}, {}, "const_nee"),                    # CAMAX 1: P_x, P_y per unit
    (TILTED, {}, "const_nee_cam"),            # CAMAX 2: P_x, P_y, P_z per unit
    ({}, dict(nee_prob=0.5), "const"),        # the run-time estimator: raster terms, P per ray
], ids=["reference_camera", "tilted_camera", "runtime_estimator"])
def test_camera_forms(spt, oracle, camkw, pkw, kernel):
    p = spt.default_params(width=40, height=36, spp=8, seed=3, device=0, **pkw)
    _check(spt, oracle, spt.cornell_scene(), spt.Camera(aspect=40 / 36, **camkw), p, kernel)


def test_sample_window(spt, oracle):
    """Two film passes of 8 spp at 64x48 (the second with s_base = 8) are the one-shot 16 spp
    render, and the oracle's, bit for bit; their statistics add up to the oracle's."""
    p = spt.default_params(width=64, height=48, spp=16, seed=1, device=0)
    cam = spt.Camera(aspect=64 / 48)
    prims = spt.cornell_scene()
    one = spt.render(prims, cam, p)
    cpu, cst = oracle.counter_render(prims, cam._c, p)
    r, film = spt.Renderer(0), spt.Film(p, 0)
    try:
        stats = []
        for base in (0, 8):
            film.render(r, prims, cam, p, base, 8)
            stats.append(r.stats())
        assert film.info()["samples_done"] == 16
        img = film.resolve()
    finally:
        film.close()
        r.close()
    assert np.array_equal(img, one)
    assert np.array_equal(img, cpu)
    for k in spt.STAT_KEYS:
        assert stats[0][k] + stats[1][k] == cst[k], k

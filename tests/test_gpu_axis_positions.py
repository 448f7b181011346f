"""The literal kernels' slot numbering (spt_cornell.h, cornell_slot: the hit's plane axis in bits 4 and
5 of the winning key) where it can matter: candidates of different axes whose t share the upper 26
bits, so that the key's low six bits decide the winner. Rays from three points inside the room at the
room's corners and edges and the boxes' corners and top edges, and at their one-ulp neighbours
(tests/axis_positions_cases.py), ray by ray through the render kernels as tests/test_gpu_rays.py
traces single rays (a camera with horizontal = vertical = 0), against oracle.intersect_batch.

Per ray, two renders of one pixel:
  * the id scene (ray_truth.id_scene: every primitive black and emitting its index) at 1 spp, which the
    `const` kernel runs: the pixel decodes to the first hit's id (a miss is counted, and shows prim
    0's id, which a missed path ray keeps), which must be the oracle's for the direction the contract
    normalises the camera's to (guide_truth.camera_rays);
  * the HEAD scene itself at 8 spp (const_nee_cam; const_cos_cam as well for the tie rays): image and
    statistics bit for bit the oracle's counter mode. A render returns no t as such; every sample's path
    goes on from the hit point o + d t, so a first hit's t that is not the oracle's shows in the bits
    of the pixel. The oracle's own t of a hit is checked to be its winner's plane distance, the contract's
    fma restated from the oracle's pieces (axis_positions_cases.plane_ts).
The oracle alone first counts the rays whose two nearest candidates lie on different axes and agree in
the upper 26 bits of t: fewer than 32 and the test fails as vacuous (the three origins hold 259, 263
and 191 of 308 rays each).
"""
import numpy as np
import pytest

import axis_positions_cases as ac
import ray_truth as rt

pytestmark = pytest.mark.gpu
MIN_TIES = 32


@pytest.fixture(scope="module")
def scenes(spt):
    prims = spt.cornell_scene()
    return prims, rt.id_scene(spt, prims)


def _render(spt, oracle, prims, cam, p, want, label):
    gpu, gst = spt.render(prims, cam, p, return_stats=True)
    assert gst["kernel"] == want, (label, gst["kernel"], want)
    cpu, cst = oracle.counter_render(prims, cam._c, p)
    assert np.array_equal(gpu, cpu), (label, gpu.tolist(), cpu.tolist())
    assert {k: gst[k] for k in spt.STAT_KEYS} == cst, label
    return gpu, gst


@pytest.mark.parametrize("oi", range(len(ac.ORIGINS)))
def test_first_hits_at_axis_ties(spt, oracle, scenes, oi):
    prims, id_prims = scenes
    origin = ac.ORIGINS[oi]
    rays = ac.rays(spt, oracle, prims, origin)
    tgts = [t for _, t in rays]
    d = ac.traced_dirs(spt, oracle, origin, tgts)
    o = np.broadcast_to(np.asarray(origin, np.float32), d.shape).copy()
    ties = ac.axis_ties(spt, oracle, prims, origin, d)
    print(f"origin {origin}: {len(rays)} rays, {int(ties.sum())} axis ties")
    assert int(ties.sum()) >= MIN_TIES, "vacuous: too few rays whose key's position bits decide between axes"
    t32, ids = oracle.intersect_batch(prims, spt.default_params(), o, d)
    # the oracle's t of a hit is its winner's own plane distance, the contract's fma, bit for bit
    tp = ac.plane_ts(oracle, prims, origin, d)
    hit = ids >= 0
    assert np.array_equal(t32[hit].view(np.uint32), tp[hit, ids[hit]].view(np.uint32))
    assert np.all(t32[~hit] == np.float32(1e20))
    p_id = spt.default_params(width=1, height=1, spp=1, seed=5)
    p_nee = spt.default_params(width=1, height=1, spp=ac.SPP, seed=5, nee_prob=1.0)
    p_cos = spt.default_params(width=1, height=1, spp=ac.SPP, seed=5, nee_prob=0.0)
    got = np.empty(len(rays), dtype=np.int64)
    for i, (label, tgt) in enumerate(rays):
        cam = ac.ray_camera(spt, origin, tgt)
        img, st = _render(spt, oracle, id_prims, cam, p_id, "const", label)
        # a missed path ray keeps prim 0's id (the reference's :373-374) and the miss is counted
        got[i] = rt.decode_ids(img)[0, 0] if st["misses"] == 0 else rt.MISS
        assert st["misses"] <= 1 and (st["misses"] == 0 or rt.decode_ids(img)[0, 0] == 0), label
        _render(spt, oracle, prims, cam, p_nee, "const_nee_cam", label)
        if ties[i]:
            _render(spt, oracle, prims, cam, p_cos, "const_cos_cam", label)
    bad = np.flatnonzero(got != ids)
    assert bad.size == 0, [(rays[i][0], int(got[i]), int(ids[i])) for i in bad[:8]]
    assert len(set(ids[ties].tolist()) - {-1}) >= 4  # (ties won by walls, the light's neighbours, box faces and tops)

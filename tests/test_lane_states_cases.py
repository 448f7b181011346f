"""The cases of tests/test_gpu_lane_states.py are not vacuous (CPU: the oracle and the dispatch query).

Each variant named by a case is the one the host picks for it. The few-unit launches have at most
four waves' worth of units and the stealing launch one 64-sample unit per pixel. Every NEE case holds
misses and shadow rays of all three kinds -- proven to reach the light, traced and reached, traced and
blocked -- in non-zero numbers. The zero-component views give the oracle rays with an exactly zero
direction component that miss, zero d_z (the axis of a miss, prim 0's) among them, and between them
the cases' first hits lie on planes of all three axes."""
import numpy as np
import pytest

import guide_truth as gt
import lane_states_cases as lc


def test_cases_run_the_variants_they_name(spt, oracle):
    for family in lc.FAMILIES:
        prims, cam, p, kernel, _ = lc.family_case(spt, family)
        assert spt.select_kernel(prims, cam, p)["name"] == kernel, family
    for shape in list(lc.FEW_UNITS.values()) + [lc.STEAL, lc.FILM]:
        prims, cam, p, kernel, _ = lc.head_case(spt, shape)
        assert spt.select_kernel(prims, cam, p)["name"] == kernel, shape
    for label, prims, cam, p, kernel in lc.zero_cases(spt, oracle):
        assert spt.select_kernel(prims, cam, p)["name"] == kernel, label


def test_unit_counts(spt):
    """64 and 256 units of one sample: one wave's lanes, four waves' lanes. 3072 units of 64 samples:
    fewer units than an MI355X holds lanes (256 CUs x 256 or more), each long enough to be halved
    six times."""
    units = {k: lc.n_units(lc.head_case(spt, s)[2]) for k, s in lc.FEW_UNITS.items()}
    assert units == {"8x8_s1": 64, "16x8_s2": 256}
    p = lc.head_case(spt, lc.STEAL)[2]
    assert lc.n_units(p) == 64 * 48 < 256 * 256 and p.spp == 64


@pytest.mark.parametrize("family", [f for f, v in lc.FAMILIES.items() if v[4]])
def test_family_holds_every_shadow_outcome(spt, oracle, family):
    prims, cam, p, _, proof = lc.family_case(spt, family)
    _, st, n = lc.oracle_counts(oracle, prims, cam, p, proof)
    assert st["samples"] == p.width * p.height * p.spp
    assert min(n.values()) > 0, n


@pytest.mark.parametrize("shape", ["16x8_s2", "steal", "film"])
def test_head_shapes_hold_every_shadow_outcome(spt, oracle, shape):
    prims, cam, p, _, proof = lc.head_case(spt, dict(lc.FEW_UNITS, steal=lc.STEAL, film=lc.FILM)[shape])
    _, st, n = lc.oracle_counts(oracle, prims, cam, p, proof)
    assert min(n.values()) > 0, n


def test_smallest_launch_holds_paths_of_several_lengths(spt, oracle):
    """8x8 @ 1: 64 paths. They end at different vertices (so lanes go idle in different iterations)
    and some take a proven or a traced shadow ray."""
    prims, cam, p, _, proof = lc.head_case(spt, lc.FEW_UNITS["8x8_s1"])
    _, st, n = lc.oracle_counts(oracle, prims, cam, p, proof)
    assert st["samples"] == 64 and st["vertices"] > 2 * 64
    assert n["proven"] + n["reached"] + n["blocked"] > 0, n


def test_zero_views_miss_on_a_zero_d_a_and_hit_every_axis(spt, oracle):
    cases = lc.zero_cases(spt, oracle)
    assert len(cases) >= len(lc.ZERO_VIEWS) + 3
    zero_z_misses, zero_misses, axes = 0, 0, set()
    for label, prims, cam, p, _ in cases:
        o, d = gt.camera_rays(oracle, cam._c, p, np.arange(p.height), 0, p.spp, gt.unit_dirs(prims))
        d = d.reshape(-1, 3)
        _, ids = oracle.intersect_batch(prims, p, np.broadcast_to(o, d.shape).copy(), d)
        zero = (d == 0.0).any(axis=1)
        # (a ray with an exactly zero component misses the room's and the boxes' slabs, spt_device.h
        # rcp_nr; it can still hit the light, a rectangle of its own)
        if label.startswith("head:F2"):
            assert zero.any() and (ids[zero] < 0).any(), label
        zero_misses += int((zero & (ids < 0)).sum())
        zero_z_misses += int(((d[:, 2] == 0.0) & (ids < 0)).sum())
        axes |= {int(prims[i].kind) for i in np.unique(ids[ids >= 0])}
        oracle.zero_dir_counts()
        oracle.counter_render(prims, cam._c, p)
        traced, missed = oracle.zero_dir_counts()
        assert missed >= int((zero & (ids < 0)).sum()), label
    # prim 0 is an XY rectangle, so the plane axis a miss reports is z: d_a = +-0 at a miss
    assert all(c[1][0].kind == lc.rt.RECT_XY for c in cases)
    assert zero_z_misses > 0 and zero_misses > zero_z_misses
    assert axes >= {lc.rt.RECT_XY, lc.rt.RECT_XZ, lc.rt.RECT_YZ}

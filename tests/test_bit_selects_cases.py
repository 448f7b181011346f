"""The cases of tests/test_gpu_bit_selects.py are not vacuous (CPU: the oracle and the dispatch query).

Each variant named by a case is the one the host picks for it; every view's image differs from the
opposite view's; and the six views together put a first vertex on every one of the 17 rectangles,
the light among them, so every axis select is taken for every axis and both ways round."""
import numpy as np
import pytest

import bit_selects_cases as bc
import guide_truth as gt


@pytest.fixture(scope="module")
def view_images(spt, oracle):
    """The oracle's image of each view (the HEAD scene, const_nee_cam's case), computed once."""
    out = {}
    for view in bc.CAMERAS:
        prims, cam, p, _ = bc.view_case(spt, "const_nee_cam", view)
        out[view] = oracle.counter_render(prims, cam._c, p)[0]
    return out


def test_cases_run_the_variants_they_name(spt):
    for family in bc.VIEW_FAMILIES:
        for view in bc.CAMERAS:
            prims, cam, p, kernel = bc.view_case(spt, family, view)
            assert spt.select_kernel(prims, cam, p)["name"] == kernel, (family, view)
    for family in bc.REF_FAMILIES:
        prims, cam, p, kernel = bc.ref_case(spt, family)
        assert spt.select_kernel(prims, cam, p)["name"] == kernel, family
    for family in bc.DRAWS_FAMILIES:
        prims, cam, p, kernel = bc.draws_case(spt, family)
        assert spt.select_kernel(prims, cam, p)["name"] == kernel, family


@pytest.mark.parametrize("view", list(bc.CAMERAS))
def test_view_differs_from_its_opposite(view_images, view):
    a, b = view_images[view], view_images[bc.OPPOSITE[view]]
    assert a.shape == b.shape and not np.array_equal(a, b)
    assert np.isfinite(a).all() and a.max() > 0.0  # lit: the view is inside the room


def test_views_shade_every_rectangle_at_vertex_1(spt, oracle):
    """First hits of the six views' camera rays (guide_truth.camera_rays, oracle.intersect_batch):
    all 17 primitives of the HEAD scene, the light (prim 6) among them, and no ray misses."""
    seen = set()
    for view in bc.CAMERAS:
        prims, cam, p, _ = bc.view_case(spt, "const_nee_cam", view)
        o, d = gt.camera_rays(oracle, cam._c, p, np.arange(p.height), 0, p.spp, gt.unit_dirs(prims))
        d = d.reshape(-1, 3)
        _, ids = oracle.intersect_batch(prims, p, np.broadcast_to(o, d.shape).copy(), d)
        assert (ids >= 0).all(), view
        seen |= set(int(i) for i in np.unique(ids))
    assert seen == set(range(17)), sorted(set(range(17)) - seen)
    assert 6 in seen  # the light

"""The render loop's selects as bit operations on lane masks (spt_device.h: mask_lt, bsel, xor3;
spt_kernel.hip: axis_masks; spt_trace.h: box_keys): the hit's plane axis picks o_a, d_a, 1/d_a, the normal and the
NEE weight's |dl_a| through two masks made from the grouped position, a slab's exit is the xor of its
two keys and their min, and the azimuth's swap is a mask of one Philox bit.

Every render is compared bit for bit with the oracle's counter mode over all its pixels: the image
and every key of spt.STAT_KEYS, no tolerance (the contract is exact), and the variant that ran is the
one the case means. The cases (tests/bit_selects_cases.py) take every substituted select both ways for
every axis; tests/test_bit_selects_cases.py shows on the CPU that they do."""
import numpy as np
import pytest

import bit_selects_cases as bc

pytestmark = pytest.mark.gpu


def _check(spt, oracle, prims, cam, p, kernel):
    gpu, st = spt.render(prims, cam, p, return_stats=True)
    pixels = np.arange(p.width * p.height, dtype=np.uint32)
    cpu, cst = oracle.counter_render_pixels(prims, cam._c, p, pixels)
    assert st["kernel"] == kernel
    assert gpu.shape == (p.height, p.width, 3)
    assert np.array_equal(gpu.reshape(-1, 3), cpu)
    for k in spt.STAT_KEYS:
        assert st[k] == cst[k], (k, st[k], cst[k])
    assert st["samples"] == len(pixels) * p.spp


@pytest.mark.parametrize("view", list(bc.CAMERAS))
@pytest.mark.parametrize("family", list(bc.VIEW_FAMILIES))
def test_axis_views(spt, oracle, family, view):
    """16x12 @ 8 from inside the room along +-x, +-y, +-z, slightly off axis."""
    _check(spt, oracle, *bc.view_case(spt, family, view))


@pytest.mark.parametrize("family", list(bc.REF_FAMILIES))
def test_reference_camera(spt, oracle, family):
    """24x18 @ 16 from the reference camera: the literal kernels and the uploaded-geometry ones."""
    _check(spt, oracle, *bc.ref_case(spt, family))


@pytest.mark.parametrize("family", list(bc.DRAWS_FAMILIES))
def test_many_draws(spt, oracle, family):
    """3x1 @ 2048 per kernel with literal geometry: the swap and camera masks over many draws."""
    _check(spt, oracle, *bc.draws_case(spt, family))

"""The rays of tests/test_gpu_axis_positions.py are not vacuous: counted with the oracle alone, on the
CPU, each origin's set holds at least 32 rays whose two nearest candidates lie on planes of different
axes and agree in the upper 26 bits of t -- the only place a key's position bits decide between axes."""
import numpy as np
import pytest

import axis_positions_cases as ac


@pytest.mark.parametrize("oi", range(len(ac.ORIGINS)))
def test_axis_ties_are_there(spt, oracle, oi):
    prims = spt.cornell_scene()
    origin = ac.ORIGINS[oi]
    rays = ac.rays(spt, oracle, prims, origin)
    assert len(rays) == 7 * (8 + 12 + 2 * (8 + 4))
    d = ac.traced_dirs(spt, oracle, origin, [t for _, t in rays])
    ties = ac.axis_ties(spt, oracle, prims, origin, d)
    assert int(ties.sum()) >= 32
    o = np.broadcast_to(np.asarray(origin, np.float32), d.shape).copy()
    _, ids = oracle.intersect_batch(prims, spt.default_params(), o, d)
    won = set(ids[ties].tolist()) - {-1}
    assert len(won) >= 4 and len({prims[i].kind for i in won}) >= 2  # walls, box faces and tops win ties

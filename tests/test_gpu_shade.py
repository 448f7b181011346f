"""The tables of tests/test_contract_shade.py rendered by the library's kernels and compared with the
float64 truth (tests/shade_truth.py) directly, not through the oracle: the same conditions, the same
bounds. The CPU file checks first that no table is vacuous.

Each variant is reached and asserted from the launch itself. Family A at max_depth = 2: const,
cornell, rectdiff, sphdiff_nee, sphdiff, generic. The kernels compiled for max_depth = 0 (const_nee,
const_cos, upbox_nee, uplight_nee, rectdiff_nee) render the same tables uncapped: the Philox words
do not depend on max_depth, so the first two vertices are the capped render's, and every pixel whose
samples end by themselves at their second vertex (the black light: RR with p = 0) must equal the
truth within its bound -- except exactly the pixels that took the self-hit alternative in the capped
render, whose paths go on from their own wall. Family B: generic and the wide-sphere kernel.
"""
import numpy as np
import pytest

import shade_truth as stt

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(stt.A_CASES))
def test_gpu_family_a_direct_light(spt, oracle, case):
    prims, cam, p = stt.a_case(spt, case)
    R = stt.truth(oracle, ("A", case), prims, cam, p)
    img, st = spt.render(prims, cam, p, return_stats=True)
    assert st["kernel"] == stt.A_CASES[case][2]
    fig = stt.check_a(R, p, img, f"gpu {case} ({st['kernel']})")
    assert fig["lit"] >= 50
    assert fig["excluded"] <= 0.02
    assert fig["neither"] == 0
    assert fig["alt_share"] <= 0.03
    assert (0.02 if p.nee_prob > 0 else 0.0) <= fig["ratio"] <= 1.0
    uncapped = stt.A_CASES[case][3]
    if uncapped is None:
        return
    prims, cam, p0 = stt.a_case(spt, case, max_depth=0)
    img0, st0 = spt.render(prims, cam, p0, return_stats=True)
    assert st0["kernel"] == uncapped
    got = img0.astype(np.float64).reshape(-1, 3)
    closed = fig["keep"] & fig["closed"]
    off = closed & ~(np.abs(got - fig["value"]) <= fig["bound"]).all(axis=1)
    lit = closed & (fig["value"] > 0).any(axis=1)
    print(f"gpu {case} ({uncapped}, uncapped): {int(closed.sum())} closed pixels, {int(lit.sum())} of them lit, "
          f"{int(off.sum())} off the truth, {len(fig['alt_pixels'])} alternative pixels in the capped render")
    assert lit.sum() >= 50
    assert set(np.flatnonzero(off)) <= set(fig["alt_pixels"])


def test_gpu_family_a_clamp(spt, oracle):
    prims, cam, p = stt.a_case(spt, "head-wrap-s1", emission=12.0)
    R = stt.truth(oracle, ("A", "clamp"), prims, cam, p)
    img, st = spt.render(prims, cam, p, return_stats=True)
    assert st["kernel"] == "const"
    got = img.astype(np.float64).reshape(-1, 3)
    over = (R.L >= 1.0 + R.bound_unclamped) & (R.margin > stt.MARGIN)[:, None]
    assert over.sum() >= 300
    fig = stt.check_a(R, p, img, "gpu clamp")
    over[fig["alt_pixels"]] = False  # a self-hit sample (counted below) has its alternative's value
    assert np.all(got[over] == 1.0)
    assert fig["neither"] == 0 and fig["excluded"] <= 0.02 and fig["alt_share"] <= 0.03


@pytest.mark.parametrize("name,max_depth,rr_depth,spp,seed", stt.B_CASES)
def test_gpu_family_b_specular_tree(spt, oracle, name, max_depth, rr_depth, spp, seed):
    prims, cam, p = stt.b_case(spt, name, max_depth, rr_depth, spp, seed)
    R = stt.truth(oracle, ("B", name, max_depth, rr_depth, spp, seed), prims, cam, p)
    img, st = spt.render(prims, cam, p, return_stats=True)
    assert st["kernel"] == stt.B_SCENES[name]
    fig = stt.check_b(R, p, img, f"gpu {name} depth {max_depth} rr {rr_depth} spp {spp} seed {seed}")
    assert fig["excluded"] <= 0.02
    assert fig["n_glass"] >= 60
    assert fig["bad"] == 0
    assert fig["wall"] <= 2.0 ** -24 and fig["wall_ratio"] <= 1.0
    assert fig["mirror_ratio"] <= 1.0
    assert 0.02 <= fig["glass_ratio"] <= 1.0

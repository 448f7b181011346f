"""The shading step of the contract -- what happens between a hit and the next ray -- against a
float64 replay of the estimator (tests/shade_truth.py), sample by sample, on the CPU oracle.
tests/test_gpu_shade.py sends the same tables through the library's kernels.

Family A, direct light: 64 x 48, max_depth = 2, the light's emission 12/16 (1, .5, .25) so that no
sample clamps; one table per row of shade_truth.A_CASES. Every sample equals the truth within its
bound, or equals the truth's value had the first vertex's shadow ray been stopped by the vertex's own
wall (the reference's self-hit, DESIGN.md section 3: the scatter ray of :468 is then taken and ends
on the same wall, or goes on). Alternative matches are at most 3 % of the samples the light
contributes to and none on a sphere (the truth offers none there); margins below 1e-3 are excluded, at most 2 % per table.

Family B, the specular tree: 48 x 32, every wall black and emitting a colour of its own, the mirror
and glass balls as shipped, in the Cornell room (generic kernel) and in the 1e5-sphere box (wide
kernel); max_depth 2, 3, 4, 6 and uncapped with rr_depth = 3.

The bound is a function of the sample (shade_truth.sample_values): each vertex displaced by its
ray_truth.t_bound along the incoming ray and by the roundings of x = o + d t across it, the truth
re-evaluated, the changes summed; 2^-24 per fp32 rounding on the longest chain; 2^-31 per sample.
Where a displacement flips a decision of the sample (a sphere vertex whose shadow ray leaves at a
grazing angle: moved inside by t_bound, its own far root passes the 2e-3 epsilon) the bound spans
both outcomes; such samples pass, are counted and stay out of the err / bound figure.

Measured on the CPU oracle (the MI355X kernels give the same figures, profiles/r20_gpu_shade.txt):
family A max err / bound 0.13-0.24 per table (max relative error 2.3e-5 at 1 spp on rectangles, up to
1.7e-4 on spheres32 at 4 spp), 0.6-0.9 % of the samples excluded, alternative matches 0.7-2.1 % of
the samples the light contributes to, none fits neither; family B glass 0.09-0.19 (max error 1.5e-5
at depth 2, 3.0e-5 at 3, 6.2e-5 at 4, 6.1e-5 at 6 and uncapped: it does not grow), mirror up to 0.15,
walls 0.010-0.017 (the 1.31 floor: 2.4e-8), 0.3-0.4 % excluded. Before contract v8 (the mirror
direction not renormalised) the glass failed from max_depth 5 on: 7-40 samples per table beyond the
bound at depth 6, by up to 0.07 (err / bound up to 2400).
"""
import numpy as np
import pytest

import shade_truth as stt


@pytest.mark.parametrize("case", list(stt.A_CASES))
def test_family_a_direct_light(spt, oracle, case):
    prims, cam, p = stt.a_case(spt, case)
    assert spt.select_kernel(prims, cam, p)["name"] == stt.A_CASES[case][2]
    R = stt.truth(oracle, ("A", case), prims, cam, p)
    img, _ = oracle.counter_render(prims, cam._c, p)
    fig = stt.check_a(R, p, img, case)
    assert fig["lit"] >= 50 and (fig["reach"] >= 50 or p.nee_prob <= 0), "the table is vacuous"
    assert fig["excluded"] <= 0.02
    assert fig["neither"] == 0
    assert fig["alt_share"] <= 0.03
    # (none of them on a sphere: the truth offers no alternative there, shade_truth.sample_values)
    # a cosine-only table holds no arithmetic but T f e, exact in these scenes: its decisions are the test
    assert (0.02 if p.nee_prob > 0 else 0.0) <= fig["ratio"] <= 1.0


def test_family_a_clamp(spt, oracle):
    """The shipped emission 12 at 1 spp: exactly 1.0 wherever the truth's L >= 1 by more than its
    bound (the 1.31 fixed point's clamp); the other samples as in family A."""
    prims, cam, p = stt.a_case(spt, "head-wrap-s1", emission=12.0)
    R = stt.truth(oracle, ("A", "clamp"), prims, cam, p)
    img, _ = oracle.counter_render(prims, cam._c, p)
    got = img.astype(np.float64).reshape(-1, 3)
    keep = R.margin > stt.MARGIN
    over = (R.L >= 1.0 + R.bound_unclamped) & keep[:, None]  # spp = 1: L / spp = L
    print(f"clamp: {int(over.sum())} channel values with L >= 1 + its bound, max L {R.L.max():.2f}")
    assert over.sum() >= 300
    fig = stt.check_a(R, p, img, "clamp")
    over[fig["alt_pixels"]] = False  # a self-hit sample (counted below) has its alternative's value
    assert np.all(got[over] == 1.0)
    assert fig["neither"] == 0 and fig["excluded"] <= 0.02 and fig["alt_share"] <= 0.03


@pytest.mark.parametrize("name,max_depth,rr_depth,spp,seed", stt.B_CASES)
def test_family_b_specular_tree(spt, oracle, name, max_depth, rr_depth, spp, seed):
    prims, cam, p = stt.b_case(spt, name, max_depth, rr_depth, spp, seed)
    assert spt.select_kernel(prims, cam, p)["name"] == stt.B_SCENES[name]
    R = stt.truth(oracle, ("B", name, max_depth, rr_depth, spp, seed), prims, cam, p)
    img, _ = oracle.counter_render(prims, cam._c, p)
    fig = stt.check_b(R, p, img, f"{name} depth {max_depth} rr {rr_depth} spp {spp} seed {seed}")
    assert fig["excluded"] <= 0.02
    assert fig["n_glass"] >= 60
    if max_depth == 0 or max_depth >= 4:  # enter, reflect inside, leave, reach a wall: four vertices
        assert fig["internal_exit"] >= 40, "no glass path reflects inside the ball and leaves it"
    assert fig["bad"] == 0
    assert fig["wall"] <= 2.0 ** -24 and fig["wall_ratio"] <= 1.0
    assert fig["mirror_ratio"] <= 1.0
    assert 0.02 <= fig["glass_ratio"] <= 1.0

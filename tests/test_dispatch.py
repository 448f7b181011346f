"""Which render kernel runs: spt_select_kernel (a pure host function, no device) against a table of
(scene, camera, params) -> the variant's name, written out as literals.

Every variant computes the same contract bit for bit, so the parity tests cannot see a scene that
silently falls back to a less specialised kernel, nor a variant that nothing reaches: this table
can. tests/test_gpu_parity.py renders one row per name (ONE_PER_NAME) and checks that the launch
ran what the query said.
"""
import numpy as np
import pytest

TILTED = dict(lookfrom=(40, 55, 160), lookat=(55, 35, 10), vup=(0.1, 1, 0))
W, H, SPP = 48, 36, 8
LEAKS = 4  # SPT_FLAG_REFERENCE_LEAKS
UNIFORM = 1  # SPT_FLAG_UNIFORM_SCATTER

# Every name of spt_kernel_name(), in the enum's order.
KERNEL_NAMES = [
    "generic", "cornell", "const", "const_nee", "const_cos", "sphdiff", "wide", "sphdiff_nee",
    "rectdiff", "const_nee_ref", "const_cos_ref", "sphdiff_nee_ref", "cornell_nee", "cornell_cos",
    "rectdiff_nee", "rectdiff_cos", "upbox_nee", "upbox_cos", "const_nee_cam", "const_cos_cam",
    "upbox_nee_cam", "upbox_cos_cam", "uplight_nee", "uplight_cos", "uplight_nee_cam",
    "uplight_cos_cam"]


def recoloured(spt, prims):
    """Materials only: the light's emission 15 (:294) and a blue left wall (:290)."""
    out = [spt.spt_prim.from_buffer_copy(p) for p in prims]
    for i in range(3):
        out[6].e[i] = 15.0
    out[2].c[0], out[2].c[1], out[2].c[2] = 0.25, 0.25, 0.75
    return out


def neg_zero_walls(spt, front=False, floor=False):
    """The HEAD scene with the front wall's plane (prim 0, z = 0) and / or the floor's (prim 4,
    y = 0) at -0.0: the same planes, another bit pattern."""
    out = [spt.spt_prim.from_buffer_copy(p) for p in spt.cornell_scene()]
    if front:
        out[0].geom[4] = -0.0
    if floor:
        out[4].geom[4] = -0.0
    return out


NEG_ZERO = [dict(front=True), dict(floor=True), dict(front=True, floor=True)]


def scene(spt, name):
    import test_oracle as to

    head = spt.cornell_scene()
    if name == "head":
        return head
    if name == "mats":
        return recoloured(spt, head)
    if name == "spec":  # the short box's front face a mirror
        head[12].refl = spt.SPEC
        return head
    if name == "movebox":
        return spt.move_short_box(head, 1.0)
    if name.startswith("edit_lr"):
        return to.edited_scene(spt, **to.EDITS_LR[int(name[-1])][0])
    if name == "dropbox":
        return spt.drop_short_box(head)
    return getattr(spt, name + "_scene")()  # spheres32, smallpt_classic, smallpt_mirror_glass


def camera(spt, tilted):
    return spt.Camera(aspect=W / H, **(TILTED if tilted else {}))


def params(spt, level="auto", flags=0, **kw):
    return spt.default_params(width=W, height=H, spp=SPP, seed=31,
                              flags=flags | spt.kernel_flag(level), **kw)


NEE, COS = dict(nee_prob=1.0), dict(nee_prob=0.0)
SPH = dict(max_depth=16)

# (scene, tilted camera, params, expected variant)
TABLE = [
    ("head", False, dict(**NEE), "const_nee"),
    ("head", False, dict(**COS), "const_cos"),
    ("head", False, dict(flags=LEAKS, **NEE), "const_nee_ref"),
    ("head", False, dict(flags=LEAKS, **COS), "const_cos_ref"),
    ("head", True, dict(**NEE), "const_nee_cam"),
    ("head", True, dict(**COS), "const_cos_cam"),
    ("head", True, dict(flags=LEAKS, **NEE), "const"),
    ("head", True, dict(flags=LEAKS, **COS), "const"),
    # one parameter off the reference's estimator
    ("head", False, dict(nee_prob=0.5), "const"),
    ("head", False, dict(light_mode=1), "const"),
    ("head", False, dict(rr_depth=4), "const"),
    ("head", False, dict(max_depth=3), "const"),
    ("head", False, dict(light_x0=40.0), "const"),
    # the level cap
    ("head", False, dict(level="const", **NEE), "const"),
    ("head", False, dict(level="const", **COS), "const"),
    ("head", False, dict(level="cornell"), "cornell"),
    ("head", False, dict(level="generic"), "generic"),
    ("head", False, dict(flags=UNIFORM), "generic"),
    ("spec", False, dict(), "generic"),
    ("mats", False, dict(**NEE), "const_nee"),
    # the short box moved: the room and light literal, the boxes uploaded
    ("movebox", False, dict(**NEE), "upbox_nee"),
    ("movebox", False, dict(**COS), "upbox_cos"),
    ("movebox", True, dict(**NEE), "upbox_nee_cam"),
    ("movebox", True, dict(**COS), "upbox_cos_cam"),
    ("movebox", False, dict(level="const", **NEE), "cornell_nee"),
    ("movebox", False, dict(level="const", **COS), "cornell_cos"),
    ("movebox", False, dict(flags=LEAKS), "cornell"),
    ("movebox", True, dict(level="const"), "cornell"),
    # the light edited, the room HEAD's
    ("edit_lr0", False, dict(**NEE), "uplight_nee"),
    ("edit_lr0", False, dict(**COS), "uplight_cos"),
    ("edit_lr1", False, dict(**NEE), "uplight_nee"),
    ("edit_lr1", False, dict(**COS), "uplight_cos"),
    ("edit_lr0", True, dict(**NEE), "uplight_nee_cam"),
    ("edit_lr0", True, dict(**COS), "uplight_cos_cam"),
    ("edit_lr1", True, dict(**NEE), "uplight_nee_cam"),
    ("edit_lr1", True, dict(**COS), "uplight_cos_cam"),
    # the room edited: everything uploaded
    ("edit_lr2", False, dict(**NEE), "cornell_nee"),
    ("edit_lr2", False, dict(**COS), "cornell_cos"),
    ("edit_lr3", False, dict(**NEE), "cornell_nee"),
    ("edit_lr3", False, dict(**COS), "cornell_cos"),
    ("edit_lr2", True, dict(), "cornell"),
    ("edit_lr3", True, dict(), "cornell"),
    # another rect-only topology
    ("dropbox", False, dict(**NEE), "rectdiff_nee"),
    ("dropbox", False, dict(**COS), "rectdiff_cos"),
    ("dropbox", False, dict(level="cornell"), "rectdiff"),
    ("dropbox", False, dict(nee_prob=0.5), "rectdiff"),
    ("dropbox", False, dict(flags=LEAKS), "rectdiff"),
    ("dropbox", True, dict(), "rectdiff"),
    ("dropbox", False, dict(level="generic"), "generic"),
    # spheres
    ("spheres32", False, dict(**SPH, **NEE), "sphdiff_nee"),
    ("spheres32", False, dict(flags=LEAKS, **SPH), "sphdiff_nee_ref"),
    ("spheres32", False, dict(**SPH, **COS), "sphdiff"),
    ("spheres32", False, dict(level="const", **SPH), "sphdiff"),
    ("spheres32", False, dict(flags=UNIFORM, **SPH), "generic"),
    # wide (fp64) spheres: one kernel, whatever the params
    ("smallpt_classic", False, dict(**COS), "wide"),
    ("smallpt_classic", False, dict(light_id=8, **NEE), "wide"),
    ("smallpt_classic", True, dict(level="generic", **COS), "wide"),
    ("smallpt_mirror_glass", False, dict(**COS), "wide"),
    ("smallpt_mirror_glass", False, dict(flags=LEAKS, max_depth=6, **COS), "wide"),
]

# The first row of the table that reaches each name: the GPU matrix renders these.
ONE_PER_NAME = {}
for _row in TABLE:
    ONE_PER_NAME.setdefault(_row[3], _row)


def recipe(spt, row):
    """(prims, camera, params) of a table row."""
    name, tilted, kw, _ = row
    return scene(spt, name), camera(spt, tilted), params(spt, **kw)


def _row_id(row):
    name, tilted, kw, want = row
    return "-".join([name, "tilted" if tilted else "axis"] + [f"{k}={v}" for k, v in kw.items()]
                    + [want])


def test_name_table_is_the_librarys(spt):
    lib = spt.load_library()
    assert lib.spt_kernel_count() == len(KERNEL_NAMES)
    assert spt.kernel_names() == KERNEL_NAMES
    assert lib.spt_kernel_name(-1) is None and lib.spt_kernel_name(len(KERNEL_NAMES)) is None


@pytest.mark.parametrize("row", TABLE, ids=_row_id)
def test_dispatch_table(spt, row):
    prims, cam, p = recipe(spt, row)
    got = spt.select_kernel(prims, cam, p)
    assert got["name"] == row[3]
    assert spt.kernel_names()[got["id"]] == got["name"]


def test_table_reaches_every_variant(spt):
    """A variant added without a row here (or one no scene can reach) fails."""
    reached = {spt.select_kernel(*recipe(spt, row))["name"] for row in TABLE}
    assert reached == set(spt.kernel_names())
    assert sorted(ONE_PER_NAME) == sorted(KERNEL_NAMES)


def test_select_kernel_validates_like_a_render(spt):
    cam = camera(spt, False)
    with pytest.raises(spt.SptError) as e:
        spt.select_kernel(spt.cornell_scene(), cam, spt.default_params(width=0))
    assert e.value.status == 1
    with pytest.raises(spt.SptError) as e:  # NEE at a light that does not emit
        spt.select_kernel(spt.smallpt_classic_scene(), cam, params(spt))
    assert e.value.status == 1 and "light" in spt.load_library().spt_last_error().decode()
    lib = spt.load_library()
    assert lib.spt_select_kernel(None, 0, None, None, None) == 1


@pytest.mark.parametrize("level", ["auto", "const"])
def test_early_resolve_flag_follows_the_clause_margins(spt, level):
    """The uploaded-geometry NEE kernels resolve shadow rays early exactly where early_geo_setup
    finds the scene inside its margins: test_oracle.EDITS_LR's `on` column; every box edit of
    EDITS."""
    import test_oracle as to

    cam = camera(spt, False)
    for kw, on in to.EDITS_LR:
        got = spt.select_kernel(to.edited_scene(spt, **kw), cam, params(spt, level=level))
        assert got["early_resolve"] == on, (kw, got)
        assert got["name"].endswith("_nee"), (kw, got)
    for kw in to.EDITS:
        got = spt.select_kernel(to._move_boxes(spt, **kw), cam, params(spt, level=level))
        assert got["early_resolve"] and got["name"] == ("upbox_nee" if level == "auto" else "cornell_nee")


def test_early_resolve_flag_other_kernels(spt):
    cam = camera(spt, False)
    head = spt.cornell_scene()
    assert spt.select_kernel(head, cam, params(spt))["early_resolve"]  # the literal clauses
    assert spt.select_kernel(head, cam, params(spt, flags=LEAKS))["early_resolve"]
    assert spt.select_kernel(head, camera(spt, True), params(spt))["early_resolve"]
    for kw in (dict(**COS), dict(level="const"), dict(level="generic"), dict(nee_prob=0.5)):
        assert not spt.select_kernel(head, cam, params(spt, **kw))["early_resolve"], kw
    assert not spt.select_kernel(spt.drop_short_box(head), cam, params(spt))["early_resolve"]
    sph = spt.spheres32_scene()
    assert spt.select_kernel(sph, cam, params(spt, **SPH))["early_resolve"]
    assert spt.select_kernel(sph, cam, params(spt, flags=LEAKS, **SPH))["early_resolve"]
    assert not spt.select_kernel(sph, cam, params(spt, **SPH, **COS))["early_resolve"]


def test_early_resolve_flag_low_sphere_scenes(spt):
    """The sphere kernel's threshold needs every sphere centre within 190 of every room corner (the
    scenes of test_gpu_parity.test_early_nee_resolve_random_low_spheres): on iff `near`."""
    import test_gpu_parity as tg

    seen = set()
    for seed in tg.LOW_SPHERE_SEEDS:
        prims, near, _ = tg.low_sphere_scene(spt, seed)
        got = spt.select_kernel(prims, camera(spt, False), params(spt, max_depth=12))
        assert got["name"] == "sphdiff_nee" and got["early_resolve"] == near, (seed, near, got)
        seen.add(near)
    assert seen == {True, False}  # both outcomes occur among the seeds


@pytest.mark.parametrize("walls", NEG_ZERO, ids=["front", "floor", "both"])
@pytest.mark.parametrize("level", ["auto", "const"])
def test_negative_zero_walls_keep_their_clause(spt, walls, level):
    """A room wall at -0.0 is the same plane as HEAD's with other bits: not the literal room
    (memcmp), so the uploaded-geometry NEE kernel, with its room clause on (lo normalised to +0)."""
    got = spt.select_kernel(neg_zero_walls(spt, **walls), camera(spt, False), params(spt, level=level))
    assert got == dict(id=KERNEL_NAMES.index("cornell_nee"), name="cornell_nee", leak_end=1,
                       early_resolve=True)


def test_leak_end_flag(spt):
    cam = camera(spt, False)
    head = spt.cornell_scene()
    assert spt.select_kernel(head, cam, params(spt))["leak_end"] == 1
    assert spt.select_kernel(head, cam, params(spt, flags=LEAKS))["leak_end"] == 0
    # test_gpu_parity.test_leak_end_off_when_the_miss_vertex_emits: an emitting prim 0
    lit = [spt.spt_prim.from_buffer_copy(p) for p in head]
    lit[0].e[:] = [0.05, 0.05, 0.05]
    for est in (NEE, COS):
        got = spt.select_kernel(lit, cam, params(spt, **est))
        assert got["leak_end"] == 0 and got["name"] == ("const_nee_ref" if est is NEE else "const_cos_ref")


def test_query_does_not_depend_on_image_size_or_sharding(spt):
    """The choice is a function of scene, camera and estimator: a shard, a chunk size or another
    resolution asks for the same kernel (the shard reassembly tests rely on it)."""
    prims = spt.move_short_box(spt.cornell_scene(), 1.0)
    want = spt.select_kernel(prims, camera(spt, False), params(spt))
    for kw in (dict(width=2, height=2, spp=2048, chunk=2048), dict(width=1024, height=768, spp=512),
               dict(width=16, height=20, shard_index=2, shard_count=3, tile_rows=4)):
        p = spt.default_params(**kw)
        cam = spt.Camera(aspect=float(np.float32(p.width) / np.float32(p.height)))
        assert spt.select_kernel(prims, cam, p) == want, kw

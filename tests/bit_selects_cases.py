"""The cases of tests/test_gpu_bit_selects.py and their non-vacuity check (a helper, not a test).

The render loop's selects on the hit's plane axis, the slab exits, the azimuth's swap and the resolve
are bit operations on lane masks (spt_device.h: mask_lt, bsel, xor3). A select that is wrong for one
axis or one sign shows only where that axis is shaded facing that way, and the reference camera never
looks at the front wall or down an axis. So six cameras stand inside the room and look along +-x,
+-y, +-z, slightly off axis (the any-camera kernels), each from where it sees the box faces that
face it; together they put a first vertex on every one of the 17 rectangles, the light among them
(tests/test_bit_selects_cases.py).
"""
LEAKS = 4  # SPT_FLAG_REFERENCE_LEAKS

# name -> Camera kwargs. The room is x 1..99, y 0..81.6, z 0..170; the tall box x 12..42, z 32..62,
# y <= 50; the short box x, z 63..88, y <= 25; the light x 32..68, z 63..96 at y 81.5.
CAMERAS = {
    "+x": dict(lookfrom=(5, 20, 64), lookat=(60, 22, 66), vup=(0, 1, 0)),
    "-x": dict(lookfrom=(95, 12, 62), lookat=(40, 14, 58), vup=(0, 1, 0)),
    "+y": dict(lookfrom=(50, 10, 75), lookat=(52, 70, 78), vup=(0, 0, -1)),
    "-y": dict(lookfrom=(52, 78, 60), lookat=(50, 10, 63), vup=(0, 0, -1)),
    "+z": dict(lookfrom=(50, 20, 5), lookat=(53, 22, 90), vup=(0, 1, 0)),
    "-z": dict(lookfrom=(52, 30, 165), lookat=(49, 28, 60), vup=(0, 1, 0)),
}
OPPOSITE = {"+x": "-x", "-x": "+x", "+y": "-y", "-y": "+y", "+z": "-z", "-z": "+z"}
VIEW_SHAPE = dict(width=16, height=12, spp=8)

# family -> (scene, spt_params fields, kernel cap, the variant an off-axis camera runs)
VIEW_FAMILIES = {
    "const_nee_cam": ("head", dict(), "auto", "const_nee_cam"),
    "const_cos_cam": ("head", dict(nee_prob=0.0), "auto", "const_cos_cam"),
    "upbox_nee_cam": ("moved", dict(), "auto", "upbox_nee_cam"),
    "uplight_nee_cam": ("light", dict(), "auto", "uplight_nee_cam"),
}

# the reference camera: family -> (scene, spt_params fields, flags, kernel cap, the variant)
REF_SHAPE = dict(width=24, height=18, spp=16)
REF_FAMILIES = {
    "const_nee": ("head", dict(), 0, "auto", "const_nee"),
    "const_cos": ("head", dict(nee_prob=0.0), 0, "auto", "const_cos"),
    "const_nee_ref": ("head", dict(), LEAKS, "auto", "const_nee_ref"),
    "cornell_nee": ("moved", dict(), 0, "const", "cornell_nee"),
    "rectdiff_nee": ("nobox", dict(), 0, "auto", "rectdiff_nee"),
    "generic": ("specular", dict(), 0, "auto", "generic"),
}

# many draws of few pixels, one case per kernel with literal geometry: the swap and camera masks
# (family -> (spt_params fields, flags, kernel cap, off-axis camera?, the variant))
DRAWS_SHAPE = dict(width=3, height=1, spp=2048)
DRAWS_FAMILIES = {
    "const": (dict(), 0, "const", False, "const"),
    "const_nee": (dict(), 0, "auto", False, "const_nee"),
    "const_cos": (dict(nee_prob=0.0), 0, "auto", False, "const_cos"),
    "const_nee_ref": (dict(), LEAKS, "auto", False, "const_nee_ref"),
    "const_cos_ref": (dict(nee_prob=0.0), LEAKS, "auto", False, "const_cos_ref"),
    "const_nee_cam": (dict(), 0, "auto", True, "const_nee_cam"),
    "const_cos_cam": (dict(nee_prob=0.0), 0, "auto", True, "const_cos_cam"),
}


def scene(spt, name):
    head = spt.cornell_scene()
    if name == "head":
        return head
    if name == "moved":
        return spt.move_short_box(head, 3.0)
    if name == "light":
        return spt.edit_light(head, x=(30, 66), z=(65, 99))
    if name == "nobox":
        return spt.drop_short_box(head)
    return spt.cornell_specular_scene()


def camera(spt, name, shape):
    return spt.Camera(aspect=shape["width"] / shape["height"], **CAMERAS[name])


def view_case(spt, family, view):
    sc, pkw, level, kernel = VIEW_FAMILIES[family]
    p = spt.default_params(seed=7, device=0, flags=spt.kernel_flag(level), **dict(VIEW_SHAPE, **pkw))
    return scene(spt, sc), camera(spt, view, VIEW_SHAPE), p, kernel


def ref_case(spt, family):
    sc, pkw, flags, level, kernel = REF_FAMILIES[family]
    p = spt.default_params(seed=7, device=0, flags=flags | spt.kernel_flag(level), **dict(REF_SHAPE, **pkw))
    return scene(spt, sc), spt.Camera(aspect=REF_SHAPE["width"] / REF_SHAPE["height"]), p, kernel


def draws_case(spt, family):
    pkw, flags, level, offaxis, kernel = DRAWS_FAMILIES[family]
    p = spt.default_params(seed=7, device=0, flags=flags | spt.kernel_flag(level), **dict(DRAWS_SHAPE, **pkw))
    aspect = DRAWS_SHAPE["width"] / DRAWS_SHAPE["height"]
    cam = camera(spt, "-z", DRAWS_SHAPE) if offaxis else spt.Camera(aspect=aspect)
    return spt.cornell_scene(), cam, p, kernel

"""The cases of tests/test_gpu_lane_states.py and their non-vacuity check (a helper, not a test).

The render loop keeps one state word per lane (spt_kernel.hip, LaneStates). Its guards are single
compares on that word, the traced shadow lanes' mask and the light compare are taken once per
iteration and combined on the scalar unit, the camera / cosine select is a bit select on the mask
ls - 1, and the literal leak-end kernels take the normal's sign from the sign bit of d_a. A wrong
state value shows where lanes are idle from the first iteration, where idle lanes steal, and across
launches; a wrong mask where shadow rays are proven, traced and reached, traced and blocked in the
same wave; the sign where a ray runs parallel to a plane.
"""
import numpy as np

import ray_truth as rt

LEAKS = 4  # SPT_FLAG_REFERENCE_LEAKS
TILTED = dict(lookfrom=(40, 55, 160), lookat=(55, 35, 10), vup=(0.1, 1, 0))

# ---- every kernel family the change touches, 64x48 @ 16 from the reference camera (tilted: any camera)
FAMILY_SHAPE = dict(width=64, height=48, spp=16)
# family -> (scene, spt_params fields, camera kwargs, the variant, oracle proof mode or None)
FAMILIES = {
    "head_nee": ("head", dict(), {}, "const_nee", "literal"),
    "head_cos": ("head", dict(nee_prob=0.0), {}, "const_cos", None),
    "moved_box": ("moved", dict(), {}, "upbox_nee", "edited"),
    "edited_light": ("light", dict(), {}, "uplight_nee", None),
    "tilted": ("head", dict(), TILTED, "const_nee_cam", "literal"),
    "generic": ("specular", dict(), {}, "generic", None),
    "spheres": ("spheres32", dict(), {}, "sphdiff_nee", None),
}

# ---- launches with fewer work units than one wave, or a few waves, has lanes: most lanes are idle
# from the first iteration and every wave ends through the empty last iteration
FEW_UNITS = {
    "8x8_s1": dict(width=8, height=8, spp=1, chunk=1),
    "16x8_s2": dict(width=16, height=8, spp=2, chunk=1),
}
# ---- one unit of 64 samples per pixel, 3072 units: an MI355X holds more lanes than that, the queue
# is dry at once and idle lanes take halves of busy lanes' ranges all the way down
STEAL = dict(width=64, height=48, spp=64, chunk=64)
# ---- two windows of 8 samples through a film, the second over a pixel list
FILM = dict(width=64, height=48, spp=16)
FILM_BATCH = 8

# ---- rays parallel to planes (raw cameras, tests/ray_truth.py): fans and single rays with one exactly
# zero direction component from mid-room, and fans from origins exactly on faces of the moved box
ZERO_VIEWS = ("F2_o0_d6", "F2_o1_d2", "F2_fan_x", "F2_fan_y", "F2_fan_z_light")
ZERO_SPP = 8


def scene(spt, name):
    head = spt.cornell_scene()
    if name == "head":
        return head
    if name == "moved":
        return spt.move_short_box(head, 3.0)
    if name == "light":
        return spt.edit_light(head, x=(30, 66), z=(65, 99))
    if name == "spheres32":
        return spt.spheres32_scene()
    return spt.cornell_specular_scene()


def params(spt, **kw):
    return spt.default_params(seed=7, device=0, **kw)


def family_case(spt, family):
    sc, pkw, camkw, kernel, proof = FAMILIES[family]
    p = params(spt, **dict(FAMILY_SHAPE, **pkw))
    cam = spt.Camera(aspect=p.width / p.height, **camkw)
    return scene(spt, sc), cam, p, kernel, proof


def head_case(spt, shape):
    """The HEAD scene from the reference camera at `shape` (the literal NEE kernel)."""
    p = params(spt, **shape)
    return spt.cornell_scene(), spt.Camera(aspect=p.width / p.height), p, "const_nee", "literal"


def raw_camera(spt, origin, L, hor, ver):
    """A camera from raw vectors: origin, lower_left_corner = origin + L, horizontal, vertical."""
    cam = spt.Camera()
    for i in range(3):
        cam._c.origin[i] = float(origin[i])
        cam._c.lower_left_corner[i] = float(origin[i]) + float(L[i])
        cam._c.horizontal[i] = float(hor[i])
        cam._c.vertical[i] = float(ver[i])
    return cam


def zero_cases(spt, oracle):
    """[(label, prims, cam, p, kernel)]: the zero-component views on the HEAD scene, and every fan
    from an origin exactly on a plane (room walls, the light, box faces, edges and corners) of the
    HEAD and the moved-box scenes (ray_truth's F3)."""
    out = []
    on_plane = lambda l: l.startswith("F3_") and l.endswith("_fan")  # noqa: E731
    for name, kernel, keep in (("head", "const_nee_cam", lambda l: l in ZERO_VIEWS or on_plane(l)),
                               ("movebox", "upbox_nee_cam", on_plane)):
        prims = rt.scene(spt, name)
        for label, o, L, hor, ver, w, h in rt.views(spt, oracle, name, "raw"):
            if keep(label):
                p = params(spt, width=w, height=h, spp=ZERO_SPP)
                out.append((f"{name}:{label}", prims, raw_camera(spt, o, L, hor, ver), p, kernel))
    return out


def n_units(p):
    chunk = p.chunk if p.chunk > 0 else p.spp
    return p.width * p.height * ((p.spp + chunk - 1) // chunk)


def oracle_counts(oracle, prims, cam, p, proof):
    """The oracle's render of a case and what its statistics say about the shadow rays: proven (the
    early resolve's claims; 0 without a proof mode), traced and reached, traced and blocked."""
    if proof:
        oracle.proof_check(True, edited=proof == "edited")
    try:
        img, st = oracle.counter_render(prims, cam._c, p)
        claims, wrong = oracle.proof_counts() if proof else (0, 0)
    finally:
        oracle.proof_check(False)
    assert wrong == 0
    cand = st["shadow_traced"]  # the shadow rays the light's test accepts: proven or traced
    return img, st, dict(proven=claims, reached=st["nee_light_hits"] - claims,
                         blocked=cand - st["nee_light_hits"], misses=st["misses"])

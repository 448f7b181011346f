"""A plain float64 nearest hit over a scene, and the edge-ray families of tests/test_contract_rays.py
(the contract's c_intersect against this truth, on the CPU) and tests/test_gpu_rays.py (the same rays
through the render kernels on the GPU).

The truth is geometry, written here from the scene description alone: rectangles with closed bounds
and t > 0, spheres with the nearest root beyond the 2e-3 epsilon, everything in float64 on geometry
rounded to float32 the way the host rounds it (plane constants through oracle.plane_k, bounds as
(mid, half), sphere centres and radii to float32; spheres of radius >= SPT_WIDE_SPHERE_RADIUS stay double).
"""
import numpy as np

RECT_XY, RECT_XZ, RECT_YZ, SPHERE = 0, 1, 2, 3
AXES = {RECT_XY: (2, 0, 1), RECT_XZ: (1, 0, 2), RECT_YZ: (0, 1, 2)}  # plane axis, in-plane axes
WIDE_RADIUS = 100.0  # SPT_WIDE_SPHERE_RADIUS (include/spt.h)
EPS = 2e-3
MISS = -1


def f32(x):
    return float(np.float32(x))


class Truth:
    def __init__(self, oracle, prims):
        self.n = len(prims)
        self.rects, self.spheres = [], []
        for i, p in enumerate(prims):
            g = list(p.geom)
            if p.kind == SPHERE:
                wide = g[0] >= WIDE_RADIUS
                r, c = (g[0], g[1:4]) if wide else (f32(g[0]), [f32(v) for v in g[1:4]])
                self.spheres.append((i, r, np.array(c, dtype=np.float64)))
            else:
                ax, a, b = AXES[p.kind]
                self.rects.append((i, ax, a, b, oracle.plane_k(g[4]),
                                   f32((g[0] + g[1]) * 0.5), f32((g[1] - g[0]) * 0.5),
                                   f32((g[2] + g[3]) * 0.5), f32((g[3] - g[2]) * 0.5)))

    def all_hits(self, o, d):
        """(t, margin): (rays, prims) float64. t = inf where the primitive is not hit; margin = the
        hit point's distance to the nearest edge of the hit rectangle (inf for spheres)."""
        o = np.asarray(o, dtype=np.float32).astype(np.float64).reshape(-1, 3)
        d = np.asarray(d, dtype=np.float32).astype(np.float64).reshape(-1, 3)
        t = np.full((len(o), self.n), np.inf)
        m = np.full((len(o), self.n), np.inf)
        with np.errstate(divide="ignore", invalid="ignore"):
            for i, ax, a, b, k, ma, ha, mb, hb in self.rects:
                tt = (k - o[:, ax]) / d[:, ax]
                ea = ha - np.abs(o[:, a] + d[:, a] * tt - ma)
                eb = hb - np.abs(o[:, b] + d[:, b] * tt - mb)
                ok = (d[:, ax] != 0) & (tt > 0) & (ea >= 0) & (eb >= 0)
                t[:, i] = np.where(ok, tt, np.inf)
                m[:, i] = np.where(ok, np.minimum(ea, eb), np.inf)
            aa = (d * d).sum(axis=1)
            for i, r, c in self.spheres:
                op = c[None, :] - o
                kk = (op * d).sum(axis=1) / aa  # the cancellation-free form: a = d.d kept
                q = op - kk[:, None] * d
                det = r * r - (q * q).sum(axis=1)
                sd = np.sqrt(np.where(det >= 0, det, np.nan) / aa)
                t1, t2 = kk - sd, kk + sd
                t[:, i] = np.where(t1 > EPS, t1, np.where(t2 > EPS, t2, np.inf))
        return t, m

    def nearest(self, o, d):
        """(id, t, gap, margin): the nearest hit's index (MISS = none) and distance, the distance to
        the second nearest hit behind it, and the hit's margin to its rectangle's edge."""
        t, m = self.all_hits(o, d)
        order = np.argsort(t, axis=1, kind="stable")
        rows = np.arange(len(t))
        t0 = t[rows, order[:, 0]]
        t1 = t[rows, order[:, 1]] if self.n > 1 else np.full(len(t), np.inf)
        ids = np.where(np.isfinite(t0), order[:, 0], MISS)
        with np.errstate(invalid="ignore"):
            gap = np.where(np.isfinite(t1), t1 - t0, np.inf)
        return ids, t0, gap, m[rows, order[:, 0]]


def t_bound(T, prims, o, d, ids, t64):
    """The issue's bound on |t32 - t64| for equal ids. Rectangles: 4 (2^-24 max(|k|, |o_a|) / |d_a| +
    2^-22 t): the rounding of k - o_a, then rcp_nr, the fma and the float store. Narrow spheres, the
    analogue for t = b - sqrt(b^2 - op.op + r^2) in fp32 with |d| = 1 assumed: b carries 3 roundings
    of size 2^-24 |op|, the discriminant 2^-23 (b^2 + op.op + r^2) which the root divides by 2 sd, the
    root itself rsq_nr2's 5e-6. Wide spheres are fp64 stored as a float: 2^-22 t."""
    o, d = o.astype(np.float64), d.astype(np.float64)
    b = np.full(len(o), np.nan)
    for i, ax, *_rest in T.rects:
        k = _rest[2]
        s = ids == i
        b[s] = 4 * (2.0 ** -24 * np.maximum(abs(k), np.abs(o[s, ax])) / np.abs(d[s, ax]) + 2.0 ** -22 * t64[s])
    for i, r, c in T.spheres:
        s = ids == i
        if r >= WIDE_RADIUS:
            b[s] = 2.0 ** -22 * t64[s]
            continue
        op = c[None, :] - o[s]
        op2 = (op * op).sum(axis=1)
        bb = (op * d[s]).sum(axis=1)
        sd = np.abs(bb - t64[s])
        b[s] = 4 * (2.0 ** -24 * (3 * np.sqrt(op2) + (bb * bb + op2 + r * r) / np.maximum(sd, 1e-6))
                    + 5e-6 * sd + 2.0 ** -22 * t64[s])
    return b


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.sqrt((v * v).sum(axis=-1, keepdims=True))


def fan(origin, target, n=16, extent=2.0 ** -10, normalise=True):
    """An n x n fan of directions of angular extent `extent` centred on origin -> target. Returns
    (directions (n, n, 3) float32, step): neighbours in the fan are one `step` (radians) apart."""
    origin, target = np.asarray(origin, np.float64), np.asarray(target, np.float64)
    c = unit(target - origin)
    helper = np.array([0.0, 1.0, 0.0]) if abs(c[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    u = unit(np.cross(c, helper))
    v = np.cross(c, u)
    step = extent / n
    k = (np.arange(n) - (n - 1) / 2.0) * step
    d = c[None, None, :] + k[:, None, None] * v[None, None, :] + k[None, :, None] * u[None, None, :]
    if normalise:
        d = unit(d)
    return d.astype(np.float32), step


def fan_neighbours(origin, d, step):
    """The four directions one fan step to either side of each direction in d (rays, 3)."""
    d = np.asarray(d, dtype=np.float64)
    n = np.sqrt((d * d).sum(axis=1, keepdims=True))
    helper = np.where(np.abs(d[:, 1:2]) < 0.9 * n, [[0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0]])
    u = unit(np.cross(d, helper))
    v = np.cross(d / n, u)
    return [d + s * step * n * w for s in (1, -1) for w in (u, v)]


# ---- scenes ----------------------------------------------------------------------------------
def scene(spt, name):
    import test_dispatch as td
    import test_oracle as to

    if name == "classic":
        return spt.smallpt_classic_scene()
    if name == "editroom":
        return to.edited_scene(spt, **to.EDITS_LR[2][0])
    if name == "editlight":
        return to.edited_scene(spt, **to.EDITS_LR[0][0])
    if name.startswith("negzero"):
        return td.neg_zero_walls(spt, **td.NEG_ZERO[int(name[-1])])
    if name == "three_spheres":  # the HEAD room and light with three hand-placed matte spheres
        head = spt.cornell_scene()[:7]
        return head + [spt.Sphere(10.0, (30.0, 10.0, 60.0), 0, (0.7, 0.7, 0.7)),
                       spt.Sphere(6.0, (70.0, 40.0, 90.0), 0, (0.7, 0.3, 0.3)),
                       spt.Sphere(0.5, (50.0, 20.3, 120.7), 0, (0.3, 0.3, 0.7))]
    return td.scene(spt, name)  # head, movebox, dropbox, spheres32


def room_box(prims):
    """(lo, hi) of the closed room the first six rectangles make (x, y, z)."""
    lo = np.array([prims[2].geom[4], prims[4].geom[4], prims[0].geom[4]])
    hi = np.array([prims[3].geom[4], prims[5].geom[4], prims[1].geom[4]])
    return lo, hi


def eye(prims):
    """A general point of the room (in no box, on no plane): where the graze fans start."""
    lo, hi = room_box(prims) if prims[0].kind != SPHERE else (np.array([1, 0, 0.]), np.array([99, 81.6, 170.]))
    return lo + (hi - lo) * np.array([0.47, 0.52, 0.71])


def graze_targets(prims):
    """F4 / F6: [(label, point)] -- corners, edge midpoints, rims: where a hit changes its id."""
    if prims[0].kind == SPHERE:  # the classic sphere box
        cap = 18.0  # the light's cap below the ceiling: where the two spheres meet (the ceiling is
        for _ in range(4):  # itself a sphere: y = 81.6 - r^2 / 2e5 at radius r from (50, ., 81.6))
            cap = np.sqrt(600.0 ** 2 - (681.33 - (81.6 - cap * cap / 2e5)) ** 2)
        return [("cap_rim_x", (50 + cap, 81.6, 81.6)), ("cap_rim_z", (50, 81.6, 81.6 - cap)),
                ("wall_floor", (1, 0, 80)), ("corner", (1.042, 81.555, 0.020)), ("ball_rim", tuple(tangent_point(eye(prims), 16.5, (27, 16.5, 47))))]
    lo, hi = room_box(prims)
    g = prims[6].geom
    out = [("room_corner0", (lo[0], hi[1], lo[2])), ("room_corner1", (hi[0], hi[1], lo[2])),
           ("room_corner2", (lo[0], hi[1], hi[2])), ("room_corner3", (hi[0], lo[1], hi[2])), ("light_corner", (g[0], g[4], g[2])),
           ("light_corner2", (g[1], g[4], g[3]))]
    for top in (11, 16):
        if len(prims) > top and prims[top].kind == RECT_XZ:
            x1, x2, z1, z2, y = prims[top].geom
            out += [(f"box{top}_top_corner", (x1, y, z2)), (f"box{top}_edge_mid", (x2, y / 2, z2)),
                    (f"box{top}_floor_line", ((x1 + x2) / 2, lo[1], z2))]
    return out


def sphere_list(prims):
    return [(i, p.geom[0], np.array(p.geom[1:4])) for i, p in enumerate(prims)
            if p.kind == SPHERE and p.geom[0] < WIDE_RADIUS]


def tangent_point(o, r, c, roll=0.3):
    """A point of the sphere's silhouette as seen from o."""
    o, c = np.asarray(o, np.float64), np.asarray(c, np.float64)
    u = unit(c - o)
    w = unit(np.cross(u, [np.sin(roll), np.cos(roll), 0.2]))
    s = r / np.sqrt(((c - o) ** 2).sum())
    return c + r * (-s * u + np.sqrt(1 - s * s) * w)


def sphere_rays(prims, which=(0, 1, 2)):
    """F5: [(label, origin, direction)] at the narrow spheres `which` (indices into sphere_list):
    from the surface outwards and inwards, from inside, and from 1e-3, 2e-3 and 3e-3 in front of
    the surface along the ray (the near root inside, at and beyond the 2e-3 epsilon)."""
    out = []
    sl = sphere_list(prims)
    for j in which:
        i, r, c = sl[j]
        n = unit(np.array([0.36, 0.48, -0.8]))
        surf = (c + r * n).astype(np.float32).astype(np.float64)
        d_in = unit(-n + np.array([0.3, -0.2, 0.1]))
        out += [(f"s{i}_surface_out", surf, unit(n + np.array([0.2, 0.1, 0.3]))),
                (f"s{i}_surface_in", surf, d_in), (f"s{i}_inside", c + 0.3 * r * n, d_in)]
        for k, delta in enumerate((1e-3, 2e-3, 3e-3)):
            out.append((f"s{i}_front{k + 1}e-3", surf - delta * d_in, d_in))
    return out


def plane_origins(name):
    """F3: [(origin, own prims)] for a scene (tests/test_contract_rays.py PLANE_ORIGINS)."""
    import test_contract_rays as tcr

    return [(o, own) for n, o, own in tcr.PLANE_ORIGINS if n == name]


def views(spt, oracle, name, cls):
    """The camera views of families F2-F6 for one scene: [(label, origin, L, hor, ver, w, h)].
    cls 'raw': any camera vectors (single rays hor = ver = 0, and fans); cls 'axis': hor = (hx, 0, 0),
    ver = (0, vy, 0) and every component of L nonzero (what the axis-camera kernels take)."""
    prims = scene(spt, name)
    e = eye(prims)
    out = []
    ext = 2.0 ** -10
    zero3 = (0.0, 0.0, 0.0)
    spheres = sphere_list(prims)
    if cls == "raw":
        for oi, o in enumerate(ZERO_ORIGINS):  # F2: the seven zero-component single rays
            for di, d in enumerate(ZERO_DIRS):
                out.append((f"F2_o{oi}_d{di}", o, d, zero3, zero3, 4, 4))
        out += [("F2_fan_x", (50, 40, 100), (0, -.5, -.8), (0, 1, 0), (0, 0, .5), 16, 16),
                ("F2_fan_x_light", (50, 30, 80), (0, .9, -.3), (0, .05, 0), (0, 0, .6), 16, 16),
                ("F2_fan_z_light", (50, 30, 80), (-.3, .9, 0), (.6, 0, 0), (0, .05, 0), 16, 16),
                ("F2_fan_y", (30, 40, 20), (-.5, 0, .2), (1, 0, 0), (0, 0, 1), 16, 16),
                ("F2_fan_y_low", (50, 6, 100), (-.5, 0, -1), (1, 0, 0), (0, 0, .2), 16, 16)]
    else:
        # a plain axis fan (the zero-component lattice case is test_gpu_rays' own: it needs 2^19 samples)
        out.append(("F2_axis_near_zero", (50, 40, 100), (-2, -.45, -.8), (4, 0, 0), (0, .3, 0), 4, 16))
    if prims[0].kind != SPHERE:
        for k, (o, own) in enumerate(plane_origins(name)):
            o = tuple(oracle.plane_k(float(v[1:])) if isinstance(v, str) else v for v in o)
            into = np.sign(e - np.array(o, dtype=np.float64))  # towards the room's inside
            into[into == 0] = 1.0
            if cls == "raw":
                out.append((f"F3_{k}_ray", o, tuple(into * (0.3, 0.5, 0.4)), zero3, zero3, 4, 4))
                out.append((f"F3_{k}_fan", o, tuple(into * (0.5, 0.4, 0.6) - (0.5, 0.45, 0.1)),
                            (.8, .1, -.3), (.1, .7, .3), 8, 8))
            else:
                out.append((f"F3_{k}_axis", o, tuple(into * (0.2, 0.3, 0.6) - (0.4, 0.25, 0.05)),
                            (.8, 0, 0), (0, .6, 0), 8, 8))
    targets = graze_targets(prims)
    for j, (i, r, c) in enumerate(spheres[:3] if name == "three_spheres" else spheres[1::10]):
        targets.append((f"s{i}_tangent", tuple(tangent_point(e, r, c))))
    for label, tgt in targets:  # F4, F6 and F5's tangents: 16 x 16 fans of extent 2^-10
        c = unit(np.array(tgt, dtype=np.float64) - e)
        if cls == "raw":
            u = unit(np.cross(c, [0.0, 1.0, 0.0] if abs(c[1]) < 0.9 else [1.0, 0.0, 0.0]))
            v = np.cross(c, u)
            hor, ver = ext * u, ext * v
        else:
            hor, ver = np.array([ext, 0, 0]), np.array([0, ext, 0])
        out.append((f"F4_{label}", tuple(e), tuple(c - hor / 2 - ver / 2), tuple(hor), tuple(ver), 16, 16))
    if cls == "raw" and spheres:  # F5: single rays at the epsilon
        which = sorted({0, len(spheres) // 2, len(spheres) - 1})
        for label, o, d in sphere_rays(prims, which):
            out.append((f"F5_{label}", tuple(o), tuple(d), zero3, zero3, 4, 4))
    if prims[0].kind == SPHERE and cls == "raw":  # F6: from inside a ball, from a point on a wall
        out += [("F6_in_ball", (27 + 4, 16.5 + 3, 47 - 2), (.3, .5, -.4), (.1, 0, .1), (0, .1, .05), 8, 8),
                ("F6_on_wall", (1, 40, 80), (.5, -.2, .3), (.2, 0, .1), (0, .3, 0), 8, 8)]
    return out


# the seven directions of the issue: one component an exact (signed) zero
ZERO_DIRS = [(0, 1, 0), (0, -1, 0), (0, .6, .8), (0, .6, -.8), (-0.0, .6, .8), (.6, 0, .8), (.6, .8, 0)]
# mid-room, under the light, beside the short box
ZERO_ORIGINS = [(50, 40, 100), (50, 30, 80), (60, 12, 75)]


# ---- first-hit id images ------------------------------------------------------------------------
def id_scene(spt, prims):
    """Every prim black (c = 0) and emitting its index: e_i = ((i + 1) / 64, ((7 i) mod 64 + 1) / 64, 1).
    A path ends at its first hit, so a 1 spp image is the first-hit id per pixel (a miss is black)."""
    out = [spt.spt_prim.from_buffer_copy(p) for p in prims]
    for i, p in enumerate(out):
        p.c[0] = p.c[1] = p.c[2] = 0.0
        p.e[0], p.e[1], p.e[2] = (i + 1) / 64.0, ((7 * i) % 64 + 1) / 64.0, 1.0
    return out


def decode_ids(img):
    """The prim index per pixel of an id image (MISS where black); checks the second channel."""
    r = np.rint(img[..., 0].astype(np.float64) * 64).astype(np.int64) - 1
    ids = np.where(img[..., 2] > 0.5, r, MISS)
    g = np.where(ids >= 0, ((7 * ids) % 64 + 1) / 64.0, 0.0)
    assert np.array_equal(img[..., 1].astype(np.float64), g), "not an id image"
    return ids


TILTED = dict(lookfrom=(40, 55, 160), lookat=(55, 35, 10), vup=(0.1, 1, 0))
# (label, scene, camera kwargs, params, level, variant): the views of the id images, chosen on the CPU
# so that at most 15 % (HEAD) / 20 % of the pixels straddle a boundary
ID_VIEWS = [
    ("head_ref_nee", "head", {}, dict(nee_prob=1.0), "auto", "const_nee_ref"),
    ("head_ref_cos", "head", {}, dict(nee_prob=0.0), "auto", "const_cos_ref"),
    ("head_tilted", "head", TILTED, dict(nee_prob=1.0), "auto", "const"),
    ("movebox", "movebox", {}, dict(nee_prob=1.0), "auto", "cornell"),
    ("spheres32", "spheres32", {}, dict(nee_prob=1.0, max_depth=12), "auto", "sphdiff_nee_ref"),
    ("head_generic", "head", TILTED, dict(nee_prob=0.0), "generic", "generic"),
]
ID_W, ID_H = 64, 48


def id_view(spt, label, seed):
    _, name, camkw, kw, level, want = next(v for v in ID_VIEWS if v[0] == label)
    prims = id_scene(spt, scene(spt, name))
    cam = spt.Camera(aspect=float(np.float32(ID_W) / np.float32(ID_H)), **camkw)
    p = spt.default_params(width=ID_W, height=ID_H, spp=1, seed=seed, flags=spt.kernel_flag(level), **kw)
    return prims, cam, p, want


def footprint_ids(T, cam, w, h):
    """Per pixel the fp64 id shared by nine rays over its jitter range (corners, edge midpoints,
    centre), or -2 where they differ: (h, w) int."""
    c = cam._c
    f = lambda v: np.array([f32(x) for x in v], dtype=np.float64)  # noqa: E731 -- the kernel's floats
    o, llc, hor, ver = f(c.origin), f(c.lower_left_corner), f(c.horizontal), f(c.vertical)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    out = None
    for ju in (0.0, 0.5, 65535.0 / 65536.0):
        for jv in (0.0, 0.5, 65535.0 / 65536.0):
            su = (xs - 0.5 + ju) / w
            sv = (h - ys - 1 - 0.5 + jv) / h
            d = llc[None, None] + hor[None, None] * su[..., None] + ver[None, None] * sv[..., None] - o
            ids = T.nearest(np.tile(o, (w * h, 1)), unit(d).reshape(-1, 3))[0].reshape(h, w)
            out = ids if out is None else np.where(out == ids, out, -2)
    return out

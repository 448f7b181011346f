"""Temporal accumulation (include/spt.h, SPT_HAS_TEMPORAL) restated in numpy float32, operation for
operation in the header's order, and a synthetic sequence maker for the tests: an fp64 ray-caster for
the pixel-mean rays of two axis-parallel rectangles.

A camera here is a (4, 3) float64 array: origin, lower_left_corner, horizontal, vertical. A state is a
dict of the planes c, v, X, N (h, w, 3) and n (h, w), float32.
"""
import numpy as np

F = np.float32
STATE_PLANES = ("c", "v", "n", "X", "N")


def to_struct(spt, cam):
    """The spt_camera of a (4, 3) camera."""
    c = spt.spt_camera()
    for k in range(3):
        c.origin[k], c.lower_left_corner[k] = cam[0][k], cam[1][k]
        c.horizontal[k], c.vertical[k] = cam[2][k], cam[3][k]
    return c


def _cross(u, v):
    return np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]])


def camera_consts(cam, w, h):
    """The header's host constants: doubles, each value rounded once. None for a singular camera."""
    o, llc, hor, ver = np.asarray(cam, np.float64)
    a, b, c = hor / np.float64(w), ver / np.float64(h), llc - o
    bc, ca, ab = _cross(b, c), _cross(c, a), _cross(a, b)
    det = (a[0] * bc[0] + a[1] * bc[1]) + a[2] * bc[2]
    if not np.isfinite(det) or not abs(det) > 0.0:
        return None
    with np.errstate(all="ignore"):
        K = {"o": o.astype(F), "E": c.astype(F), "Hx": a.astype(F), "Vy": b.astype(F),
             "M": np.concatenate([bc / det, ca / det, ab / det]).astype(F)}
    return K if all(np.all(np.isfinite(v)) for v in K.values()) else None


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def accumulate_truth(rgb, se, albedo, normal, depth, cam, prev=None, prev_cam=None, n_max=32.0, normal_min=0.9,
                     plane_tol=0.01, albedo_floor=0.01, flags=0):
    """-> {"rgb", "se", "n", "hist", "state"}: steps 1-7 of the header at every pixel."""
    rgb, se, albedo, normal = (np.asarray(a, F) for a in (rgb, se, albedo, normal))
    z = np.asarray(depth, F)
    h, w = z.shape
    K = camera_consts(cam, w, h)
    assert K is not None and (prev is None) == (prev_cam is None)
    n_max, normal_min, plane_tol, albedo_floor = F(n_max), F(normal_min), F(plane_tol), F(albedo_floor)
    one, zero = F(1.0), F(0.0)
    with np.errstate(all="ignore"):
        # 1
        a = np.ones_like(albedo) if flags & 1 else np.fmax(albedo, albedo_floor)
        c = rgb / a
        e = se / a
        var = e * e
        # 2
        px = np.arange(w, dtype=np.int64).astype(F)[None, :]
        py = (h - 1 - np.arange(h, dtype=np.int64)).astype(F)[:, None]
        D = np.stack([(K["E"][k] + K["Hx"][k] * px) + K["Vy"][k] * py for k in range(3)], axis=-1)
        length = np.sqrt((D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1]) + D[..., 2] * D[..., 2])
        X = np.stack([K["o"][k] + (D[..., k] / length) * z for k in range(3)], axis=-1)
        miss = z == zero
        ok = np.zeros((h, w), bool) if prev is None else ~miss
        gy, gx = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
        W = np.zeros((h, w), F)
        Ch, Vh, Nh = np.zeros((h, w, 3), F), np.zeros((h, w, 3), F), np.zeros((h, w), F)
        if prev is not None:
            same = np.array_equal(np.asarray(cam, np.float64), np.asarray(prev_cam, np.float64))
            if same:  # 5
                x0, y0, taps = gx, gy, [(0, 0)]
            else:  # 3
                Kp = camera_consts(prev_cam, w, h)
                assert Kp is not None
                q = [X[..., k] - Kp["o"][k] for k in range(3)]
                M = Kp["M"]
                A, B, C = [(M[3 * r] * q[0] + M[3 * r + 1] * q[1]) + M[3 * r + 2] * q[2] for r in range(3)]
                ok = ok & (C > zero)
                fx = A / C
                fy = F(h - 1) - B / C
                ok = ok & (fx >= F(-1.0)) & (fx < F(w)) & (fy >= F(-1.0)) & (fy < F(h))
                flx, fly = np.floor(fx), np.floor(fy)
                x0 = np.where(ok, flx, zero).astype(np.int64)
                y0 = np.where(ok, fly, zero).astype(np.int64)
                tx, ty = fx - flx, fy - fly
                taps = [(0, 0), (1, 0), (0, 1), (1, 1)]  # (i, j): j then i
            # 4
            for i, j in taps:
                xx, yy = x0 + i, y0 + j
                inside = ok & (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
                xc, yc = np.clip(xx, 0, w - 1), np.clip(yy, 0, h - 1)
                b = np.ones((h, w), F) if same else (tx if i else one - tx) * (ty if j else one - ty)
                nq, Nq, Xq = prev["n"][yc, xc], prev["N"][yc, xc], prev["X"][yc, xc]
                valid = inside & (nq > zero) & (_dot3(normal, Nq) >= normal_min)
                valid = valid & (np.abs(_dot3(normal, Xq - X)) <= plane_tol * z)
                W = np.where(valid, W + b, W)
                Ch = np.where(valid[..., None], Ch + b[..., None] * prev["c"][yc, xc], Ch)
                Vh = np.where(valid[..., None], Vh + b[..., None] * prev["v"][yc, xc], Vh)
                Nh = np.where(valid, Nh + b * nq, Nh)
            ok = ok & (W >= F(0.25))
        # 6
        n1 = np.fmin(Nh / W + one, n_max)
        alpha = one / n1
        beta = one - alpha
        ch, vh = Ch / W[..., None], Vh / W[..., None]
        okc = ok[..., None]
        c1 = np.where(okc, beta[..., None] * ch + alpha[..., None] * c, c)
        v1 = np.where(okc, (beta * beta)[..., None] * vh + (alpha * alpha)[..., None] * var, var)
        n = np.where(ok, n1, np.where(miss, zero, one)).astype(F)
        # 7
        out = {"rgb": np.fmin(c1 * a, one), "se": np.sqrt(v1) * a, "n": n, "hist": np.where(okc, ch * a, rgb)}
    out["state"] = {"c": c1.astype(F), "v": v1.astype(F), "n": n, "X": X.astype(F), "N": normal.copy()}
    for k in ("rgb", "se", "hist"):
        out[k] = out[k].astype(F)
    return out


# ---- the synthetic sequences ----------------------------------------------------------------------
# Rectangles in planes z = const, facing +z: (x0, x1, y0, y1, z, albedo).
WALL_AND_SQUARE = [(-30.0, 30.0, -30.0, 30.0, -100.0, (0.7, 0.6, 0.5)),
                   (-8.0, 8.0, -6.0, 6.0, -50.0, (0.2, 0.5, 0.8))]


def camera(w, h, origin=(0.0, 0.0, 0.0), half_width=None):
    """A camera at `origin` that looks down -z, its image plane at distance 1, 2 * half_width wide (default
    0.4 * w / max(w, h)) with square pixels."""
    a = 0.4 * w / max(w, h) if half_width is None else half_width
    b = a * h / w
    o = np.array(origin, np.float64)
    return np.array([o, o + np.array([-a, -b, -1.0]), [2.0 * a, 0.0, 0.0], [0.0, 2.0 * b, 0.0]], np.float64)


def cast(cam, w, h, rects=WALL_AND_SQUARE):
    """The pixel-mean rays against the rectangles in fp64 -> (t (h, w), the ray parameter of the unit
    direction, 0 at a miss; id (h, w), -1 at a miss; X (h, w, 3))."""
    o, llc, hor, ver = np.asarray(cam, np.float64)
    px = np.arange(w, dtype=np.float64)[None, :, None]
    py = (h - 1 - np.arange(h, dtype=np.float64))[:, None, None]
    d = (llc - o) + (hor / w) * px + (ver / h) * py
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    return cast_rays(o, d, rects)


def cast_rays(o, d, rects=WALL_AND_SQUARE):
    """Rays o + t d (d of unit length, any leading shape) -> (t, id, X) of the nearest hit."""
    t = np.full(d.shape[:-1], np.inf)
    pid = np.full(d.shape[:-1], -1, np.int64)
    with np.errstate(all="ignore"):
        for k, (x0, x1, y0, y1, zk, _) in enumerate(rects):
            tk = (zk - o[..., 2]) / d[..., 2]
            x, y = o[..., 0] + tk * d[..., 0], o[..., 1] + tk * d[..., 1]
            hit = (tk > 0) & (tk < t) & (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1)
            t = np.where(hit, tk, t)
            pid = np.where(hit, k, pid)
    t = np.where(pid >= 0, t, 0.0)
    return t, pid, o + t[..., None] * d


def shade(X):
    """A smooth function of the world position, within 0.3 .. 0.9."""
    return 0.6 + 0.3 * np.sin(X[..., 0] / 7.0) * np.cos(X[..., 1] / 9.0)


def frame(cam, w, h, seed, se=0.04, rects=WALL_AND_SQUARE, short_normals=True):
    """One frame's five planes (float32) and "id": rgb = albedo * shade(X) plus seeded gaussian noise of
    the standard deviation se (a constant plane). A miss has albedo, normal and depth 0. short_normals: a
    pixel whose right-hand neighbour sees another primitive gets half a normal, as a partly covered
    pixel of a real guide has."""
    t, pid, X = cast(cam, w, h, rects)
    albedo = np.zeros((h, w, 3))
    for k, r in enumerate(rects):
        albedo[pid == k] = r[5]
    normal = np.zeros((h, w, 3))
    normal[pid >= 0] = (0.0, 0.0, 1.0)
    if short_normals and w > 1:
        edge = np.zeros((h, w), bool)
        edge[:, :-1] = pid[:, :-1] != pid[:, 1:]
        normal[edge] *= 0.5
    rng = np.random.default_rng(seed)
    rgb = albedo * shade(X)[..., None] + se * rng.standard_normal((h, w, 3))
    return {"rgb": rgb.astype(F), "se": np.full((h, w, 3), se, F), "albedo": albedo.astype(F),
            "normal": normal.astype(F), "depth": t.astype(F), "id": pid}


def planes_of(f):
    return f["rgb"], f["se"], f["albedo"], f["normal"], f["depth"]


# ---- a real scene's first hits --------------------------------------------------------------------
def camera_of(cam_struct):
    """The (4, 3) camera of an spt_camera."""
    return np.array([list(cam_struct.origin), list(cam_struct.lower_left_corner), list(cam_struct.horizontal),
                     list(cam_struct.vertical)], np.float64)


def first_hit_refl(prims, cam, w, h):
    """The refl (0 DIFF, 1 SPEC, 2 REFR; -1 at a miss) of the primitive every pixel-mean ray hits first,
    in fp64: rectangles in the planes z, y, x = const (kinds 0, 1, 2) and spheres (kind 3)."""
    o, llc, hor, ver = np.asarray(cam, np.float64)
    px = np.arange(w, dtype=np.float64)[None, :, None]
    py = (h - 1 - np.arange(h, dtype=np.float64))[:, None, None]
    d = (llc - o) + (hor / w) * px + (ver / h) * py
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    best = np.full((h, w), np.inf)
    refl = np.full((h, w), -1, np.int64)
    axes = {0: (0, 1, 2), 1: (0, 2, 1), 2: (1, 2, 0)}  # kind -> the two bounded axes and the plane's
    with np.errstate(all="ignore"):
        for p in prims:
            g = list(p.geom)
            if p.kind == 3:
                oc = o - np.array(g[1:4])
                b = d @ oc
                disc = b * b - (oc @ oc - g[0] * g[0])
                sq = np.sqrt(np.where(disc > 0, disc, np.nan))
                t = np.where(-b - sq > 1e-9, -b - sq, -b + sq)
                hit = (disc > 0) & (t > 1e-9)
            else:
                u, v, k = axes[p.kind]
                t = (g[4] - o[k]) / d[..., k]
                pu, pv = o[u] + t * d[..., u], o[v] + t * d[..., v]
                hit = (t > 1e-9) & (pu >= g[0]) & (pu <= g[1]) & (pv >= g[2]) & (pv <= g[3])
            hit = hit & (t < best)
            best = np.where(hit, t, best)
            refl = np.where(hit, p.refl, refl)
    return refl

"""The guide contract of include/spt.h (SPT_HAS_GUIDE) restated from the oracle's exported pieces and
nothing else (a helper, not a test): Philox and the jitter through oracle.map_words, the camera's fma
chain with libm's fmaf through ctypes (no float64 emulation: it double-rounds), the normaliser through
the oracle's "normalize" / "normalize_free", (t, id) from oracle.intersect_batch, fix from
oracle.fix_batch, the sphere's hit point and normal as numpy float32 multiply-then-add.
"""
import ctypes
import ctypes.util

import numpy as np

SPHERE, REFR = 3, 2
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fmaf.argtypes = [ctypes.c_float] * 3
_libm.fmaf.restype = ctypes.c_float
F = np.float32


def fmaf(a, b, c):
    """libm's fmaf over float32 arrays (broadcast), one call per element."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F), np.asarray(c, F))
    out = np.empty(a.shape, F)
    fa, fb, fc, fo = a.ravel(), b.ravel(), c.ravel(), out.reshape(-1)
    f = _libm.fmaf
    for i in range(fo.size):
        fo[i] = f(fa[i], fb[i], fc[i])
    return out


def unit_dirs(prims) -> bool:
    """The scene's direction contract: unit directions iff a sphere or a REFR primitive."""
    return any(p.kind == SPHERE or p.refl == REFR for p in prims)


def camera_rays(oracle, cam_c, params, rows, base, count, unit):
    """(o (3,), d (nrows, w, count, 3)) float32: the render's first ray of every (pixel, sample)."""
    w, h = params.width, params.height
    cam = np.array(list(cam_c.origin) + list(cam_c.lower_left_corner) + list(cam_c.horizontal) +
                   list(cam_c.vertical), dtype=np.float64).astype(F)
    rows = np.asarray(rows, dtype=np.int64)
    py, px = np.meshgrid(rows, np.arange(w), indexing="ij")
    words = np.empty((len(rows), w, count, 4), dtype=np.uint32)
    words[..., 0] = (py * w + px)[:, :, None]
    words[..., 1] = np.arange(base, base + count, dtype=np.uint32)[None, None, :]
    words[..., 2] = 1
    words[..., 3] = params.seed
    r = oracle.map_words("philox", words.reshape(-1, 4))
    Fu = oracle.map_words("jitter", r[:, 0:2]).view(F).reshape(len(rows), w, count)
    Fv = oracle.map_words("jitter", r[:, 2:4]).view(F).reshape(len(rows), w, count)
    inv_w, inv_h = F(1.0) / F(w), F(1.0) / F(h)
    fx = ((px.astype(F) - F(0.5)) - F(128.0))
    fy = (((h - py - 1).astype(F) - F(0.5)) - F(128.0))
    v = np.empty((len(rows), w, count, 3), dtype=F)
    for c in range(3):
        Au, Av = cam[6 + c] * inv_w, cam[9 + c] * inv_h
        Pc = fmaf(Au, fx, fmaf(Av, fy, cam[3 + c] - cam[c]))
        v[..., c] = fmaf(Fv, Av * F(2.0 ** -16), fmaf(Fu, Au * F(2.0 ** -16), Pc[:, :, None]))
    op = "normalize" if unit else "normalize_free"
    d = oracle.map_words(op, v.reshape(-1, 3).view(np.uint32)).view(F).reshape(v.shape)
    return cam[0:3].copy(), d


def ray_records(oracle, prims, params, o, d):
    """One record int64[8] per ray (zeros on a miss): o (n, 3) or (3,), d (n, 3) float32."""
    d = np.ascontiguousarray(d, dtype=F).reshape(-1, 3)
    o = np.ascontiguousarray(np.broadcast_to(np.asarray(o, F), d.shape))
    t, ids = oracle.intersect_batch(prims, params, o, d)
    n = len(d)
    rec = np.zeros((n, 8), dtype=np.int64)
    hit = ids >= 0
    safe = np.where(hit, ids, 0)
    kind = np.array([p.kind for p in prims])[safe]
    col = np.array([[p.c[0], p.c[1], p.c[2]] for p in prims], dtype=np.float64).astype(F)[safe]
    inv_spp = F(1.0) / F(params.spp)
    nl = np.zeros((n, 3), dtype=F)
    for k, axis in ((0, 2), (1, 1), (2, 0)):  # RECT_XY -> z, RECT_XZ -> y, RECT_YZ -> x
        m = kind == k
        nl[m, axis] = np.where(d[m, axis] < 0, F(1.0), F(-1.0))
    m = kind == SPHERE
    if m.any():
        cen = np.array([[p.geom[1], p.geom[2], p.geom[3]] for p in prims], dtype=np.float64).astype(F)[safe]
        rad = np.array([p.geom[0] for p in prims], dtype=np.float64).astype(F)[safe]
        rad = np.where(m, rad, F(1.0))
        inv_r = (F(1.0) / rad).astype(F)
        x = (o + (d * t[:, None]).astype(F)).astype(F)  # a multiply, then an add
        gn = ((x - cen).astype(F) * inv_r[:, None]).astype(F)
        dot = fmaf(gn[m, 2], d[m, 2], fmaf(gn[m, 1], d[m, 1], gn[m, 0] * d[m, 0]))
        nl[m] = np.where((dot < 0)[:, None], gn[m], -gn[m])
    for k in range(3):
        rec[:, k] = oracle.fix_batch(col[:, k], inv_spp).astype(np.int64)
        mag = oracle.fix_batch(np.abs(nl[:, k]), inv_spp).astype(np.int64)
        rec[:, 3 + k] = np.where(nl[:, k] < 0, -mag, mag)
    depth = (np.minimum(t, F(2.0 ** 20)) * F(65536.0)).astype(F)
    rec[:, 6] = depth.astype(np.float64).astype(np.int64)  # exact: < 2^36, truncation
    rec[:, 7] = 1
    rec[~hit] = 0
    return rec


def guide_truth(oracle, prims, cam_c, params, base=0, count=None, rows=None):
    """The records (nrows, w, 8) int64 of the window [base, base + count) (default: all of
    [0, spp)) over `rows` (default: every image row)."""
    count = params.spp - base if count is None else count
    rows = np.arange(params.height) if rows is None else np.asarray(rows)
    o, d = camera_rays(oracle, cam_c, params, rows, base, count, unit_dirs(prims))
    rec = ray_records(oracle, prims, params, o, d.reshape(-1, 3))
    return rec.reshape(len(rows), params.width, count, 8).sum(axis=2)


def resolve_numpy(records, spp_total, samples_done):
    """The resolve of include/spt.h as a numpy statement -> dict of the four float32 planes."""
    rec = np.asarray(records, dtype=np.int64)
    shape = rec.shape[:-1]
    n = int(samples_done)
    if n == 0:
        return {"albedo": np.zeros(shape + (3,), F), "normal": np.zeros(shape + (3,), F),
                "depth": np.zeros(shape, F), "coverage": np.zeros(shape, F)}
    full = n == spp_total
    r = F(np.float64(spp_total) / np.float64(n))

    def scaled(mag):  # (float)mag * 2^-31 [* r]
        f = mag.astype(np.uint64).astype(F) * F(2.0 ** -31)
        return f if full else (f * r).astype(F)

    alb = scaled(rec[..., 0:3])
    alb = np.where(alb > F(1.0), F(1.0), alb).astype(F)
    s = rec[..., 3:6]
    f = scaled(np.abs(s))
    nor = np.where(s < 0, -f, f).astype(F)
    hits = rec[..., 7]
    with np.errstate(divide="ignore", invalid="ignore"):
        dep = (rec[..., 6].astype(np.float64) / (hits.astype(np.float64) * 65536.0)).astype(F)
    dep = np.where(hits != 0, dep, F(0.0)).astype(F)
    cov = (hits.astype(np.float64) / np.float64(n)).astype(F)
    return {"albedo": alb, "normal": nor, "depth": dep, "coverage": cov}


def albedo_scene(spt, prims):
    """Every primitive emits its colour: with max_depth = 1 and nee_prob = 0 a render is the first
    hit's albedo (a miss reads primitive 0)."""
    out = [spt.spt_prim.from_buffer_copy(p) for p in prims]
    for p in out:
        for k in range(3):
            p.e[k] = p.c[k]
    return out

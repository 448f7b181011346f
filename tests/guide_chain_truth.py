"""The chain rule of include/spt.h (SPT_HAS_GUIDE_CHAIN) restated from what tests/guide_truth.py uses
and nothing else (a helper, not a test): the camera rays of guide_truth.camera_rays, (t, id) from
oracle.intersect_batch with per-ray origins, the contract's reciprocal and normalisers through
oracle.map_f32 / map_words ("rcp_nr", "normalize"), fix from oracle.fix_batch, libm's fmaf through
ctypes, and numpy float32 with one rounding per operation (sqrt included: IEEE).
"""
import numpy as np

import guide_truth as gt

F = np.float32
DIFF, SPEC, REFR = 0, 1, 2
SPHERE = gt.SPHERE
MAX_CHAIN = 8  # SPT_GUIDE_MAX_CHAIN
AXIS = ((0, 2), (1, 1), (2, 0))  # RECT_XY -> z, RECT_XZ -> y, RECT_YZ -> x


def dot3(a, b):
    """fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)) over rows."""
    return gt.fmaf(a[:, 2], b[:, 2], gt.fmaf(a[:, 1], b[:, 1], (a[:, 0] * b[:, 0]).astype(F)))


def _normalize(oracle, v):
    v = np.ascontiguousarray(v, dtype=F)
    return oracle.map_words("normalize", v.view(np.uint32)).view(F).reshape(v.shape)


def _tables(oracle, prims):
    kind = np.array([p.kind for p in prims])
    refl = np.array([p.refl for p in prims])
    col = np.array([[p.c[0], p.c[1], p.c[2]] for p in prims], dtype=np.float64).astype(F)
    plane = np.array([oracle.plane_k(p.geom[4]) if p.kind != SPHERE else 0.0 for p in prims], dtype=F)
    cen = np.array([[p.geom[1], p.geom[2], p.geom[3]] for p in prims], dtype=np.float64).astype(F)
    rad = np.array([p.geom[0] if p.kind == SPHERE else 1.0 for p in prims], dtype=np.float64).astype(F)
    return kind, refl, col, plane, cen, (F(1.0) / rad).astype(F)


def chain_records(oracle, prims, params, o, d, unit):
    """-> (records int64 (n, 8), segments int (n,)): one record per ray (zeros where the chain ends in
    a miss) and the number of segments traced. o (3,) or (n, 3), d (n, 3) float32."""
    d = np.array(d, dtype=F).reshape(-1, 3)
    o = np.array(np.broadcast_to(np.asarray(o, F), d.shape))
    n = len(d)
    KIND, REFL, COL, PLANE, CEN, INV_R = _tables(oracle, prims)
    inv_spp = F(1.0) / F(params.spp)
    A, D = np.ones((n, 3), dtype=F), np.zeros(n, dtype=F)
    rec, segs = np.zeros((n, 8), dtype=np.int64), np.zeros(n, dtype=np.int64)
    active = np.ones(n, dtype=bool)
    for seg in range(MAX_CHAIN):
        idx = np.flatnonzero(active)
        if idx.size == 0:
            break
        t, ids = oracle.intersect_batch(prims, params, o[idx], d[idx])
        segs[idx] = seg + 1
        hit = ids >= 0
        active[idx[~hit]] = False  # a miss on any segment adds nothing
        idx, t, ids = idx[hit], t[hit], ids[hit]
        if idx.size == 0:
            break
        oo, dd = o[idx], d[idx]
        kind, refl, col = KIND[ids], REFL[ids], COL[ids]
        # the hit point and the normals as the render forms them
        tr = t.copy()
        gn, nl = np.zeros((len(idx), 3), dtype=F), np.zeros((len(idx), 3), dtype=F)
        for k, axis in AXIS:
            m = kind == k
            if m.any():
                num = (PLANE[ids[m]] - oo[m, axis]).astype(F)
                da = dd[m, axis]
                tr[m] = gt.fmaf(gt.fmaf(-t[m], da, num), oracle.map_f32("rcp_nr", da), t[m])
                gn[m, axis] = F(1.0)
                nl[m, axis] = np.where(da < 0, F(1.0), F(-1.0))
        x = (oo + (dd * tr[:, None]).astype(F)).astype(F)  # a multiply, then an add
        m = kind == SPHERE
        if m.any():
            g = ((x[m] - CEN[ids[m]]).astype(F) * INV_R[ids[m]][:, None]).astype(F)
            gn[m] = g
            nl[m] = np.where((dot3(g, dd[m]) < 0)[:, None], g, -g)
        end = (refl == DIFF) | (seg == MAX_CHAIN - 1)
        e = idx[end]
        if e.size:
            a = (A[e] * col[end]).astype(F)
            for k in range(3):
                rec[e, k] = oracle.fix_batch(a[:, k], inv_spp).astype(np.int64)
                mag = oracle.fix_batch(np.abs(nl[end, k]), inv_spp).astype(np.int64)
                rec[e, 3 + k] = np.where(nl[end, k] < 0, -mag, mag)
            depth = (np.minimum((D[e] + t[end]).astype(F), F(2.0 ** 20)) * F(65536.0)).astype(F)
            rec[e, 6] = depth.astype(np.float64).astype(np.int64)
            rec[e, 7] = 1
            active[e] = False
        c = ~end
        ci = idx[c]
        if ci.size == 0:
            continue
        A[ci] = (A[ci] * col[c]).astype(F)
        D[ci] = (D[ci] + t[c]).astype(F)
        dc, g, nlc = dd[c], gn[c], nl[c]
        k2 = (F(2.0) * dot3(g, dc)).astype(F)
        nd = (dc - (g * k2[:, None]).astype(F)).astype(F)  # reflRay
        if unit:
            nd = _normalize(oracle, nd)
        r = refl[c] == REFR
        if r.any():
            gr, dr, nr = g[r], dc[r], nlc[r]
            into = dot3(gr, nr) > 0
            nnt = np.where(into, F(1.0) / F(1.5), F(1.5) / F(1.0)).astype(F)
            ddn = dot3(dr, nr)
            cos2t = (F(1.0) - ((nnt * nnt).astype(F) * (F(1.0) - (ddn * ddn).astype(F)).astype(F)).astype(F)).astype(F)
            ok = ~(cos2t < 0)  # else total internal reflection: the reflection
            with np.errstate(invalid="ignore"):
                root = np.sqrt(np.where(ok, cos2t, F(0.0))).astype(F)
            kk = (np.where(into, F(1.0), F(-1.0)) * ((ddn * nnt).astype(F) + root).astype(F)).astype(F)
            tdir = _normalize(oracle, ((dr * nnt[:, None]).astype(F) - (gr * kk[:, None]).astype(F)).astype(F))
            sub = nd[r]
            sub[ok] = tdir[ok]
            nd[r] = sub
        o[ci] = x[c]
        d[ci] = nd
    assert A.dtype == F and D.dtype == F and o.dtype == F and d.dtype == F
    return rec, segs


def chain_truth(oracle, prims, cam_c, params, base=0, count=None, rows=None, return_segments=False):
    """The chain guide's records (nrows, w, 8) int64 of the window [base, base + count) (default: all
    of [0, spp)) over `rows` (default: every image row); return_segments: also the longest chain per
    pixel (nrows, w)."""
    count = params.spp - base if count is None else count
    rows = np.arange(params.height) if rows is None else np.asarray(rows)
    unit = gt.unit_dirs(prims)
    o, d = gt.camera_rays(oracle, cam_c, params, rows, base, count, unit)
    rec, segs = chain_records(oracle, prims, params, o, d.reshape(-1, 3), unit)
    out = rec.reshape(len(rows), params.width, count, 8).sum(axis=2)
    if return_segments:
        return out, segs.reshape(len(rows), params.width, count).max(axis=2)
    return out


def albedo_render_scene(spt, prims):
    """The scene whose film is the chain guide's albedo: every DIFF primitive emits its colour and
    reflects nothing, the specular ones keep theirs and emit nothing (with nee_prob = 0 and rr_depth
    beyond any depth a path's radiance is A * c of its first diffuse vertex)."""
    out = [spt.spt_prim.from_buffer_copy(p) for p in prims]
    for p in out:
        for k in range(3):
            if p.refl == DIFF:
                p.e[k], p.c[k] = p.c[k], 0.0
            else:
                p.e[k] = 0.0
    return out


def _with(spt, prims, edits):
    """A copy of the scene with primitive i made specular: edits = {i: refl}, colour .999."""
    out = [spt.spt_prim.from_buffer_copy(p) for p in prims]
    for i, refl in edits.items():
        out[i].refl = refl
        for k in range(3):
            out[i].c[k], out[i].e[k] = 0.999, 0.0
    return out


# The hall's camera looks across the room at the left mirror, nearly head-on: the rays at the centre
# of the view go back and forth between the two mirrors until the cap, those at its edges reach the
# floor, the ceiling or the far walls after a few segments.
HALL_CAM = dict(lookfrom=(50, 40, 120), lookat=(1, 42, 116))


def scene(spt, name):
    """The chain tests' scenes. HEAD's walls: 0 the one the camera faces (z = 0, at the back of the
    view), 1 the one behind the camera, 2 / 3 left / right."""
    if name == "mirror_glass":
        return spt.smallpt_mirror_glass_scene()
    if name == "classic":
        return spt.smallpt_classic_scene()
    if name == "specular":
        return spt.cornell_specular_scene()
    if name == "head":
        return spt.cornell_scene()
    if name == "spheres32":
        return spt.spheres32_scene()
    if name == "hall":  # a hall of mirrors: chains run into the cap; rect-only, free-scale directions
        return _with(spt, spt.cornell_scene(), {2: SPEC, 3: SPEC})
    if name == "one_mirror_wall":  # one specular primitive, rect-only (free-scale): the wall in view
        return _with(spt, spt.cornell_scene(), {0: SPEC})
    if name == "one_mirror_ball":  # one specular primitive, unit directions: a ball on the short box
        return spt.cornell_scene() + [spt.Sphere(12.0, (75.5, 37.0, 75.5), 0, (0.999, 0.999, 0.999), SPEC)]
    raise KeyError(name)

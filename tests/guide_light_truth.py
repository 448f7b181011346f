"""The light guide's contract of include/spt.h (SPT_HAS_GUIDE_LIGHT) restated from what the two guide
truths use and nothing else (a helper, not a test): the camera rays of guide_truth.camera_rays, (t, id)
from oracle.intersect_batch with per-ray origins, Philox / u01 / the normaliser through oracle.map_words,
the contract's reciprocal through oracle.map_f32("rcp_nr"), fix from oracle.fix_batch, libm's fmaf
through ctypes, and numpy float32 with one rounding per operation (sqrt included: IEEE).
"""
import numpy as np

import guide_chain_truth as gct
import guide_truth as gt

F = np.float32
DIFF, SPEC, REFR = gct.DIFF, gct.SPEC, gct.REFR
SPHERE = gt.SPHERE
INV_PI = F(0.318309886183790672)


def vertices(oracle, prims, params, o, d, unit, chain):
    """The guide's vertex of every ray -> (found bool (n,), id (n,), x (n, 3), nl (n, 3), segments (n,)):
    the first hit, or with `chain` the vertex where the chain guide takes its record (the first DIFF hit
    or the hit of the last segment). found is False where a segment missed."""
    d = np.array(d, dtype=F).reshape(-1, 3)
    o = np.array(np.broadcast_to(np.asarray(o, F), d.shape))
    n = len(d)
    KIND, REFL, COL, PLANE, CEN, INV_R = gct._tables(oracle, prims)
    found = np.zeros(n, dtype=bool)
    vid = np.full(n, -1, dtype=np.int64)
    vx, vnl = np.zeros((n, 3), dtype=F), np.zeros((n, 3), dtype=F)
    segs = np.zeros(n, dtype=np.int64)
    active = np.ones(n, dtype=bool)
    n_segs = gct.MAX_CHAIN if chain else 1
    for seg in range(n_segs):
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
        kind, refl = KIND[ids], REFL[ids]
        tr = t.copy()
        gn, nl = np.zeros((len(idx), 3), dtype=F), np.zeros((len(idx), 3), dtype=F)
        for k, axis in gct.AXIS:
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
            nl[m] = np.where((gct.dot3(g, dd[m]) < 0)[:, None], g, -g)
        end = (refl == DIFF) | (seg == n_segs - 1)
        e = idx[end]
        found[e], vid[e], vx[e], vnl[e] = True, ids[end], x[end], nl[end]
        active[e] = False
        c = ~end
        ci = idx[c]
        if ci.size == 0:
            continue
        dc, g, nlc = dd[c], gn[c], nl[c]
        k2 = (F(2.0) * gct.dot3(g, dc)).astype(F)
        nd = (dc - (g * k2[:, None]).astype(F)).astype(F)  # reflRay
        if unit:
            nd = gct._normalize(oracle, nd)
        r = refl[c] == REFR
        if r.any():
            gr, dr, nr = g[r], dc[r], nlc[r]
            into = gct.dot3(gr, nr) > 0
            nnt = np.where(into, F(1.0) / F(1.5), F(1.5) / F(1.0)).astype(F)
            ddn = gct.dot3(dr, nr)
            cos2t = (F(1.0) - ((nnt * nnt).astype(F) * (F(1.0) - (ddn * ddn).astype(F)).astype(F)).astype(F)).astype(F)
            ok = ~(cos2t < 0)  # else total internal reflection: the reflection
            with np.errstate(invalid="ignore"):
                root = np.sqrt(np.where(ok, cos2t, F(0.0))).astype(F)
            kk = (np.where(into, F(1.0), F(-1.0)) * ((ddn * nnt).astype(F) + root).astype(F)).astype(F)
            tdir = gct._normalize(oracle, ((dr * nnt[:, None]).astype(F) - (gr * kk[:, None]).astype(F)).astype(F))
            sub = nd[r]
            sub[ok] = tdir[ok]
            nd[r] = sub
        o[ci] = x[c]
        d[ci] = nd
    return found, vid, vx, vnl, segs


def nee_weight(oracle, unit, dl, nl, t2, light_area):
    """PDF_inverse * BRDF of a lit sample, the header's two forms."""
    light_area = F(light_area)
    tt = (t2 * t2).astype(F)
    if unit:
        pdf = np.abs(((light_area * dl[:, 1]).astype(F) * oracle.map_f32("rcp_nr", tt)).astype(F))
        brdf = np.abs((gct.dot3(dl, nl) * INV_PI).astype(F))
        return (pdf * brdf).astype(F)
    nee_c = F(np.float64(light_area) / np.pi)
    num = (np.abs(dl[:, 1]) * np.abs(gct.dot3(dl, nl))).astype(F)
    vv = gct.dot3(dl, dl)
    den = (tt * (vv * vv).astype(F)).astype(F)
    return ((num * nee_c).astype(F) * oracle.map_f32("rcp_nr", den)).astype(F)


def light_truth(oracle, prims, cam_c, params, chain=False, base=0, count=None, rows=None, return_detail=False):
    """The light guide's records (nrows, w, 4) int64 of the window [base, base + count) (default: all of
    [0, spp)) over `rows` (default: every image row). return_detail: also a dict of per-sample arrays
    (nrows, w, count): "tested", "lit", "vertex" (the vertex primitive, -1 without one), "segments",
    "weight" (float32, 0 where not lit), and "x" (nrows, w, count, 3), the vertex itself."""
    count = params.spp - base if count is None else count
    rows = np.arange(params.height) if rows is None else np.asarray(rows)
    w = params.width
    unit = gt.unit_dirs(prims)
    o, d = gt.camera_rays(oracle, cam_c, params, rows, base, count, unit)
    found, vid, x, nl, segs = vertices(oracle, prims, params, o, d.reshape(-1, 3), unit, chain)
    n = len(found)
    refl = np.array([p.refl for p in prims])
    tested = found & (refl[np.where(found, vid, 0)] == DIFF) & (vid != params.light_id)
    ti = np.flatnonzero(tested)
    # the light point: Philox word 2 = 0
    py, px = np.meshgrid(rows, np.arange(w), indexing="ij")
    words = np.empty((len(rows), w, count, 4), dtype=np.uint32)
    words[..., 0] = (py * w + px)[:, :, None]
    words[..., 1] = np.arange(base, base + count, dtype=np.uint32)[None, None, :]
    words[..., 2] = 0
    words[..., 3] = params.seed
    r = oracle.map_words("philox", words.reshape(-1, 4)[ti])
    ux = oracle.map_words("u01", r[:, 0]).view(F).reshape(-1)
    uz = oracle.map_words("u01", r[:, 1]).view(F).reshape(-1)
    xl = gt.fmaf(ux, F(params.light_dx), F(params.light_x0))
    zl = gt.fmaf(uz, F(params.light_dz), F(params.light_z0))
    xv = x[ti]
    dl = np.stack([(xl - xv[:, 0]).astype(F), (F(params.light_y) - xv[:, 1]).astype(F),
                   (zl - xv[:, 2]).astype(F)], axis=1).astype(F)
    if unit:
        dl = gct._normalize(oracle, dl)
    lit = np.zeros(n, dtype=bool)
    weight = np.zeros(n, dtype=F)
    rec = np.zeros((n, 4), dtype=np.int64)
    if ti.size:
        t2, id2 = oracle.intersect_batch(prims, params, np.ascontiguousarray(xv), np.ascontiguousarray(dl))
        li = id2 == params.light_id  # (a miss has id -1)
        lit[ti[li]] = True
        wt = nee_weight(oracle, unit, dl[li], nl[ti][li], t2[li], params.light_area)
        weight[ti[li]] = wt
        inv_spp = F(1.0) / F(params.spp)
        rec[ti[li], 2] = oracle.fix_batch(wt, inv_spp).astype(np.int64)
    rec[:, 0] = tested
    rec[:, 1] = lit
    out = rec.reshape(len(rows), w, count, 4).sum(axis=2)
    if not return_detail:
        return out
    shape = (len(rows), w, count)
    return out, {"tested": tested.reshape(shape), "lit": lit.reshape(shape),
                 "vertex": np.where(found, vid, -1).reshape(shape), "segments": segs.reshape(shape),
                 "weight": weight.reshape(shape), "x": x.reshape(shape + (3,))}


def resolve_numpy(records, spp_total, samples_done):
    """The resolve of include/spt.h as a numpy statement -> dict of the three float32 planes."""
    rec = np.asarray(records, dtype=np.int64)
    shape = rec.shape[:-1]
    n = int(samples_done)
    if n == 0:
        return {k: np.zeros(shape, F) for k in ("visibility", "direct", "tested")}
    tested, lit = rec[..., 0], rec[..., 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        vis = (lit.astype(np.float64) / tested.astype(np.float64)).astype(F)
    vis = np.where(tested != 0, vis, F(0.0)).astype(F)
    share = (tested.astype(np.float64) / np.float64(n)).astype(F)
    direct = rec[..., 2].astype(np.uint64).astype(F) * F(2.0 ** -31)
    if n != spp_total:
        direct = (direct * F(np.float64(spp_total) / np.float64(n))).astype(F)
    return {"visibility": vis, "direct": direct.astype(F), "tested": share}


def shade_numpy(albedo, visibility, shade_floor):
    """spt_light_shade's statement: a multiply, then an add, then the product per channel."""
    f = F(shade_floor)
    m = (f + ((F(1.0) - f) * np.asarray(visibility, F)).astype(F)).astype(F)
    return (np.asarray(albedo, F) * m[..., None]).astype(F)


def edited_light(spt, prims, params):
    """The `head` case with an edited light: light_x0 + 2 and light_dz 24 in the parameters, and the
    light primitive moved to match (its plane stays)."""
    params.light_x0 = params.light_x0 + 2.0
    params.light_dz = 24.0
    params.light_area = params.light_dx * params.light_dz
    x0, z0 = params.light_x0, params.light_z0
    return spt.edit_light(prims, x=(x0, x0 + params.light_dx), z=(z0, z0 + params.light_dz))


def light_params(spt, name, params):
    """The scene's light in the parameters. The classic box's light is prim 8, a sphere of radius 600
    whose cap reaches 0.27 below the ceiling (a disc of radius ~18 around (50, 81.6)): the sample
    rectangle is the 24 x 24 square inside that disc, at the ceiling's height (inside the sphere, so a
    shadow ray that reaches it hits the sphere first)."""
    if name in ("mirror_glass", "classic"):
        params.light_id = 8
        params.light_x0, params.light_dx = 38.0, 24.0
        params.light_z0, params.light_dz = 69.6, 24.0
        params.light_y = 81.6
        params.light_area = 576.0
    return params

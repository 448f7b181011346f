"""The two-half a-trous filter of include/spt.h (SPT_HAS_DENOISE_PAIR) restated in numpy float32 from
the header's text alone (a helper, not a test). It reuses denoise_truth's helpers: vectorised over the
pixels, a Python loop over the taps in the header's order, one rounding per operation, a skipped tap
leaves the sums as they are.
"""
import numpy as np

from denoise_truth import F, H5, NO_DEMODULATE, _dot3, _gradient, _phi, _tap

OWN_WEIGHTS = 1


def _vt(v):
    h, w = v.shape
    vs, ws = np.zeros((h, w), F), np.zeros((h, w), F)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            k = F((2 - abs(dy)) * (2 - abs(dx))) / F(16)
            vq, ok = _tap(v, dx, dy)
            vs = np.where(ok, vs + k * vq, vs)
            ws = np.where(ok, ws + k, ws)
    return vs / ws


def denoise_pair_truth(rgb_a, se_a, rgb_b, se_b, albedo, normal, depth, iterations=5, sigma_color=4.0,
                       sigma_depth=1.0, sigma_albedo=0.1, normal_squarings=7, albedo_floor=0.01, flags=0,
                       pair_flags=0, return_v=False):
    """-> (out, se_out, diff), each (h, w, 3) float32; return_v (iterations > 0): also the halves' final
    v planes (h, w)."""
    rgb_a, se_a, rgb_b, se_b, albedo, normal = (np.asarray(a, F) for a in
                                                (rgb_a, se_a, rgb_b, se_b, albedo, normal))
    z = np.asarray(depth, F)
    h, w = z.shape
    with np.errstate(all="ignore"):
        if iterations == 0:
            out = F(0.5) * (rgb_a + rgb_b)
            diff = F(0.5) * (rgb_a - rgb_b)
            se_out = F(0.5) * np.sqrt(se_a * se_a + se_b * se_b)
            return out, se_out, diff
        own = bool(pair_flags & OWN_WEIGHTS)
        sc2 = F(sigma_color) * F(sigma_color)
        sa2 = F(sigma_albedo) * F(sigma_albedo)
        sd = F(sigma_depth)
        a = np.ones_like(albedo) if flags & NO_DEMODULATE else np.fmax(albedo, F(albedo_floor))
        c, v = [], []
        for rgb, se in ((rgb_a, se_a), (rgb_b, se_b)):
            e = se / a
            c.append(rgb / a)
            v.append(((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]) * (F(1) / F(3)))
        gx, gy = _gradient(z, 1), _gradient(z, 0)
        for it in range(iterations):
            s = 1 << it
            vt = [_vt(v[0]), _vt(v[1])]
            W = [np.zeros((h, w), F), np.zeros((h, w), F)]
            V = [np.zeros((h, w), F), np.zeros((h, w), F)]
            C = [np.zeros((h, w, 3), F), np.zeros((h, w, 3), F)]
            for j in range(-2, 3):
                for i in range(-2, 3):
                    _, ok = _tap(z, i * s, j * s)
                    cq = [_tap(c[H], i * s, j * s)[0] for H in (0, 1)]
                    vq = [_tap(v[H], i * s, j * s)[0] for H in (0, 1)]
                    if i == 0 and j == 0:
                        wgt = [np.full((h, w), H5[2] * H5[2], F)] * 2
                    else:
                        nq, _ = _tap(normal, i * s, j * s)
                        zq, _ = _tap(z, i * s, j * s)
                        aq, _ = _tap(albedo, i * s, j * s)
                        wn = np.fmax(F(0), _dot3(normal, nq))
                        for _k in range(normal_squarings):
                            wn = wn * wn
                        dxf, dyf = F(i * s), F(j * s)
                        wz = _phi(np.abs(z - zq) / ((sd * np.abs(gx * dxf + gy * dyf) + F(1e-3) * z) + F(1e-6)))
                        da = albedo - aq
                        wa = _phi(_dot3(da, da) / sa2)
                        g = (((H5[j + 2] * H5[i + 2]) * wn) * wz) * wa
                        wc = []
                        for H in (0, 1):
                            vtq, _ = _tap(vt[H], i * s, j * s)
                            dc = c[H] - cq[H]
                            wc.append(_phi(_dot3(dc, dc) / (sc2 * (vt[H] + vtq) + F(1e-10))))
                        wgt = [g * wc[0], g * wc[1]] if own else [g * wc[1], g * wc[0]]
                    for H in (0, 1):
                        W[H] = np.where(ok, W[H] + wgt[H], W[H])
                        C[H] = np.where(ok[..., None], C[H] + wgt[H][..., None] * cq[H], C[H])
                        V[H] = np.where(ok, V[H] + (wgt[H] * wgt[H]) * vq[H], V[H])
            c = [C[H] / W[H][..., None] for H in (0, 1)]
            v = [V[H] / (W[H] * W[H]) for H in (0, 1)]
        oa, ob = np.fmin(c[0] * a, F(1)), np.fmin(c[1] * a, F(1))
        out = F(0.5) * (oa + ob)
        diff = F(0.5) * (oa - ob)
        se_out = (F(0.5) * np.sqrt(v[0] + v[1]))[..., None] * a
    assert out.dtype == F and se_out.dtype == F and diff.dtype == F
    return (out, se_out, diff, v[0], v[1]) if return_v else (out, se_out, diff)


def pair_summary_truth(diff):
    """-> {"rmse": [3 floats], "rmse_all", "diff_max"} in float64 (diff_max the exact float32 maximum)."""
    d = np.asarray(diff, F).astype(np.float64).reshape(-1, 3)
    s = (d * d).sum(axis=0)
    n = d.shape[0]
    return {"rmse": [float(np.sqrt(s[k] / n)) for k in range(3)],
            "rmse_all": float(np.sqrt(s.sum() / (3.0 * n))),
            "diff_max": float(np.abs(np.asarray(diff, F)).max())}


def synthetic_halves(w, h, seed=1, sigma=0.05, realisation=0):
    """denoise_truth.synthetic's clean image and guides with two independent noisy halves: each half is
    clean + N(0, (sigma * sqrt 2)^2) with se = sigma * sqrt 2 where synthetic's se > 0 (so their mean has
    the noise sigma of synthetic's single image). -> (rgb_a, se_a, rgb_b, se_b, albedo, normal, depth),
    and the clean image."""
    import denoise_truth as dt
    s = dt.synthetic(w, h, seed=seed, sigma=sigma)
    rng = np.random.default_rng([seed, 7919, realisation])
    sh = F(sigma * np.sqrt(2.0))
    se = np.where(s["se"] > 0, sh, F(0)).astype(F)
    halves = []
    for _ in range(2):
        noise = rng.normal(0.0, float(sh), s["rgb"].shape).astype(F)
        halves.append(np.where(se > 0, s["clean"] + noise, s["clean"]).astype(F))
    return (halves[0], se, halves[1], se.copy(), s["albedo"], s["normal"], s["depth"]), s["clean"]

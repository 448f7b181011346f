"""The filter bank of include/spt.h (SPT_HAS_DENOISE_BANK) restated in numpy float32 from the header's
text alone (a helper, not a test): the pair filter's two halves per candidate, the cross-validated error,
its smoothing with the geometric factor, the choice and the blend. Vectorised over the pixels, a Python
loop over the taps in the header's order, one rounding per operation, a skipped tap leaves the sums as
they are. Also the generators of the synthetic halves the bank's CPU and GPU tests share.
"""
import numpy as np

from denoise_truth import F, H5, NO_DEMODULATE, _dot3, _gradient, _phi, _tap

OWN_WEIGHTS = 1
DEFAULTS = dict(iterations=5, sigma_color=4.0, sigma_depth=1.0, sigma_albedo=0.1, normal_squarings=7,
                albedo_floor=0.01, flags=0)


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


def _geom(i, j, s, normal, z, albedo, gx, gy, sd, sa2, squarings):
    """g of the tap (i, j) at step s for every pixel (not the centre tap)."""
    nq, _ = _tap(normal, i * s, j * s)
    zq, _ = _tap(z, i * s, j * s)
    aq, _ = _tap(albedo, i * s, j * s)
    wn = np.fmax(F(0), _dot3(normal, nq))
    for _k in range(squarings):
        wn = wn * wn
    dxf, dyf = F(i * s), F(j * s)
    wz = _phi(np.abs(z - zq) / ((sd * np.abs(gx * dxf + gy * dyf) + F(1e-3) * z) + F(1e-6)))
    da = albedo - aq
    wa = _phi(_dot3(da, da) / sa2)
    return (((H5[j + 2] * H5[i + 2]) * wn) * wz) * wa


def pair_halves_truth(rgb_a, se_a, rgb_b, se_b, albedo, normal, z, pair_flags, iterations, sigma_color,
                      sigma_depth, sigma_albedo, normal_squarings, albedo_floor, flags):
    """-> (o^A, o^B): the pair statement's finish values of the two halves, (h, w, 3) float32 each."""
    if iterations == 0:
        return rgb_a.copy(), rgb_b.copy()
    h, w = z.shape
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
                    g = _geom(i, j, s, normal, z, albedo, gx, gy, sd, sa2, normal_squarings)
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
    return np.fmin(c[0] * a, F(1)), np.fmin(c[1] * a, F(1))


def _choice(m):
    """m: (n, h, w) -> the smallest k whose m_k is least, by `<` with k ascending."""
    k = np.zeros(m.shape[1:], np.uint8)
    best = m[0]
    for j in range(1, m.shape[0]):
        less = m[j] < best
        k = np.where(less, np.uint8(j), k)
        best = np.where(less, m[j], best)
    return k


def denoise_bank_truth(rgb_a, se_a, rgb_b, se_b, albedo, normal, depth, cands, error_iterations=2,
                       pair_flags=OWN_WEIGHTS):
    """cands: a list of dicts of spt_denoise_params fields (missing ones: DEFAULTS).
    -> (out (h, w, 3) float32, mse (h, w) float32, choice (h, w) uint8)."""
    rgb_a, se_a, rgb_b, se_b, albedo, normal = (np.asarray(a, F) for a in
                                                (rgb_a, se_a, rgb_b, se_b, albedo, normal))
    z = np.asarray(depth, F)
    h, w = z.shape
    cands = [dict(DEFAULTS, **c) for c in cands]
    n = len(cands)
    with np.errstate(all="ignore"):
        outk, m = [], []
        for c in cands:
            oa, ob = pair_halves_truth(rgb_a, se_a, rgb_b, se_b, albedo, normal, z, pair_flags, **c)
            outk.append(F(0.5) * (oa + ob))
            d = F(0.5) * (oa - ob)
            ra, rb = oa - rgb_b, ob - rgb_a
            e = F(0.5) * ((ra * ra - se_b * se_b) + (rb * rb - se_a * se_a))
            mc = e - d * d
            m.append(((mc[..., 0] + mc[..., 1]) + mc[..., 2]) * (F(1) / F(3)))
        m = np.stack(m)
        sd = F(cands[0]["sigma_depth"])
        sa2 = F(cands[0]["sigma_albedo"]) * F(cands[0]["sigma_albedo"])
        squarings = cands[0]["normal_squarings"]
        gx, gy = _gradient(z, 1), _gradient(z, 0)

        def taps(s):
            for j in range(-2, 3):
                for i in range(-2, 3):
                    _, ok = _tap(z, i * s, j * s)
                    g = (np.full((h, w), H5[2] * H5[2], F) if i == 0 and j == 0 else
                         _geom(i, j, s, normal, z, albedo, gx, gy, sd, sa2, squarings))
                    yield i * s, j * s, ok, g

        for it in range(error_iterations):
            W, M = np.zeros((h, w), F), np.zeros((n, h, w), F)
            for ox, oy, ok, g in taps(1 << it):
                W = np.where(ok, W + g, W)
                for k in range(n):
                    M[k] = np.where(ok, M[k] + g * _tap(m[k], ox, oy)[0], M[k])
            m = M / W
        choice = _choice(m)
        W, S = np.zeros((h, w), F), np.zeros((n, h, w), F)
        for ox, oy, ok, g in taps(1):
            W = np.where(ok, W + g, W)
            kq, _ = _tap(choice, ox, oy)
            for k in range(n):
                S[k] = np.where(ok, S[k] + g * np.where(kq == k, F(1), F(0)), S[k])
        s = S / W
        out, mse = np.zeros((h, w, 3), F), np.zeros((h, w), F)
        for k in range(n):
            out = out + s[k][..., None] * outk[k]
            mse = mse + s[k] * m[k]
        out = np.fmin(out, F(1))
    assert out.dtype == F and mse.dtype == F and choice.dtype == np.uint8
    return out, mse, choice


def bank_summary_truth(mse, choice):
    """-> {"mse_mean", "rmse_est", "share": [4], "mse_min", "mse_max"} in float64 (min and max the exact
    float32 values)."""
    m = np.asarray(mse, F)
    mean = float(m.astype(np.float64).sum() / m.size)
    return {"mse_mean": mean, "rmse_est": float(np.sqrt(max(0.0, mean))),
            "share": [float((np.asarray(choice) == k).sum() / m.size) for k in range(4)],
            "mse_min": float(m.min()), "mse_max": float(m.max())}


def bank_halves(w, h, seed=1, sigma=0.05, realisation=0):
    """The edge cases of denoise_truth.synthetic (two regions, misses, clamped pixels) as two halves whose
    noise differs: half A with sigma * sqrt 2, half B with sigma * 2 (se the exact standard deviations), so
    that swapping the halves swaps different planes. -> the seven planes."""
    import denoise_truth as dt
    s = dt.synthetic(w, h, seed=seed, sigma=sigma)
    rng = np.random.default_rng([seed, 104729, realisation])
    planes = []
    for scale in (np.sqrt(2.0), 2.0):
        sh = F(sigma * scale)
        se = np.where(s["se"] > 0, sh, F(0)).astype(F)
        noise = rng.normal(0.0, float(sh), s["rgb"].shape).astype(F)
        planes += [np.where(se > 0, s["clean"] + noise, s["clean"]).astype(F), se]
    return planes + [s["albedo"], s["normal"], s["depth"]]


DETAIL_X0 = 32  # calibration_halves: columns below are flat, the others carry the colour-only detail


def calibration_halves(w=64, h=48, sigma=0.02, amplitude=0.06, realisation=0, seed=1):
    """One plane facing the camera with a constant albedo 0.5, a constant normal and a gentle depth ramp,
    so that no guide separates anything. The clean colour is 0.4 for x < DETAIL_X0 (flat) and 0.4 +-
    amplitude in a checkerboard of 2 x 2 pixel squares elsewhere (detail that only the colours carry). Each
    half is clean + N(0, (sigma * sqrt 2)^2) with NO clamping, and its se plane is that standard deviation
    exactly. -> (the seven planes, the clean image)."""
    y, x = np.mgrid[0:h, 0:w]
    check = np.where(((x // 2) + (y // 2)) % 2 == 0, 1.0, -1.0)
    lum = np.where(x < DETAIL_X0, 0.4, 0.4 + amplitude * check)
    clean = np.repeat(lum[..., None], 3, axis=2).astype(F)
    albedo = np.full((h, w, 3), 0.5, F)
    normal = np.zeros((h, w, 3), F)
    normal[..., 2] = 1
    depth = (10 + 0.01 * x + 0.02 * y).astype(F)
    sh = F(sigma * np.sqrt(2.0))
    se = np.full((h, w, 3), sh, F)
    rng = np.random.default_rng([seed, 15485863, realisation])
    halves = [(clean + rng.normal(0.0, float(sh), clean.shape).astype(F)).astype(F) for _ in range(2)]
    return (halves[0], se, halves[1], se.copy(), albedo, normal, depth), clean

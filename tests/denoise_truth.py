"""The a-trous filter of include/spt.h (SPT_HAS_DENOISE) restated in numpy float32 from the header's
text alone (a helper, not a test). Vectorised over the pixels, a Python loop over the taps in the
header's order, so every pixel sees the header's operation sequence: one rounding per operation, no
fused multiply-add, a skipped tap leaves the sums as they are (np.where keeps the old value).

Also the generator of synthetic planes the CPU and the GPU tests share.
"""
import numpy as np

F = np.float32
NO_DEMODULATE = 1
H5 = [F(1) / F(16), F(4) / F(16), F(6) / F(16), F(4) / F(16), F(1) / F(16)]


def _phi(x):
    t = np.fmax(F(0), F(1) - F(0.25) * x)
    t = t * t
    return t * t


def _tap(plane, ox, oy):
    """plane shifted so that element (y, x) holds plane(y + oy, x + ox), and the mask of the places
    where that tap lies inside the image (elsewhere the value is arbitrary)."""
    h, w = plane.shape[:2]
    ys, xs = np.arange(h) + oy, np.arange(w) + ox
    valid = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]
    return plane[np.clip(ys, 0, h - 1)][:, np.clip(xs, 0, w - 1)], valid


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _gradient(z, axis):
    n = z.shape[axis]
    g = np.zeros_like(z)
    if n == 1:
        return g
    zz = np.moveaxis(z, axis, 0)
    gg = np.moveaxis(g, axis, 0)
    gg[1:-1] = F(0.5) * (zz[2:] - zz[:-2])
    gg[0] = zz[1] - zz[0]
    gg[-1] = zz[-1] - zz[-2]
    return g


def denoise_truth(rgb, se, albedo, normal, depth, iterations=5, sigma_color=4.0, sigma_depth=1.0,
                  sigma_albedo=0.1, normal_squarings=7, albedo_floor=0.01, flags=0):
    """-> (out, se_out), both (h, w, 3) float32."""
    rgb, se, albedo, normal = (np.asarray(a, F) for a in (rgb, se, albedo, normal))
    z = np.asarray(depth, F)
    h, w = z.shape
    if iterations == 0:
        return rgb.copy(), se.copy()
    sc2 = F(sigma_color) * F(sigma_color)
    sa2 = F(sigma_albedo) * F(sigma_albedo)
    sd = F(sigma_depth)
    with np.errstate(all="ignore"):
        a = np.ones_like(albedo) if flags & NO_DEMODULATE else np.fmax(albedo, F(albedo_floor))
        c = rgb / a
        e = se / a
        v = ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]) * (F(1) / F(3))
        gx, gy = _gradient(z, 1), _gradient(z, 0)
        for it in range(iterations):
            s = 1 << it
            vs, ws = np.zeros((h, w), F), np.zeros((h, w), F)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    k = F((2 - abs(dy)) * (2 - abs(dx))) / F(16)
                    vq, ok = _tap(v, dx, dy)
                    vs = np.where(ok, vs + k * vq, vs)
                    ws = np.where(ok, ws + k, ws)
            vt = vs / ws
            W, V = np.zeros((h, w), F), np.zeros((h, w), F)
            C = np.zeros((h, w, 3), F)
            for j in range(-2, 3):
                for i in range(-2, 3):
                    cq, ok = _tap(c, i * s, j * s)
                    vq, _ = _tap(v, i * s, j * s)
                    if i == 0 and j == 0:
                        wgt = np.full((h, w), H5[2] * H5[2], F)
                    else:
                        nq, _ = _tap(normal, i * s, j * s)
                        zq, _ = _tap(z, i * s, j * s)
                        aq, _ = _tap(albedo, i * s, j * s)
                        vtq, _ = _tap(vt, i * s, j * s)
                        wn = np.fmax(F(0), _dot3(normal, nq))
                        for _k in range(normal_squarings):
                            wn = wn * wn
                        dxf, dyf = F(i * s), F(j * s)
                        wz = _phi(np.abs(z - zq) / ((sd * np.abs(gx * dxf + gy * dyf) + F(1e-3) * z) + F(1e-6)))
                        da = albedo - aq
                        wa = _phi(_dot3(da, da) / sa2)
                        dc = c - cq
                        wc = _phi(_dot3(dc, dc) / (sc2 * (vt + vtq) + F(1e-10)))
                        wgt = ((((H5[j + 2] * H5[i + 2]) * wn) * wz) * wa) * wc
                    W = np.where(ok, W + wgt, W)
                    C = np.where(ok[..., None], C + wgt[..., None] * cq, C)
                    V = np.where(ok, V + (wgt * wgt) * vq, V)
            c = C / W[..., None]
            v = V / (W * W)
        out = np.fmin(c * a, F(1))
        se_out = np.sqrt(v)[..., None] * a
    assert out.dtype == F and se_out.dtype == F
    return out, se_out


def synthetic(w, h, seed=1, sigma=0.05):
    """Two planar regions side by side (x < w // 2 and the rest) with orthogonal unit normals,
    distinct albedos and their own depth ramps, lit by a smooth ramp; a few miss pixels (all features
    zero, a flat background colour) and a few clamped pixels (rgb = 1, se = 0); Gaussian noise of
    standard deviation sigma on every other pixel, se = sigma there. -> dict of float32 planes: rgb, se,
    albedo, normal, depth, clean, and the int plane region (0, 1; 2 miss, 3 clamped)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    right = x >= w // 2
    region = right.astype(np.int32)
    albedo = np.where(right[..., None], F([0.2, 0.6, 0.8]), F([0.7, 0.3, 0.25])).astype(F)
    normal = np.where(right[..., None], F([1, 0, 0]), F([0, 0, 1])).astype(F)
    depth = np.where(right, 20 - 0.1 * x + 0.02 * y, 10 + 0.05 * x + 0.03 * y).astype(F)
    light = (0.5 + 0.3 * y / max(h - 1, 1) + 0.1 * x / max(w - 1, 1)).astype(F)
    clean = (albedo * light[..., None]).astype(F)
    se = np.full((h, w, 3), sigma, F)
    npix = w * h
    k = max(1, npix // 500) if npix >= 6 else 0
    special = rng.choice(npix, size=2 * k, replace=False) if k else np.zeros(0, np.int64)
    for n, p in enumerate(special):
        py, px = divmod(int(p), w)
        if n < k:  # a miss
            albedo[py, px] = normal[py, px] = 0
            depth[py, px] = 0
            clean[py, px] = 0.25
            region[py, px] = 2
        else:      # a clamped pixel
            clean[py, px] = 1
            se[py, px] = 0
            region[py, px] = 3
    noise = rng.normal(0.0, sigma, (h, w, 3)).astype(F)
    rgb = np.where(se > 0, clean + noise, clean).astype(F)
    return {"rgb": rgb, "se": se, "albedo": albedo, "normal": normal, "depth": depth, "clean": clean,
            "region": region}


PLANES = ("rgb", "se", "albedo", "normal", "depth")


def planes_of(s):
    return [s[k] for k in PLANES]

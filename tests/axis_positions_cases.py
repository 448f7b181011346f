"""The rays of tests/test_gpu_axis_positions.py and their non-vacuity count (a helper, not a test).

The literal kernels number their primitive slots so that bits 4 and 5 of a winning key name the hit's
plane axis (spt_cornell.h, cornell_slot). A key's low six bits are only the tie-break among candidates
whose t share the upper 26 bits, so a wrong slot can change a winner only there -- and only between
rectangles of different kinds, whose order the renumbering has to keep. Such ties sit where planes of
two axes meet: the room's corners and edges, the boxes' corners and top edges. The rays here run from
inside the room at those points and at their one-ulp neighbours.

A ray is a camera of four raw vectors with horizontal = vertical = 0 (tests/test_gpu_rays.py): origin,
lower_left_corner = the target. The direction the kernel traces is the contract's normalised
lower_left_corner - origin, restated by guide_truth.camera_rays from the oracle's pieces.
"""
import numpy as np

import guide_truth as gt
import ray_truth as rt

F = np.float32
ORIGINS = [(50.0, 40.0, 100.0), (30.0, 60.0, 140.0), (70.0, 10.0, 20.0)]
SPP = 8  # samples of a single-ray render of the scene itself (every one starts with the same ray)


def targets(spt, oracle, prims):
    """[(label, point float32 (3,))]: the eight room corners, the twelve room edges' midpoints, and the
    eight corners and the four top edges' midpoints of each box, on the planes' fp32 coordinates."""
    k = lambda i: oracle.plane_k(prims[i].geom[4])  # noqa: E731
    lo = np.array([k(2), k(4), k(0)], dtype=np.float64)
    hi = np.array([k(3), k(5), k(1)], dtype=np.float64)
    out = []

    def box(name, lo, hi, edges):
        mid = (lo + hi) * 0.5
        for c in range(8):
            sel = [(c >> a) & 1 for a in range(3)]
            out.append((f"{name}_corner{c}", np.where(sel, hi, lo)))
        for a in range(3):  # the edges along axis a: the other two coordinates at lo or hi
            b, c = [x for x in range(3) if x != a]
            for sb in (0, 1):
                for sc in (0, 1):
                    if edges == "top" and not ((b == 1 and sb == 1) or (c == 1 and sc == 1)):
                        continue  # a box: only the edges of its top face (y = hi)
                    p = mid.copy()
                    p[b] = (lo, hi)[sb][b]
                    p[c] = (lo, hi)[sc][c]
                    out.append((f"{name}_edge{a}{sb}{sc}", p))

    box("room", lo, hi, "all")
    for name, (z0, z1, x0, x1, top) in (("tall", (7, 8, 9, 10, 11)), ("short", (12, 13, 14, 15, 16))):
        box(name, np.array([k(x0), lo[1], k(z0)]), np.array([k(x1), k(top), k(z1)]), "top")
    return [(label, p.astype(F)) for label, p in out]


def rays(spt, oracle, prims, origin):
    """[(label, target float32 (3,))] from one origin: every target and its six neighbours one ulp to
    either side in one component."""
    out = []
    for label, p in targets(spt, oracle, prims):
        if np.array_equal(p, np.asarray(origin, F)):
            continue
        out.append((label, p))
        for a in range(3):
            for s, to in (("+", np.inf), ("-", -np.inf)):
                q = p.copy()
                q[a] = np.nextafter(p[a], F(to))
                out.append((f"{label}_{'xyz'[a]}{s}", q))
    return out


def ray_camera(spt, origin, target):
    cam = spt.Camera()
    for i in range(3):
        cam._c.origin[i] = float(origin[i])
        cam._c.lower_left_corner[i] = float(target[i])
        cam._c.horizontal[i] = cam._c.vertical[i] = 0.0
    return cam


def traced_dirs(spt, oracle, origin, tgts):
    """The directions the kernel traces for these rays (free-scale contract): (n, 3) float32."""
    p = spt.default_params(width=1, height=1, spp=1, seed=5)
    d = np.empty((len(tgts), 3), dtype=F)
    for i, t in enumerate(tgts):
        _, di = gt.camera_rays(oracle, ray_camera(spt, origin, t)._c, p, [0], 0, 1, False)
        d[i] = di.reshape(3)
    return d


def plane_ts(oracle, prims, origin, d):
    """The contract's plane distance of every rectangle (oracle c_plane_t): fma(k - o_a, rcp_nr(d_a),
    -2^-149) in fp32, (n, prims) float32."""
    o = np.asarray(origin, F)
    inv = oracle.map_words("rcp_nr", d.reshape(-1).view(np.uint32)).view(F).reshape(d.shape)
    t = np.empty((len(d), len(prims)), dtype=F)
    for i, pr in enumerate(prims):
        ax = rt.AXES[pr.kind][0]
        t[:, i] = gt.fmaf(F(oracle.plane_k(pr.geom[4])) - o[ax], inv[:, ax], F(-2.0 ** -149))
    return t


SLACK = 1e-3  # a candidate: the plane's crossing lies within its rectangle's bounds or this close to them


def axis_ties(spt, oracle, prims, origin, d):
    """Per ray: do the two nearest candidates lie on planes of different axes and agree in the upper
    26 bits of t? A candidate is a rectangle whose plane the ray crosses at a positive contract t
    (plane_ts) inside its bounds, or within SLACK of them: at an edge the in-plane test's rounding
    decides, which is the case this counts. (n,) bool."""
    o64 = np.asarray(origin, F).astype(np.float64)
    d64 = d.astype(np.float64)
    t = plane_ts(oracle, prims, origin, d)
    keys = np.full(t.shape, 0xFFFFFFFF, dtype=np.uint64)
    for i, pr in enumerate(prims):
        _, a, b = rt.AXES[pr.kind]
        g = pr.geom
        x = o64[None, :] + d64 * t[:, i:i + 1].astype(np.float64)
        with np.errstate(invalid="ignore"):
            ok = ((t[:, i] > 0) & (t[:, i] < 1e20) & (x[:, a] >= g[0] - SLACK) & (x[:, a] <= g[1] + SLACK) &
                  (x[:, b] >= g[2] - SLACK) & (x[:, b] <= g[3] + SLACK))
        keys[:, i] = np.where(ok, t[:, i].view(np.uint32).astype(np.uint64), 0xFFFFFFFF)
    order = np.argsort(keys, axis=1, kind="stable")
    rows = np.arange(len(d))
    k0, k1 = keys[rows, order[:, 0]], keys[rows, order[:, 1]]
    kind = np.array([pr.kind for pr in prims])
    return (k1 != 0xFFFFFFFF) & ((k0 >> 6) == (k1 >> 6)) & (kind[order[:, 0]] != kind[order[:, 1]])

"""A float64 replay of the estimator, sample by sample: what happens between a hit and the next ray.
Shared by tests/test_contract_shade.py (the CPU oracle against this truth) and tests/test_gpu_shade.py
(the library's kernels against it).

Written from DESIGN.md section 3 and the reference's lines cited there, not from the oracle's code:
the camera ray (:533-536) from the camera's doubles rounded to float with the 16-bit jitter; the
vertex loop (:419-496): emission, the RR rule (:448), max_depth; at a DIFF vertex the light point
(:365-367, the wrap lattice or the uniform rectangle, plane and area from the params), "reaches" =
the fp64 nearest hit is light_id (:466-467), the weight |area dl.y / t^2| |dl.nl| / pi (:471-472)
with unit dl and the true distance (the free-scale contract states the same number), otherwise the
cosine / uniform scatter (:340-359, contract_truth.cosine_truth); at a SPEC / REFR vertex the
commented-out lines :482-495: the mirror direction, Snell, Schlick with R0 = .04, both children
weighted Re / Tr at depth <= 2 and the roulette P = 1/4 + Re/2 beyond, the refraction child of the
split at depth k drawing its words with bit 24 + k - 1 of the counter's vertex word set. Random
words are oracle.map_words("philox", ...), which test_philox_batch_is_the_contracts_generator pins.
Geometry is ray_truth.Truth's, on float64 rays; a ray does not re-hit the rectangle it starts on.

The replay is vectorised over a frontier of path-tree nodes; a split appends both children (the
order of the sums is irrelevant in float64; the kernels' depth-first stack is pinned by the values:
a child popped early or late draws other words and carries another weight).
"""
import numpy as np

import contract_truth as ct
import ray_truth as rt

DIFF, SPEC, REFR = 0, 1, 2
FLAG_UNIFORM_SCATTER = 1
LIGHT_WRAP, LIGHT_UNIFORM = 0, 1
MARGIN = 1e-3


def _words(oracle, pix, s, word2, seed):
    c = np.empty((len(pix), 4), dtype=np.uint32)
    c[:, 0], c[:, 1], c[:, 2], c[:, 3] = pix, s, word2, seed
    return oracle.map_words("philox", c)


def _u16(lo, hi):
    return ((lo & np.uint32(0xFF)) | ((hi & np.uint32(0xFF)) << np.uint32(8))).astype(np.float64) * 2.0 ** -16


def _dot(a, b):
    return (a * b).sum(axis=1)


class Scene:
    """The scene's float64 geometry (ray_truth.Truth) and materials."""

    def __init__(self, oracle, prims):
        self.T = rt.Truth(oracle, prims)
        self.prims = prims
        self.kind = np.array([p.kind for p in prims])
        self.refl = np.array([p.refl for p in prims])
        self.e = np.array([list(p.e) for p in prims], dtype=np.float64)
        self.c = np.array([list(p.c) for p in prims], dtype=np.float64)
        self.pmax = self.c.max(axis=1)  # :447
        self.axis = np.array([rt.AXES[p.kind][0] if p.kind != rt.SPHERE else -1 for p in prims])
        self.centre = np.zeros((len(prims), 3))
        self.radius = np.ones(len(prims))
        for i, r, c in self.T.spheres:
            self.centre[i], self.radius[i] = c, r

    def nearest(self, o, d, own, shadow=False, shadow_to=-1):
        """(id, t, margin) of float64 rays; `own` = the rectangle a ray starts on (-1: none), which
        it cannot hit. margin = the smallest distance of any decision from its threshold: the gap to
        the second nearest hit, the distance to an edge of every rectangle whose plane lies at or
        before the hit (a near miss decides as much as a near hit), of the ray's line to every
        sphere's surface in front of the hit, of every sphere root to the 2e-3 epsilon, and |d_a|
        (a ray with an exactly zero component misses the room in the contract)."""
        T = self.T
        n = len(o)
        t = np.full((n, T.n), np.inf)
        edge = np.full((n, T.n), np.inf)   # |signed distance| of a decision, with the t it applies at
        at = np.full((n, T.n), np.inf)
        eps_m = np.full(n, np.inf)
        outside = np.zeros(n)
        with np.errstate(divide="ignore", invalid="ignore"):
            for i, ax, a, b, k, ma, ha, mb, hb in T.rects:
                tt = (k - o[:, ax]) / d[:, ax]
                ea = ha - np.abs(o[:, a] + d[:, a] * tt - ma)
                eb = hb - np.abs(o[:, b] + d[:, b] * tt - mb)
                ok = (d[:, ax] != 0) & (tt > 0) & (own != i)
                t[:, i] = np.where(ok & (ea >= 0) & (eb >= 0), tt, np.inf)
                edge[:, i] = np.where(ok, np.abs(np.minimum(ea, eb)), np.inf)
                at[:, i] = np.where(ok, tt, np.inf)
                if shadow and i == shadow_to:
                    outside = np.where(ok, -np.minimum(ea, eb), np.inf)
            aa = _dot(d, d)
            for i, r, c in T.spheres:
                op = c[None, :] - o
                kk = _dot(op, d) / aa
                q = op - kk[:, None] * d
                det = r * r - _dot(q, q)
                sd = np.sqrt(np.where(det >= 0, det, np.nan) / aa)
                t1, t2 = kk - sd, kk + sd
                t[:, i] = np.where(t1 > rt.EPS, t1, np.where(t2 > rt.EPS, t2, np.inf))
                ahead = np.nan_to_num(kk + np.nan_to_num(sd), nan=-1.0) > 0
                edge[:, i] = np.where(ahead, np.abs(r - np.sqrt(_dot(q, q))), np.inf)
                at[:, i] = np.where(ahead, np.maximum(kk - r, 0.0), np.inf)
                for root in (t1, t2):
                    eps_m = np.fmin(eps_m, np.where(np.isnan(root), np.inf, np.abs(root - rt.EPS)))
        order = np.argsort(t, axis=1, kind="stable")
        rows = np.arange(n)
        t0 = t[rows, order[:, 0]]
        t1_ = t[rows, order[:, 1]] if T.n > 1 else np.full(n, np.inf)
        ids = np.where(np.isfinite(t0), order[:, 0], rt.MISS)
        with np.errstate(invalid="ignore"):
            gap = np.where(np.isfinite(t1_), t1_ - t0, np.inf)
            before = at <= (t0 + MARGIN)[:, None]
        m = np.minimum(gap, np.where(before, edge, np.inf).min(axis=1))
        m = np.minimum(m, eps_m)
        if not shadow:
            return ids, t0, np.where(ids >= 0, np.minimum(m, np.abs(d).min(axis=1)), 0.0)
        # a shadow ray decides one thing, whether it reaches the light. Where the truth does not
        # reach it a zero component changes nothing (the contract then misses everything: no reach
        # either; the rays from the ceiling towards a light point at the ceiling's height), and
        # a ray that passes the light's rectangle far outside its edges does not reach it whatever
        # else it grazes
        return ids, t0, np.where(ids == shadow_to, np.minimum(m, np.abs(d).min(axis=1)),
                                 np.maximum(m, outside))


def camera_rays(oracle, cam, w, h, pix, s, seed):
    """:533-536: d = norm(llc + hor su + ver sv - origin), su = (x - .5 + ju 2^-16) / w, sv =
    (h - y - 1 - .5 + jv 2^-16) / h; the camera's doubles rounded to float as the host passes them
    on; ju, jv = the low bytes of vertex 1's words 0, 1 and 2, 3."""
    f = lambda v: np.array([rt.f32(x) for x in v], dtype=np.float64)  # noqa: E731
    o, llc, hor, ver = f(cam.origin), f(cam.lower_left_corner), f(cam.horizontal), f(cam.vertical)
    r = _words(oracle, pix, s, np.uint32(1), seed)
    x, y = (pix % w).astype(np.float64), (pix // w).astype(np.float64)
    su = (x - 0.5 + _u16(r[:, 0], r[:, 1])) / w
    sv = (h - y - 1 - 0.5 + _u16(r[:, 2], r[:, 3])) / h
    d = llc[None] + hor[None] * su[:, None] + ver[None] * sv[:, None] - o[None]
    return np.tile(o, (len(pix), 1)), rt.unit(d)


def _light_points(p, r0, r1):
    """:365-366. Wrap lattice: x0 - 1 + (r >> (7 + a)) 2^(a - 24) for an edge
    dx = 2^a odd; uniform: x0 + u01(r) dx."""
    out = []
    for r, x0, dx in ((r0, p.light_x0, p.light_dx), (r1, p.light_z0, p.light_dz)):
        if p.light_mode == LIGHT_UNIFORM:
            out.append(float(x0) + ct.u01_truth(r) * float(dx))
            continue
        dxi = int(dx)
        assert dxi == dx and dxi > 0 and dxi % 2 == 0, "the truth states the wrap lattice for even edges"
        a = (dxi & -dxi).bit_length() - 1
        out.append(float(x0) - 1.0 + (r >> np.uint32(7 + a)).astype(np.float64) * 2.0 ** (a - 24))
    return out


def _scatter(nl, ra, rb, uniform):
    out = np.empty((len(nl), 3))
    keys = {}
    for j, v in enumerate(map(tuple, nl)):
        keys.setdefault(v, []).append(j)
    for v, rows in keys.items():
        rows = np.array(rows)
        out[rows] = ct.cosine_truth(np.array(v), ra[rows], rb[rows], uniform)
    return out


class Result:
    pass


def replay(oracle, prims, cam, p, shift=None, scene=None, depth_cap=None):
    """Every sample of the image p describes (p.width x p.height x p.spp), in float64.

    shift = (k, s, axis): the k-th vertex of every path is displaced by s times the contract's error
    of that hit, for the first-order bound: axis 0 along its incoming ray by ray_truth.t_bound, axes
    1 and 2 across it by the roundings of x = o + d t and of the direction. depth_cap ends displaced
    paths that do not end by themselves (their signature is then another one).

    Returns a Result with, per sample (index (y w + x) spp + s): L (n, 3) unclamped; margin; v1 (the
    first vertex's prim, -1 a miss); reach (a DIFF first vertex whose shadow ray reaches the light);
    alt_e1, alt_scatter (n, 3): L had the first vertex's shadow ray not reached the light -- the
    scatter ray of :468 is taken instead, stopped by the vertex's own wall (nothing after e1) or
    not; closed: the path ends without help from max_depth by its second vertex; internal_exit: a
    glass path that reflects inside a ball and later leaves it; cls: 0 wall / 1 mirror / 2 glass
    (the first vertex's material class); depth: the deepest vertex; sig: a signature of the tree's
    decisions (which prim at which node), to tell a displaced replay that decided otherwise."""
    S = scene or Scene(oracle, prims)
    w, h, spp = p.width, p.height, p.spp
    n = w * h * spp
    pix_all = (np.arange(n) // spp).astype(np.uint32)
    s_all = (np.arange(n) % spp).astype(np.uint32)
    uniform = bool(p.flags & FLAG_UNIFORM_SCATTER)
    R = Result()
    R.L = np.zeros((n, 3))
    R.margin = np.full(n, np.inf)
    R.v1 = np.full(n, -1)
    R.reach = np.zeros(n, dtype=bool)
    R.alt_e1 = np.zeros((n, 3))
    R.alt_scatter = np.zeros((n, 3))
    R.closed = np.zeros(n, dtype=bool)
    R.has_alt = np.zeros(n, dtype=bool)
    R.internal_exit = np.zeros(n, dtype=bool)
    R.depth = np.zeros(n, dtype=np.int64)
    R.sig = np.zeros(n, dtype=np.int64)  # the path tree's decisions: which prim at which node

    o, d = camera_rays(oracle, cam, w, h, pix_all, s_all, p.seed)
    idx = np.arange(n)
    Tw = np.ones((n, 3))
    depth = np.zeros(n, dtype=np.int64)
    branch = np.zeros(n, dtype=np.uint32)
    own = np.full(n, -1)
    car_id = np.full(n, -2)          # >= -1: the nearest hit is known (the shadow ray's)
    car_t = np.zeros(n)
    inside = np.zeros(n, dtype=bool)  # reflected inside a ball so far
    alt = np.zeros(n, dtype=bool)     # this node is the alternative (scatter) child of vertex 1

    while len(idx):
        ids, t, m = S.nearest(o, d, own)
        known = car_id >= -1
        ids, t, m = np.where(known, car_id, ids), np.where(known, car_t, t), np.where(known, np.inf, m)
        np.minimum.at(R.margin, idx[~alt], m[~alt])
        hit = ids >= 0
        # a miss: outside the issue's scope, excluded by its margin of 0; the node ends
        (idx, o, d, Tw, depth, branch, own, ids, t, inside, alt) = [
            a[hit] for a in (idx, o, d, Tw, depth, branch, own, ids, t, inside, alt)]
        if not len(idx):
            break
        depth = depth + 1
        if depth_cap is not None and (depth > depth_cap).any():  # a displaced path that does not end
            live = depth <= depth_cap
            R.sig[idx[~live]] = -1
            (idx, o, d, Tw, depth, branch, own, ids, t, inside, alt) = [
                a[live] for a in (idx, o, d, Tw, depth, branch, own, ids, t, inside, alt)]
            if not len(idx):
                break
        if shift is not None:
            sel = (depth == shift[0]) & (shift[2] == 0)
            if sel.any():
                t = t.copy()
                t[sel] += shift[1] * rt.t_bound(S.T, S.prims, o[sel], d[sel], ids[sel], t[sel])
        x = o + d * t[:, None]
        if shift is not None and shift[2] and (depth == shift[0]).any():
            # across the ray: x = o + d t rounds a product and a sum per component, 3 2^-24 max|x_c|
            # at most, and the direction carries its normalisation's error (RSQ_NR_REL and three
            # roundings of its own, 2 RSQ_NR_REL together) over the distance t
            sel = depth == shift[0]
            dn = rt.unit(d[sel])
            helper = np.where((np.abs(dn[:, 1:2]) < 0.9), [[0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0]])
            u = rt.unit(np.cross(dn, helper))
            across = u if shift[2] == 1 else np.cross(dn, u)
            amount = 3 * 2.0 ** -24 * np.abs(x[sel]).max(axis=1) + 2 * ct.RSQ_NR_REL * t[sel] * np.sqrt(_dot(d[sel], d[sel]))
            x[sel] += shift[1] * amount[:, None] * across
        first = (depth == 1) & ~alt
        R.v1[idx[first]] = ids[first]
        np.maximum.at(R.depth, idx[~alt], depth[~alt])
        np.add.at(R.sig, idx[~alt], ((ids + 2) * (1 + 64 * depth + 4096 * branch.astype(np.int64)))[~alt])
        # normals: the axis normal or (x - p) / r (:248), oriented against the ray (:445)
        gn = np.zeros((len(idx), 3))
        ax = S.axis[ids]
        rect = ax >= 0
        gn[rect, ax[rect]] = 1.0
        gn[~rect] = (x[~rect] - S.centre[ids[~rect]]) / S.radius[ids[~rect], None]
        nl = np.where((_dot(gn, d) < 0)[:, None], gn, -gn)
        e, f, pm, refl = S.e[ids], S.c[ids].copy(), S.pmax[ids], S.refl[ids]
        # the vertex's words; vertex 1's RR / mix draws come from stream 1 (its low bytes were the jitter)
        pix, s = pix_all[idx], s_all[idx]
        r = _words(oracle, pix, s, depth.astype(np.uint32) | (branch << np.uint32(24)), p.seed)
        rl = r.copy()
        one = depth == 1
        if one.any():
            rl[one] = _words(oracle, pix[one], s[one], np.uint32(1) | np.uint32(0x80000000), p.seed)
        u_rr, u_mix = _u16(rl[:, 0], rl[:, 1]), _u16(rl[:, 2], rl[:, 3])
        # :448 and max_depth
        capped = (p.max_depth > 0) & (depth >= p.max_depth)
        rr = ~capped & ((depth > p.rr_depth) | (pm == 0))
        roul = rr & (pm > 0) & (pm < 1)
        np.minimum.at(R.margin, idx[roul & ~alt], np.abs(u_rr - pm)[roul & ~alt])
        keep = ~capped & (~rr | ((pm > 0) & ((pm >= 1) | (u_rr < pm))))
        f[rr & keep] /= pm[rr & keep, None]
        np.add.at(R.L, idx[~alt], (Tw * e)[~alt])
        np.add.at(R.alt_scatter, idx[alt], (Tw * e)[alt])
        # closed: the path ends at its first or second vertex whatever max_depth is (p = 0, :448)
        R.closed[idx[~alt & (pm == 0) & (depth <= 2)]] = True
        nxt = []

        def push(rows, o_, d_, T_, br, own_, cid=None, ct_=None, ins=None, al=None):
            k = len(rows)
            nxt.append((idx[rows], o_, d_, T_, depth[rows], br, own_,
                        np.full(k, -2) if cid is None else cid, np.zeros(k) if ct_ is None else ct_,
                        inside[rows] if ins is None else ins, alt[rows] if al is None else al))

        own_next = np.where(rect, ids, -1)
        # ---- DIFF (:457-480)
        dv = np.flatnonzero(keep & (refl == DIFF))
        if len(dv):
            if p.nee_prob >= 1.0:
                nee = np.ones(len(dv), dtype=bool)
            elif p.nee_prob <= 0.0:
                nee = np.zeros(len(dv), dtype=bool)
            else:
                q = float(np.float32(p.nee_prob))
                nee = u_mix[dv] < q
                np.minimum.at(R.margin, idx[dv], np.abs(u_mix[dv] - q))
            reach = np.zeros(len(dv), dtype=bool)
            wgt = np.ones(len(dv))
            dl = np.zeros((len(dv), 3))
            ts = np.zeros(len(dv))
            a_ = dv[nee]
            if len(a_):
                xl, zl = _light_points(p, r[a_, 0], r[a_, 1])
                lv = np.stack([xl - x[a_, 0], float(p.light_y) - x[a_, 1], zl - x[a_, 2]], axis=1)  # :367
                du = rt.unit(lv)
                sid, st, sm = S.nearest(x[a_], du, own_next[a_], shadow=True, shadow_to=p.light_id)
                np.minimum.at(R.margin, idx[a_][~alt[a_]], sm[~alt[a_]])
                got = sid == p.light_id
                if shift is not None and got.any():
                    sel = got & (depth[a_] + 1 == shift[0]) & (shift[2] == 0)
                    st = st.copy()
                    st[sel] += shift[1] * rt.t_bound(S.T, S.prims, x[a_][sel], du[sel], sid[sel], st[sel])
                with np.errstate(divide="ignore", invalid="ignore"):
                    ww = np.abs(float(p.light_area) * du[:, 1] / (st * st)) * np.abs(_dot(du, nl[a_])) / np.pi
                reach[nee] = got
                wgt[nee] = np.where(got, ww, 1.0)
                dl[nee] = du
                ts[nee] = st
            sc = _scatter(nl[dv], r[dv, 2], r[dv, 3], uniform)
            R.reach[idx[dv[reach & first[dv]]]] = True
            R.alt_e1[idx[dv[first[dv]]]] = e[dv[first[dv]]]
            R.has_alt[idx[dv[first[dv]]]] = True
            go = dv[reach]
            push(go, x[go], dl[reach], Tw[go] * f[go] * wgt[reach, None], branch[go], own_next[go],
                 cid=np.full(len(go), p.light_id), ct_=ts[reach])
            no = dv[~reach]
            push(no, x[no], sc[~reach], Tw[no] * f[no], branch[no], own_next[no])
            # the alternative of a first vertex that reaches: :468's scatter ray instead
            al = dv[reach & first[dv]]
            if len(al):
                R.alt_scatter[idx[al]] = e[al]
                push(al, x[al], sc[reach & first[dv]], Tw[al] * f[al], branch[al], own_next[al],
                     al=np.ones(len(al), dtype=bool))
        # ---- SPEC / REFR (:482-495)
        sv = np.flatnonzero(keep & (refl != DIFF))
        if len(sv):
            dd, n_, nls = d[sv], gn[sv], nl[sv]
            Tf = Tw[sv] * f[sv]
            rd = dd - n_ * (2.0 * _dot(n_, dd))[:, None]
            glass = refl[sv] == REFR
            into = _dot(n_, nls) > 0
            nnt = np.where(into, 1.0 / 1.5, 1.5)
            ddn = _dot(dd, nls)
            cos2t = 1.0 - nnt * nnt * (1.0 - ddn * ddn)
            np.minimum.at(R.margin, idx[sv[glass]], np.abs(cos2t[glass]))
            tir = glass & (cos2t < 0)
            only_refl = ~glass | tir
            g = sv[only_refl]
            push(g, x[g], rd[only_refl], Tf[only_refl], branch[g], own_next[g],
                 ins=inside[g] | (tir[only_refl] & ~into[only_refl]))
            tr = glass & ~tir
            if tr.any():
                g = sv[tr]
                sgn = np.where(into[tr], 1.0, -1.0)
                td = rt.unit(dd[tr] * nnt[tr, None]
                             - n_[tr] * (sgn * (ddn[tr] * nnt[tr] + np.sqrt(cos2t[tr])))[:, None])
                R0 = (0.5 * 0.5) / (2.5 * 2.5)
                c = 1.0 - np.where(into[tr], -ddn[tr], _dot(td, n_[tr]))
                Re = R0 + (1.0 - R0) * c ** 5
                Tr = 1.0 - Re
                P = 0.25 + 0.5 * Re
                deep = depth[g] > 2
                u = u_mix[g]
                np.minimum.at(R.margin, idx[g[deep]], np.abs(u - P)[deep])
                pick_r = deep & (u < P)
                pick_t = deep & ~(u < P)
                both = ~deep
                ins_r = inside[g] | ~into[tr]      # a reflection on the way out stays inside
                leaves = inside[g] & ~into[tr]     # a refraction on the way out after one
                for rows, dirs, wt, br, ins, lv_ in (
                        (pick_r, rd[tr], Re / P, branch[g], ins_r, None),
                        (pick_t, td, Tr / (1.0 - P), branch[g], inside[g], leaves),
                        (both, rd[tr], Re, branch[g], ins_r, None),
                        (both, td, Tr, branch[g] | (np.uint32(1) << (depth[g] - 1).astype(np.uint32)),
                         inside[g], leaves)):
                    if rows.any():
                        gg = g[rows]
                        push(gg, x[gg], dirs[rows], Tf[tr][rows] * wt[rows, None], br[rows], own_next[gg],
                             ins=ins[rows])
                        if lv_ is not None:
                            R.internal_exit[idx[gg[lv_[rows]]]] = True
        if not nxt:
            break
        (idx, o, d, Tw, depth, branch, own, car_id, car_t, inside, alt) = [
            np.concatenate([c[j] for c in nxt]) for j in range(11)]
    R.cls = np.where(R.v1 >= 0, S.refl[np.clip(R.v1, 0, None)], 0)
    R.v1_sphere = (R.v1 >= 0) & (S.kind[np.clip(R.v1, 0, None)] == rt.SPHERE)
    R.alt_scatter = np.where(R.reach[:, None], R.alt_scatter, R.L)
    R.alt_e1 = np.where(R.has_alt[:, None], R.alt_e1, R.L)
    return R


# roundings of size 2^-24 (relative to the sample's value) on the longest chain, counted from
# DESIGN.md section 3's statements. Per sample: the fixed point's product and the resolve's
# float, 2. Camera ray and per vertex: the direction's normalisation (3 products, a sum of 3, the
# rsqrt = RSQ_NR_REL ~ 2.2 roundings, the scaling) 8, the hit point's mul and add 2, the throughput's
# product 1 and the emission's fma 1: 12. A NEE weight: the shadow vector 1, its normalisation 8 (unit)
# or d.d squared 4 (free), two dot products of 3 terms 6, area dl.y 1, t t 1, the quotient
# (RCP_NR_REL ~ 1 rounding + 1), 1/pi 1, pdf brdf 1, T f w 1: 22. A REFR vertex: ddn 3, cos2t 5, its root
# 1, kk 3, tdir's 2 per component and normalisation 8, c 4, c^5 4, Re, Tr, P, the quotient 5, the
# weight 1: 36; the mirror direction 3 + 2: 5.
R_SAMPLE, R_VERTEX, R_NEE, R_REFR, R_SPEC = 2, 12, 22, 36, 5


def sample_values(oracle, prims, cam, p):
    """The truth and its bound per sample, as the 1.31 fixed point sees them.

    value = min(L / spp, 1) per channel. bound, to first order: the sum over the path's vertices k
    of the larger change of the value when vertex k is moved by + or - its t_bound along the incoming
    ray (this carries the hit-point displacement through everything after it: the light distance and
    the cosines, where dl.y is small on the ceiling and high on the walls; the sphere normal, the
    Fresnel terms and the next hits of a glass path), plus 2^-24 per fp32 rounding on the longest
    chain times the value (R_* above, with RCP_NR_REL, RSQ_NR_REL inside the counts; RSQ_NR2_REL is
    inside t_bound's sphere term; COSINE_FREE_ABS moves a scatter ray by less than the 1e-3 margin
    over any distance in these rooms, 2.5e-6 x 200, and a scatter ray's value depends on nothing but
    which prim it hits), plus 2^-31 for the truncation. Returns a Result as replay()'s with value,
    bound, alt_e1, alt_scatter scaled and clamped alike."""
    S = Scene(oracle, prims)
    R = replay(oracle, prims, cam, p, scene=S)
    inv = 1.0 / p.spp
    fix = lambda L: np.minimum(L * inv, 1.0)  # noqa: E731
    R.value = fix(R.L)
    kmax = int(R.depth.max())
    R.flip = np.zeros(len(R.value), dtype=bool)
    bound, unclamped = np.zeros_like(R.value), np.zeros_like(R.value)
    for k in range(1, kmax + 1):
        for axis in (0, 1, 2):
            dv, du = np.zeros_like(R.value), np.zeros_like(R.value)
            for sgn in (1.0, -1.0):
                Rk = replay(oracle, prims, cam, p, shift=(k, sgn, axis), scene=S, depth_cap=kmax + 2)
                dv = np.maximum(dv, np.abs(fix(Rk.L) - R.value))
                du = np.maximum(du, np.abs(Rk.L - R.L) * inv)
                # a decision that the displacement itself flips: the bound then spans both outcomes
                R.flip |= Rk.sig != R.sig
            bound += dv
            unclamped += du
    glass = any(q.refl == REFR for q in prims)
    spec = any(q.refl != DIFF for q in prims)
    per_vertex = R_VERTEX + (R_REFR if glass else 0) + (R_SPEC if spec else 0)
    nr = R_SAMPLE + R_VERTEX + R.depth * per_vertex + np.where(R.reach, R_NEE, 0)
    R.bound = bound + (nr * 2.0 ** -24)[:, None] * R.value + 2.0 ** -31
    R.bound_unclamped = unclamped + (nr * 2.0 ** -24)[:, None] * R.L * inv + 2.0 ** -31  # of L / spp
    # a sphere vertex has no self-hit (the 2e-3 epsilon skips the near root): no alternative there,
    # so a sphere sample off its truth fits neither and fails
    sph = R.v1_sphere[:, None]
    R.alt_e1 = np.where(sph, R.value, fix(R.alt_e1))
    R.alt_scatter = np.where(sph, R.value, fix(R.alt_scatter))
    return R


def pixel_sums(R, p, what="value"):
    """Per-pixel sums over the spp samples of a per-sample array: (h, w, ...)."""
    a = getattr(R, what) if isinstance(what, str) else what
    return a.reshape((p.height, p.width, p.spp) + a.shape[1:]).sum(axis=2)


# ---- the tables of tests/test_contract_shade.py and tests/test_gpu_shade.py ------------------------
A_W, A_H = 64, 48
B_W, B_H = 48, 32
DIM = 1.0 / 16  # the light's emission 12 / 16 (1, .5, .25): no sample of family A clamps
UNI = FLAG_UNIFORM_SCATTER

# Family A (direct light): id -> (scene, params, the kernel at max_depth = 2, the kernel at max_depth = 0
# or None). The second kernel is compiled for max_depth = 0 only: there the test keeps the samples whose
# path ends by itself at its second vertex (Result.closed), which no cap is needed for.
A_CASES = {
    "head-wrap-s1": ("head", dict(seed=1, spp=1), "const", "const_nee"),
    "head-uniform-s2": ("head", dict(seed=2, spp=1, light_mode=LIGHT_UNIFORM), "const", None),
    "head-wrap-spp4": ("head", dict(seed=2, spp=4), "const", None),
    "head-uniform-spp4": ("head", dict(seed=1, spp=4, light_mode=LIGHT_UNIFORM), "const", None),
    "movebox": ("movebox", dict(seed=1, spp=1), "cornell", "upbox_nee"),
    "editlight-wrap": ("editlight2", dict(seed=2, spp=1), "cornell", "uplight_nee"),
    "editlight-uniform": ("editlight2", dict(seed=1, spp=1, light_mode=LIGHT_UNIFORM), "cornell", None),
    "dropbox": ("dropbox", dict(seed=1, spp=1), "rectdiff", "rectdiff_nee"),
    "spheres32-wrap": ("spheres32", dict(seed=1, spp=1), "sphdiff_nee", None),
    "spheres32-uniform-spp4": ("spheres32", dict(seed=2, spp=4, light_mode=LIGHT_UNIFORM), "sphdiff", None),
    "head-uniform-scatter": ("head", dict(seed=1, spp=1, flags=UNI), "generic", None),
    "head-cosine-only": ("head", dict(seed=2, spp=4, nee_prob=0.0), "const", "const_cos"),
    "head-cosine-uniform-scatter": ("head", dict(seed=1, spp=4, nee_prob=0.0, flags=UNI), "generic", None),
}


def a_scene(spt, name, emission=12.0 * DIM):
    if name == "editlight2":  # another rectangle and another height
        prims = spt.edit_light(spt.cornell_scene(), x=(28, 72), z=(60, 100), y=80.0)
    else:
        prims = rt.scene(spt, name)
    out = [spt.spt_prim.from_buffer_copy(q) for q in prims]
    out[6].e[0], out[6].e[1], out[6].e[2] = emission, emission / 2, emission / 4
    return out


def a_case(spt, case, max_depth=2, emission=12.0 * DIM):
    name, kw, _, _ = A_CASES[case]
    kw = dict(dict(nee_prob=1.0), **kw)
    p = spt.default_params(width=A_W, height=A_H, max_depth=max_depth, **kw)
    cam = spt.Camera(aspect=float(np.float32(A_W) / np.float32(A_H)))
    return a_scene(spt, name, emission), cam, p


# Family B (the specular tree): every DIFF prim emits a colour of its own and is black, so a path ends
# at the first wall it meets; the mirror and glass balls as shipped.
B_SCENES = {"room": "generic", "widebox": "wide"}   # the kernel each runs
B_DEPTHS = [(2, 2), (3, 3), (4, 4), (6, 6), (0, 3)]  # (max_depth, rr_depth); the last: uncapped, RR on .999
B_CASES = [(sc, md, rr, spp, seed) for sc in B_SCENES for md, rr in B_DEPTHS for spp, seed in ((1, 1), (4, 2))]


def b_scene(spt, name):
    base = spt.cornell_specular_scene() if name == "room" else spt.smallpt_mirror_glass_scene()
    out = [spt.spt_prim.from_buffer_copy(q) for q in base]
    for i, q in enumerate(out):
        if q.refl == DIFF:
            q.c[0] = q.c[1] = q.c[2] = 0.0
            q.e[0], q.e[1], q.e[2] = (i + 1) / 10, ((3 * i) % 7 + 1) / 10, ((5 * i) % 9 + 1) / 10
    return out


def b_case(spt, name, max_depth, rr_depth, spp, seed):
    kw = dict(nee_prob=0.0) if name == "widebox" else {}  # the box has no light rectangle
    p = spt.default_params(width=B_W, height=B_H, spp=spp, seed=seed, max_depth=max_depth,
                           rr_depth=rr_depth, **kw)
    cam = spt.Camera(aspect=float(np.float32(B_W) / np.float32(B_H)))
    return b_scene(spt, name), cam, p


_TRUTHS = {}


def truth(oracle, key, prims, cam, p):
    """sample_values, computed once per table and shared by the CPU and the GPU tests."""
    if key not in _TRUTHS:
        _TRUTHS[key] = sample_values(oracle, prims, cam, p)
    return _TRUTHS[key]


def check_a(R, p, img, label):
    """Family A's conditions on an image (h, w, 3) float32 against the truth R. Returns the figures."""
    spp = p.spp
    got = img.astype(np.float64).reshape(-1, 3)
    px = lambda a: a.reshape((-1, spp) + a.shape[1:])  # noqa: E731
    value, bound = px(R.value).sum(axis=1), px(R.bound).sum(axis=1)
    resolve = lambda v: np.minimum(v, 1.0)  # noqa: E731
    bound = bound + 2.0 ** -24 * value
    keep = px(R.margin).min(axis=1) > MARGIN
    flip = px(R.flip).any(axis=1)
    err = np.abs(got - resolve(value))
    ok = (err <= bound).all(axis=1)
    # the alternatives: any one sample of the pixel stopped by its own wall (:468's scatter ray
    # taken, which its own wall stops too, or which goes on to whatever it hits)
    import itertools
    cand = (px(R.value), px(R.alt_e1), px(R.alt_scatter))
    n_alts = np.full(len(got), 99)   # the fewest samples of the pixel that took an alternative
    for combo in sorted(itertools.product((0, 1, 2), repeat=spp), key=lambda c: sum(k > 0 for k in c)):
        if not any(combo):
            continue
        v = sum(cand[k][:, s] for s, k in enumerate(combo))
        differs = np.ones(len(got), dtype=bool)
        for s, k in enumerate(combo):
            if k:
                differs &= (cand[k][:, s] != cand[0][:, s]).any(axis=1)
        m = (np.abs(got - resolve(v)) <= bound).all(axis=1) & differs
        n_alts = np.where(m & (n_alts == 99), sum(k > 0 for k in combo), n_alts)
    alt = n_alts < 99
    lit = (px(R.value) != px(R.alt_e1)).any(axis=(1, 2))      # the light contributes: alternatives differ
    n_alt = int(n_alts[keep & ~ok & alt].sum())
    neither = keep & ~ok & ~alt
    ratio = (err / bound).max(axis=1)
    rel = (err / np.maximum(resolve(value), 1e-30)).max(axis=1)
    sel = keep & ok & ~flip
    n_lit = int((px(R.value) != px(R.alt_e1)).any(axis=2)[keep].sum())  # samples, as n_alt
    fig = dict(excluded=float(np.mean(R.margin <= MARGIN)), lit=n_lit, reach=int(px(R.reach).any(axis=1).sum()),
               alt=n_alt, alt_share=n_alt / max(n_lit, 1), pixels_lost=float(np.mean(~keep)),
               flips=int((keep & flip).sum()),
               neither=int(neither.sum()), ratio=float(ratio[sel].max()),
               rel=float(rel[sel & lit].max()) if (sel & lit).any() else 0.0,
               alt_pixels=np.flatnonzero(keep & ~ok & alt), keep=keep, ok=ok, bound=bound,
               value=resolve(value), closed=px(R.closed).all(axis=1))
    print(f"{label}: {fig['excluded']:.2%} of the samples excluded ({fig['pixels_lost']:.2%} of the pixels), {fig['lit']} lit, {fig['reach']} reach, {n_alt} alternative "
          f"({fig['alt_share']:.2%} of lit), {fig['flips']} flipped by the "
          f"displacement, {fig['neither']} neither; max err / bound {fig['ratio']:.3f}, max relative error "
          f"{fig['rel']:.2e}")
    return fig


def check_b(R, p, img, label):
    """Family B's conditions: every kept pixel within its bound; the figures per material class."""
    spp = p.spp
    got = img.astype(np.float64).reshape(-1, 3)
    px = lambda a: a.reshape((-1, spp) + a.shape[1:])  # noqa: E731
    value, bound = px(R.value).sum(axis=1), px(R.bound).sum(axis=1)
    bound = bound + 2.0 ** -24 * value
    keep = px(R.margin).min(axis=1) > MARGIN
    flip = px(R.flip).any(axis=1)
    cls = px(R.cls).max(axis=1)
    err = np.abs(got - np.minimum(value, 1.0))
    ratio = (err / bound).max(axis=1)
    fig = dict(excluded=float(np.mean(R.margin <= MARGIN)), flips=int((keep & flip).sum()), bad=int((keep & (ratio > 1)).sum()),
               internal_exit=int(px(R.internal_exit).any(axis=1).sum()), n_glass=int((keep & (cls == REFR)).sum()))
    for c, nm in ((DIFF, "wall"), (SPEC, "mirror"), (REFR, "glass")):
        k = keep & (cls == c)
        fig[nm] = float(err[k].max())
        fig[nm + "_ratio"] = float(ratio[k & ~flip].max())
    print(f"{label}: {fig['excluded']:.2%} of the samples excluded, {fig['flips']} flipped, {fig['internal_exit']} pixels reflect "
          f"inside the glass and leave it; max error wall {fig['wall']:.2e} mirror {fig['mirror']:.2e} glass "
          f"{fig['glass']:.2e}; max err / bound wall {fig['wall_ratio']:.3f} mirror {fig['mirror_ratio']:.3f} "
          f"glass {fig['glass_ratio']:.3f}; {fig['bad']} beyond the bound")
    return fig

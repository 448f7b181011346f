// spt_dispatch.cpp — the host decisions of a render, with no HIP in them: validation, the scene's
// grouped geometry (build_geo), which kernel variant runs (select_variant over kKernelInfo,
// spt_variants.h) and how the launch is sized (plan_launch). Pure functions of their arguments, so
// spt_select_kernel answers without a device and tests/probe/spt_dispatch_check.cpp runs them
// under the sanitizers. spt_context.cpp launches what they return.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>

#include "spt_launch.h"

static thread_local std::string g_last_error;
void spt_set_last_error(const std::string& msg) { g_last_error = msg; }
extern "C" const char* spt_last_error(void) { return g_last_error.c_str(); }

namespace spt {

spt_status fail(spt_status s, const std::string& msg) {
  g_last_error = msg;
  return s;
}

spt_status validate(const spt_prim* prims, int32_t n, const spt_camera* cam,
                    const spt_params* p) {
  if (!prims || !cam || !p) return fail(SPT_ERR_INVALID_ARG, "null argument");
  if (n <= 0 || n > kMaxPrims) return fail(SPT_ERR_INVALID_ARG, "n_prims must be in [1, 64]");
  if (p->width <= 0 || p->height <= 0 || p->spp <= 0)
    return fail(SPT_ERR_INVALID_ARG, "width/height/spp must be positive");
  if ((uint64_t)p->width * (uint64_t)p->height > 0xFFFFFFFFull)
    return fail(SPT_ERR_INVALID_ARG, "image too large for 32-bit pixel counters");
  if (p->shard_count < 1 || p->shard_index < 0 || p->shard_index >= p->shard_count)
    return fail(SPT_ERR_INVALID_ARG, "bad shard_index/shard_count");
  if (p->tile_rows < 0 || p->chunk < 0) return fail(SPT_ERR_INVALID_ARG, "negative tile/chunk");
  if (p->flags & ~(SPT_FLAG_UNIFORM_SCATTER | SPT_FLAG_REFERENCE_LEAKS | SPT_FLAG_KERNEL_LEVEL_MASK))
    return fail(SPT_ERR_INVALID_ARG, "unknown flags");
  if (((p->flags & SPT_FLAG_KERNEL_LEVEL_MASK) >> 8) > SPT_KERNEL_LEVEL_CONST)
    return fail(SPT_ERR_INVALID_ARG, "bad kernel level");
  if (p->light_mode != SPT_LIGHT_GLIBC_WRAP && p->light_mode != SPT_LIGHT_UNIFORM)
    return fail(SPT_ERR_INVALID_ARG, "bad light_mode");
  if (p->light_mode == SPT_LIGHT_GLIBC_WRAP &&
      (p->light_dx != (float)(uint32_t)p->light_dx || p->light_dz != (float)(uint32_t)p->light_dz))
    return fail(SPT_ERR_INVALID_ARG, "GLIBC_WRAP light sampling needs integral light_dx/dz");
  for (int i = 0; i < n; ++i) {
    if (prims[i].kind < SPT_RECT_XY || prims[i].kind > SPT_SPHERE)
      return fail(SPT_ERR_INVALID_ARG, "bad primitive kind");
    // Sphere::normal (:248) is (x - p).norm(); the contract's (x - p) * (1/r) equals it only for
    // r > 0 (a negative radius would flip the geometric normal of the REFR test :485)
    if (prims[i].kind == SPT_SPHERE && !(prims[i].geom[0] > 0.0 && std::isfinite(prims[i].geom[0])))
      return fail(SPT_ERR_INVALID_ARG, "sphere radius must be positive and finite");
    if (prims[i].refl < SPT_DIFF || prims[i].refl > SPT_REFR)
      return fail(SPT_ERR_INVALID_ARG, "bad material");
  }
  // NEE (:464-472) weights shadow rays that reach prims[light_id] as light hits: that primitive
  // must exist and emit, or the image is silently wrong (e.g. the classic sphere box with the HEAD
  // light id 6, a ball).
  if (p->nee_prob > 0.0f) {
    if (p->light_id < 0 || p->light_id >= n)
      return fail(SPT_ERR_INVALID_ARG, "nee_prob > 0 needs light_id in [0, n_prims)");
    const double* e = prims[p->light_id].e;
    if (!(e[0] != 0.0 || e[1] != 0.0 || e[2] != 0.0))
      return fail(SPT_ERR_INVALID_ARG, "nee_prob > 0 but prims[light_id] emits nothing");
  }
  return SPT_OK;
}

// max(c) of a primitive's fp32 colour: the Russian-roulette survival probability (:447)
static float prim_pmax(const spt_prim& s) {
  const float cx = (float)s.c[0], cy = (float)s.c[1], cz = (float)s.c[2];
  return cx > cy && cx > cz ? cx : cy > cz ? cy : cz;
}

void to_dev(const spt_prim* s, int n, DevPrim* out) {
  for (int i = 0; i < n; ++i) {
    DevPrim P;
    std::memset(&P, 0, sizeof P);
    P.kind = s[i].kind;
    if (s[i].kind == SPT_SPHERE) {
      const float r = (float)s[i].geom[0];
      P.w1 = (float)s[i].geom[1]; P.w2 = (float)s[i].geom[2]; P.w3 = (float)s[i].geom[3];
      P.w4 = r * r;
      P.w5 = 1.0f / r;  // the normal as (x - p) * (1/r) (contract, oracle c_path)
    } else {
      P.w1 = plane_k(s[i].geom[4]);  // contract plane coordinate (spt_cornell.h)
      P.w2 = (float)s[i].geom[0]; P.w3 = (float)s[i].geom[1];
      P.w4 = (float)s[i].geom[2]; P.w5 = (float)s[i].geom[3];
    }
    P.ex = (float)s[i].e[0]; P.ey = (float)s[i].e[1]; P.ez = (float)s[i].e[2];
    P.cx = (float)s[i].c[0]; P.cy = (float)s[i].c[1]; P.cz = (float)s[i].c[2];
    P.pmax = prim_pmax(s[i]);
    P.ip = 1.0f / P.pmax;  // IEEE single division, as the device's 1.0f / p
    // u * 2^-16 < p (u < 2^16 an integer, p * 2^16 exact) <=> u < ceil(p * 2^16): the RR draw as
    // one integer compare instead of a conversion, a scale and a float compare (same decision)
    P.rr_t = P.pmax == 0.0f ? INT32_MIN
             : !(P.pmax > 0.0f) ? 0
             : P.pmax >= 1.0f   ? 65536
                                : (int32_t)std::ceil((double)P.pmax * 65536.0);
    P.refl = s[i].refl;
    out[i] = P;
  }
}

// Rect bounds [lo, hi] as |a - mid| <= half (contract; oracle c_rect_mid).
static void rect_mid(double lo, double hi, float* mid, float* half) {
  *mid = (float)((lo + hi) * 0.5);
  *half = hi >= lo ? (float)((hi - lo) * 0.5) : -1.0f;
}

// Grouped geometry; *light_pos = position of prim `light` in rect[] / sph[] (-1 if absent).
void build_geo(const spt_prim* s, int n, SceneGeo* g, int light, int* light_pos) {
  std::memset(g, 0, sizeof *g);
  *light_pos = -1;
  int r = 0;
  const int kinds[3] = {SPT_RECT_XY, SPT_RECT_XZ, SPT_RECT_YZ};
  int* counts[3] = {&g->n_xy, &g->n_xz, &g->n_yz};
  for (int k = 0; k < 3; ++k) {
    for (int i = 0; i < n; ++i) {
      if (s[i].kind != kinds[k]) continue;
      GeoRect& R = g->rect[r++];
      R.k = plane_k(s[i].geom[4]);
      rect_mid(s[i].geom[0], s[i].geom[1], &R.ma, &R.ha);
      rect_mid(s[i].geom[2], s[i].geom[3], &R.mb, &R.hb);
      R.idx = i;
      if (i == light) *light_pos = r - 1;
      ++*counts[k];
    }
  }
  // Rect tests (oracle c_build_tests): inside each kind group, in order, a rectangle pairs with the
  // first later unpaired one of bit-identical bounds on a different plane; the light never pairs.
  {
    bool used[kMaxPrims] = {};
    const int grp[4] = {0, g->n_xy, g->n_xy + g->n_xz, g->n_xy + g->n_xz + g->n_yz};
    int* tcounts[3] = {&g->n_txy, &g->n_txz, &g->n_tyz};
    int nt = 0;
    auto bits = [](float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; };
    for (int k = 0; k < 3; ++k) {
      for (int i = grp[k]; i < grp[k + 1]; ++i) {
        if (used[i]) continue;
        used[i] = true;
        const GeoRect& A = g->rect[i];
        GeoTest& T = g->test[nt++];
        T = GeoTest{A.k, A.k, A.ma, A.ha, A.mb, A.hb, i, i};
        ++*tcounts[k];
        if (i == *light_pos) continue;
        for (int j = i + 1; j < grp[k + 1]; ++j) {
          const GeoRect& B = g->rect[j];
          if (used[j] || j == *light_pos || bits(A.ma) != bits(B.ma) || bits(A.ha) != bits(B.ha) ||
              bits(A.mb) != bits(B.mb) || bits(A.hb) != bits(B.hb) || bits(A.k) == bits(B.k) ||
              !(A.k == A.k) || !(B.k == B.k))
            continue;
          used[j] = true;
          if (A.k < B.k) { T.k1 = B.k; T.pos1 = j; }
          else { T.k0 = B.k; T.pos0 = j; T.k1 = A.k; T.pos1 = i; }
          break;
        }
      }
    }
  }
  // Contract v5's room (oracle c_find_room): the first XY, XZ, YZ pair tests (test order) whose
  // planes are exactly -- in the caller's doubles -- the other pairs' in-plane bounds (each pair's
  // bounds read from its k0 member). Its tests move behind the per-kind lists (the nearest hit is a
  // minimum of keys, so test order cannot matter).
  {
    const int nt = g->n_txy + g->n_txz + g->n_tyz;
    auto member = [&](int pos) -> const spt_prim& { return s[g->rect[pos].idx]; };
    auto same_range = [](double k1, double k2, double b1, double b2) {
      return std::min(k1, k2) == b1 && std::max(k1, k2) == b2;
    };
    int room[3] = {-1, -1, -1};
    for (int a = 0; a < g->n_txy && room[0] < 0; ++a) {
      const GeoTest& A = g->test[a];
      if (A.pos0 == A.pos1) continue;
      for (int b = g->n_txy; b < g->n_txy + g->n_txz && room[0] < 0; ++b) {
        const GeoTest& B = g->test[b];
        if (B.pos0 == B.pos1) continue;
        for (int c = g->n_txy + g->n_txz; c < nt; ++c) {
          const GeoTest& D = g->test[c];
          if (D.pos0 == D.pos1) continue;
          const double* ga = member(A.pos0).geom, *gb = member(B.pos0).geom, *gd = member(D.pos0).geom;
          const double zA = ga[4], zB = member(A.pos1).geom[4], yA = gb[4], yB = member(B.pos1).geom[4];
          const double xA = gd[4], xB = member(D.pos1).geom[4];
          if (!same_range(xA, xB, ga[0], ga[1]) || !same_range(xA, xB, gb[0], gb[1]) ||
              !same_range(yA, yB, ga[2], ga[3]) || !same_range(yA, yB, gd[0], gd[1]) ||
              !same_range(zA, zB, gb[2], gb[3]) || !same_range(zA, zB, gd[2], gd[3]))
            continue;
          room[0] = a; room[1] = b; room[2] = c;
          break;
        }
      }
    }
    g->has_room = room[0] >= 0;
    if (g->has_room) {
      const GeoTest A = g->test[room[0]], B = g->test[room[1]], D = g->test[room[2]];
      GeoTest rest[kMaxPrims];
      int n = 0;
      for (int i = 0; i < nt; ++i)
        if (i != room[0] && i != room[1] && i != room[2]) rest[n++] = g->test[i];
      for (int i = 0; i < n; ++i) g->test[i] = rest[i];
      g->test[n] = A; g->test[n + 1] = B; g->test[n + 2] = D;
      --g->n_txy; --g->n_txz; --g->n_tyz;
    }
  }
  // Contract v6's boxes (oracle c_find_boxes): an XY pair, a YZ pair and an XZ top (not the light)
  // closing a box on the room's floor, inside the floor's bounds, in the caller's doubles; searched
  // in test order. Their tests move behind the room's, three per box (XY pair, YZ pair, top).
  if (g->has_room) {
    const int nt = g->n_txy + g->n_txz + g->n_tyz;
    auto member = [&](int pos) -> const spt_prim& { return s[g->rect[pos].idx]; };
    auto same_range = [](double k1, double k2, double b1, double b2) {
      return std::min(k1, k2) == b1 && std::max(k1, k2) == b2;
    };
    const GeoTest& F = g->test[nt + 1];
    const double floor_k = std::min(member(F.pos0).geom[4], member(F.pos1).geom[4]);
    const double* gf = member(F.pos0).geom;
    bool used[kMaxPrims] = {};
    int box[kMaxPrims / 5][3], nb = 0;
    for (int a = 0; a < g->n_txy && nb < kMaxPrims / 5; ++a) {  // (5 rects a box: <= 12 of them)
      const GeoTest& A = g->test[a];
      if (A.pos0 == A.pos1 || used[a]) continue;
      for (int b = g->n_txy + g->n_txz; b < nt && !used[a]; ++b) {
        const GeoTest& D = g->test[b];
        if (D.pos0 == D.pos1 || used[b]) continue;
        for (int c = g->n_txy; c < g->n_txy + g->n_txz; ++c) {
          const GeoTest& T = g->test[c];
          if (T.pos0 != T.pos1 || T.pos0 == *light_pos || used[c]) continue;
          const double *ga = member(A.pos0).geom, *gd = member(D.pos0).geom, *gt = member(T.pos0).geom;
          const double xA = gd[4], xB = member(D.pos1).geom[4], zA = ga[4], zB = member(A.pos1).geom[4];
          if (!same_range(xA, xB, ga[0], ga[1]) || !same_range(xA, xB, gt[0], gt[1]) ||
              !same_range(zA, zB, gd[2], gd[3]) || !same_range(zA, zB, gt[2], gt[3]) ||
              !same_range(floor_k, gt[4], ga[2], ga[3]) || !same_range(floor_k, gt[4], gd[0], gd[1]) ||
              !(gt[4] > floor_k))
            continue;
          if (!(gf[0] <= ga[0] && ga[1] <= gf[1] && gf[2] <= gd[2] && gd[3] <= gf[3])) continue;
          used[a] = used[b] = used[c] = true;
          box[nb][0] = a; box[nb][1] = b; box[nb][2] = c;
          ++nb;
          break;
        }
      }
    }
    if (nb > 0) {
      GeoTest rest[kMaxPrims];
      int n = 0, kind_n[3] = {0, 0, 0};
      for (int i = 0; i < nt; ++i) {
        if (used[i]) continue;
        rest[n++] = g->test[i];
        ++kind_n[i < g->n_txy ? 0 : (i < g->n_txy + g->n_txz ? 1 : 2)];
      }
      for (int r = 0; r < 3; ++r) rest[n + r] = g->test[nt + r];  // the room
      for (int b = 0; b < nb; ++b)
        for (int r = 0; r < 3; ++r) rest[n + 3 + 3 * b + r] = g->test[box[b][r]];
      for (int i = 0; i < n + 3 + 3 * nb; ++i) g->test[i] = rest[i];
      g->n_txy = kind_n[0]; g->n_txz = kind_n[1]; g->n_tyz = kind_n[2];
      g->n_box = nb;
    }
  }
  // Spheres in index order, the narrow (fp32) ones first, then the wide (fp64) ones (oracle
  // c_intersect): the kernel's fp32 loop carries no per-sphere precision test.
  for (int pass = 0; pass < 2; ++pass)
  for (int i = 0; i < n; ++i) {
    if (s[i].kind != SPT_SPHERE) continue;
    if ((s[i].geom[0] >= SPT_WIDE_SPHERE_RADIUS) != (pass == 1)) continue;
    g->n_sph_wide += pass;
    GeoSph& S = g->sph[g->n_sph++];
    const float rad = (float)s[i].geom[0];
    S.px = (float)s[i].geom[1]; S.py = (float)s[i].geom[2]; S.pz = (float)s[i].geom[3];
    S.rad2 = rad * rad;
    S.idx = i;
    S.wide = s[i].geom[0] >= SPT_WIDE_SPHERE_RADIUS ? 1 : 0;
    GeoSphD& D = g->sphd[g->n_sph - 1];
    D.px = s[i].geom[1]; D.py = s[i].geom[2]; D.pz = s[i].geom[3];
    D.rad2 = s[i].geom[0] * s[i].geom[0];
    if (i == light) *light_pos = g->n_sph - 1;
  }
}

// Contract v6 (oracle c_find_leak_end): a leaked path ends at its first miss when the scene has a
// room, the miss vertex (the origin, :373-374) lies strictly outside the room's box, prim 0 does
// not emit and every emitter lies strictly inside the box -- compared on the caller's doubles.
static int leak_end_of(const spt_prim* s, int n, const SceneGeo& g) {
  if (!g.has_room) return 0;
  const int nt = g.n_txy + g.n_txz + g.n_tyz;
  double lo[3], hi[3];
  for (int a = 0; a < 3; ++a) {  // room tests: XY pair (planes z), XZ (y), YZ (x)
    const GeoTest& T = g.test[nt + a];
    const double k0 = s[g.rect[T.pos0].idx].geom[4], k1 = s[g.rect[T.pos1].idx].geom[4];
    const int ax = a == 0 ? 2 : (a == 1 ? 1 : 0);
    lo[ax] = std::min(k0, k1);
    hi[ax] = std::max(k0, k1);
  }
  if (!(0.0 < lo[0] || 0.0 > hi[0] || 0.0 < lo[1] || 0.0 > hi[1] || 0.0 < lo[2] || 0.0 > hi[2])) return 0;
  if (s[0].e[0] != 0.0 || s[0].e[1] != 0.0 || s[0].e[2] != 0.0) return 0;
  for (int i = 0; i < n; ++i) {
    const double* gm = s[i].geom;
    if (s[i].e[0] == 0.0 && s[i].e[1] == 0.0 && s[i].e[2] == 0.0) continue;
    if (s[i].kind == SPT_SPHERE) {
      for (int a = 0; a < 3; ++a)
        if (!(gm[1 + a] - gm[0] > lo[a] && gm[1 + a] + gm[0] < hi[a])) return 0;
      continue;
    }
    const int pa = s[i].kind == SPT_RECT_XY ? 2 : (s[i].kind == SPT_RECT_XZ ? 1 : 0);
    const int ua = s[i].kind == SPT_RECT_YZ ? 1 : 0, va = s[i].kind == SPT_RECT_XY ? 1 : 2;
    if (!(gm[4] > lo[pa] && gm[4] < hi[pa] && gm[0] >= lo[ua] && gm[1] <= hi[ua] && gm[2] >= lo[va] &&
          gm[3] <= hi[va]))
      return 0;
  }
  return 1;
}

// Multiply-shift reciprocal of d for 31-bit numerators: l = ceil(log2 d), m = floor(2^(31+l)/d) + 1
// (< 2^32), n / d = (n * m) >> (31 + l) exactly for all n < 2^31 (Granlund & Montgomery 1994).
static void magic31(uint32_t d, uint32_t* m, uint32_t* sh) {
  uint32_t l = 0;
  while ((1ull << l) < d) ++l;
  *m = (uint32_t)(((unsigned __int128)1 << (31 + l)) / d + 1);
  *sh = 31 + l;
}

// ---- How much of a scene is the compile-time HEAD scene (spt_cornell.h).
// rect[pos] is HEAD's rectangle at that grouped position: the same primitive, the same fp32 bits.
static bool head_rect(const SceneGeo& g, int pos) {
  const GeoRect& R = g.rect[pos];
  const CRect& H = kCornellRects[pos];
  const float a[5] = {R.k, R.ma, R.ha, R.mb, R.hb}, b[5] = {H.k, H.ma, H.ha, H.mb, H.hb};
  return std::memcmp(a, b, sizeof a) == 0 && R.idx == H.idx;
}
// HEAD's topology (TopoCornell): 6 XY, 5 XZ, 6 YZ rects and no sphere, the light at grouped position
// 8, a room, two boxes, and the light's as the one test besides them. The three matches below are
// asked of such scenes only.
static bool head_topology(const SceneGeo& g, int light_pos) {
  return g.n_xy == kCornellNXY && g.n_xz == kCornellNXZ && g.n_yz == kCornellNYZ && g.n_sph == 0 &&
         light_pos == kCornellLightPos && g.n_txy == 0 && g.n_txz == 1 && g.n_tyz == 0 && g.has_room &&
         g.n_box == kCornellBoxes.n;
}
// The room is the reference's (:288-293): its three pair tests at HEAD's grouped positions with
// HEAD's fp32 geometry (materials may differ). The boxes-only-uploaded kernels (TopoCornellUpBox)
// take the room as literals and everything else from LDS.
static bool head_room_match(const SceneGeo& g) {
  const int nt = g.n_txy + g.n_txz + g.n_tyz;
  for (int r = 0; r < 3; ++r) {
    const CTest& C = kCornellTests.t[kCornellRoom[r]];
    if (g.test[nt + r].pos0 != C.pos0 || g.test[nt + r].pos1 != C.pos1) return false;
    if (!head_rect(g, C.pos0) || !head_rect(g, C.pos1)) return false;
  }
  return true;
}
// The light is the reference's (:294): the boxes-only-uploaded kernels keep it literal, the
// UPLIGHT ones read it from the uploaded scene.
static bool head_light_match(const SceneGeo& g) { return head_rect(g, kCornellLightPos); }
// The grouped geometry equals the compile-time HEAD scene bit for bit: the room's and the boxes'
// tests (behind the per-kind lists) at HEAD's positions, every rectangle HEAD's.
static bool head_literal_match(const SceneGeo& g) {
  const int nt = g.n_txy + g.n_txz + g.n_tyz;
  for (int r = 0; r < 3; ++r) {
    const CTest& C = kCornellTests.t[kCornellRoom[r]];
    if (g.test[nt + r].pos0 != C.pos0 || g.test[nt + r].pos1 != C.pos1) return false;
  }
  for (int b = 0; b < kCornellBoxes.n; ++b)
    for (int r = 0; r < 3; ++r) {
      const CTest& C = kCornellTests.t[kCornellBoxes.t[b][r]];
      const GeoTest& T = g.test[nt + 3 + 3 * b + r];
      if (T.pos0 != C.pos0 || T.pos1 != C.pos1) return false;
    }
  for (int i = 0; i < kCornellNXY + kCornellNXZ + kCornellNYZ; ++i)
    if (!head_rect(g, i)) return false;
  return true;
}


// The early resolve's clauses for a HEAD-topology scene with the reference's estimator (oracle
// c_find_early_clauses, which the proof tests check claim by claim): the room's box with y below
// the light plane (early_room_ok_k), the light's rectangle >= 1 inside the side walls and >= 1 above
// the floor, its plane <= 81.5 (0.1 below the reference's sample plane :367) and >= 0.05 below the
// ceiling, the room < 1000 across with X0, Y0, Z0 >= 0; per box a top >= 0.5 below the light plane
// and the clause its position allows against the reference's wrapped samples (x in [31, 33), z in
// [62, 64)). on = false, or a condition failing: no clause (+inf / -inf, nothing resolved early).
static void early_geo_setup(const SceneGeo& g, int light_pos, bool on, KParams* K) {
  for (int b = 0; b < 2; ++b) {
    K->eb_top[b] = INFINITY; K->eb_sgn[b] = 1.0f; K->eb_bnd[b] = -INFINITY; K->eb_z[b] = 0;
  }
  for (int a = 0; a < 3; ++a) K->er_lo[a] = K->er_span[a] = 0;
  bool ok = on && g.has_room && g.n_box == 2 && light_pos >= 0 && light_pos < g.n_xy + g.n_xz + g.n_yz &&
            light_pos >= g.n_xy && light_pos < g.n_xy + g.n_xz;  // an XZ light
  if (!ok) return;
  const int nt = g.n_txy + g.n_txz + g.n_tyz;
  float lo[3], hi[3];
  for (int a = 0; a < 3; ++a) {  // room tests: XY pair (planes z), XZ (y), YZ (x)
    const GeoTest& R = g.test[nt + a];
    const int ax = a == 0 ? 2 : (a == 1 ? 1 : 0);
    lo[ax] = std::min(R.k0, R.k1);
    hi[ax] = std::max(R.k0, R.k1);
    ok = ok && lo[ax] >= 0.0f && hi[ax] - lo[ax] <= 1000.0f;
    // a wall at -0.0 passes lo >= 0 with the bits 0x80000000: the span below would wrap and the
    // uint compare hold for every negative coordinate. +0.0 instead: a vertex at exactly -0.0 then
    // fails the compare and is traced, which is exact
    if (lo[ax] == 0.0f) lo[ax] = 0.0f;
  }
  const GeoRect& L = g.rect[light_pos];
  const float yl = L.k;
  ok = ok && L.ha >= 0.0f && L.hb >= 0.0f && L.ma - L.ha >= lo[0] + 1.0f && L.ma + L.ha <= hi[0] - 1.0f &&
       L.mb - L.hb >= lo[2] + 1.0f && L.mb + L.hb <= hi[2] - 1.0f && yl >= lo[1] + 1.0f && yl <= 81.5f &&
       hi[1] >= yl + 0.05f;
  for (int b = 0; ok && b < 2; ++b) {
    const GeoTest &XY = g.test[nt + 3 + 3 * b], &YZ = g.test[nt + 4 + 3 * b], &T = g.test[nt + 5 + 3 * b];
    const float z0 = std::min(XY.k0, XY.k1), z1 = std::max(XY.k0, XY.k1);
    const float x0 = std::min(YZ.k0, YZ.k1), x1 = std::max(YZ.k0, YZ.k1);
    // the box top at least 0.5 below the light plane (a top just under the plane left
    // the box's y-slab exit within rounding of the light crossing)
    if (!(T.k0 <= yl - 0.5f)) { ok = false; break; }
    K->eb_top[b] = T.k0;
    if (x0 >= 33.0f) { K->eb_sgn[b] = 1.0f; K->eb_bnd[b] = x0; K->eb_z[b] = 0; }
    else if (x1 <= 31.0f) { K->eb_sgn[b] = -1.0f; K->eb_bnd[b] = -x1; K->eb_z[b] = 0; }
    else if (z0 >= 64.0f) { K->eb_sgn[b] = 1.0f; K->eb_bnd[b] = z0; K->eb_z[b] = 1; }
    else if (z1 <= 62.0f) { K->eb_sgn[b] = -1.0f; K->eb_bnd[b] = -z1; K->eb_z[b] = 1; }
  }
  if (!ok) {
    for (int b = 0; b < 2; ++b) { K->eb_top[b] = INFINITY; K->eb_sgn[b] = 1.0f; K->eb_bnd[b] = -INFINITY; }
    return;
  }
  for (int a = 0; a < 3; ++a) {
    const float top = a == 1 ? std::nextafter(yl, 0.0f) : hi[a];  // y < y_L
    uint32_t blo, btop;
    std::memcpy(&blo, &lo[a], 4);
    std::memcpy(&btop, &top, 4);
    K->er_lo[a] = blo;
    K->er_span[a] = btop - blo;
  }
}

// The sphere NEE kernels' early-resolve threshold (early_room_proven): the HEAD room (rect[]
// :287-294, light at index 6) as prims 0..6, nothing else but narrow spheres, and a threshold above
// every sphere's top; otherwise +inf (off: every shadow ray is traced).
static float early_sphere_y0(const spt_prim* prims, int n_prims, const SceneGeo& g) {
  if (n_prims <= 7 || g.n_sph_wide != 0) return INFINITY;
  spt_prim head[17];
  int32_t nh = 0;
  bool ok = spt_scene_cornell(head, 17, &nh) == SPT_OK;
  for (int i = 0; ok && i < 7; ++i) ok = std::memcmp(&prims[i], &head[i], sizeof(spt_prim)) == 0;
  double top = -INFINITY;
  for (int i = 7; ok && i < n_prims; ++i) {
    const double* g = prims[i].geom;
    ok = prims[i].kind == SPT_SPHERE && std::isfinite(g[0]) && std::isfinite(g[1]) &&
         std::isfinite(g[2]) && std::isfinite(g[3]);
    top = std::max(top, g[2] + std::fabs(g[0]));
    // the fp32 rounding argument of early_room_proven holds for |op| < 200 (and r < 200): every
    // sphere centre within 190 of every room corner, so no vertex in the room is farther away
    for (int c = 0; ok && c < 8; ++c) {
      const double cx = (c & 1) ? 99.0 : 1.0, cy = (c & 2) ? 81.6 : 0.0, cz = (c & 4) ? 170.0 : 0.0;
      ok = std::sqrt((g[1] - cx) * (g[1] - cx) + (g[2] - cy) * (g[2] - cy) +
                     (g[3] - cz) * (g[3] - cz)) < 190.0 && std::fabs(g[0]) < 190.0;
    }
  }
  if (!ok || !(top + 1.0 < 81.0)) return INFINITY;
  float y0 = (float)(top + 1.0);
  if ((double)y0 < top + 1.0) y0 = std::nextafter(y0, INFINITY);
  return y0;
}

// ---- The kernel choice: the first variant of kPreference whose scene class the scene is in, whose
// estimator constants the params satisfy and whose level is within SPT_FLAG_KERNEL_LEVEL's cap.
struct SceneFacts {
  bool in_class[kSceneClassCount];  // the scene classes (spt_variants.h) the scene belongs to
  bool xz_light;                    // the light is an XZ rectangle
};
struct EstimatorFacts {
  float nee_prob;
  int light_mode, max_depth, rr_depth;
  bool light_black;  // the light's colour is 0
  bool lref;         // the reference's light sampling and RR constants (the kRef* of spt_variants.h)
  bool cam_axis;     // the camera is axis-aligned (Cfg CAMAX 1)
  bool cam_fin;      // every camera term is finite
  int leak_end;      // contract v6's leak-end rule applies (leak_end_of) and is not switched off
};

// Most specialised first. Inside a scene class: the leak-end form before the reference-leaks form,
// the axis camera before any camera (a scene and params that satisfy a row satisfy no earlier row
// of another form), then the class's run-time kernel, which always matches at its level. The HEAD
// classes nest (literal < room and light < room < topology < rect-only < generic), so a scene falls
// from one group to the next as the level cap or the estimator rules rows out.
static const int kPreference[KV_COUNT] = {
    KV_CONST_NEE,   KV_CONST_NEE_REF,  KV_CONST_COS,     KV_CONST_COS_REF,    KV_CONST_NEE_CAM,
    KV_CONST_COS_CAM, KV_CONST,
    KV_UPBOX_NEE,   KV_UPBOX_COS,      KV_UPBOX_NEE_CAM, KV_UPBOX_COS_CAM,
    KV_UPLIGHT_NEE, KV_UPLIGHT_COS,    KV_UPLIGHT_NEE_CAM, KV_UPLIGHT_COS_CAM,
    KV_CORNELL_NEE, KV_CORNELL_COS,    KV_CORNELL,
    KV_RECTDIFF_NEE, KV_RECTDIFF_COS,  KV_RECTDIFF,
    KV_SPHDIFF_NEE, KV_SPHDIFF_NEE_REF, KV_SPHDIFF,
    KV_WIDE,        KV_GENERIC};

// Do the params satisfy what the variant's Cfg constants compile in? Read from the constants
// themselves, so the host's proof and the kernel's assumption cannot drift (-1: run time, anything).
static bool estimator_ok(const KernelInfo& v, const EstimatorFacts& e) {
  if (v.nee == 1 && !(e.nee_prob >= 1.0f)) return false;
  if (v.nee == 0 && !(e.nee_prob <= 0.0f)) return false;
  // LMODE is the light sampling of NEE: the cosine kernels (NEE 0) never look at light_mode, so
  // theirs is not a condition
  if (v.nee != 0 && v.lmode >= 0 && e.light_mode != v.lmode) return false;
  if (v.black == 1 && !e.light_black) return false;
  if (v.maxd0 == 1 && e.max_depth != 0) return false;
  if (v.nos1 == 1 && !(e.rr_depth >= 1 && v.nee >= 0)) return false;  // nee_prob 0 or 1: NEE above
  if (v.camax == 1 && !e.cam_axis) return false;
  // CAMAX 2 is any finite camera. The _CAM forms exist for the leak-end rule only (their LEAK is 1):
  // a tilted camera with reference leaks runs the class's run-time kernel
  if (v.camax == 2 && !e.cam_fin) return false;
  if (v.lref == 1 && !e.lref) return false;
  if (v.leak >= 0 && e.leak_end != v.leak) return false;
  return true;
}

// The kernel variant of a render, a pure host decision (no device, no context: spt_select_kernel
// answers it for any validated scene, spt_render_window launches what it returns). g, light_pos: the
// scene's grouped geometry (build_geo). Also sets what the variant runs under in *K: the fp32
// camera, light_black, leak_end, and -- from the chosen variant's early-resolve kind -- the sphere
// kernels' early_y0, the uploaded-geometry kernels' clauses (early_geo_setup) and ul_ybits.
int select_variant(const spt_prim* prims, int n_prims, const spt_camera* cam_in, const spt_params* p,
                   const SceneGeo& g, int light_pos, KParams* Kp) {
  KParams& K = *Kp;
  float* cam = K.cam;  // the kernel's fp32 camera
  for (int i = 0; i < 3; ++i) {
    cam[i] = (float)cam_in->origin[i];
    cam[3 + i] = (float)cam_in->lower_left_corner[i];
    cam[6 + i] = (float)cam_in->horizontal[i];
    cam[9 + i] = (float)cam_in->vertical[i];
  }
  // The scene. The specialisations are all-DIFF, cosine-scatter scenes; anything else (SPEC/REFR, the
  // uniform hemisphere) runs the generic kernel, and only the wide kernel has the fp64 sphere loop.
  bool all_diff = true;
  for (int i = 0; i < n_prims; ++i) all_diff = all_diff && prims[i].refl == SPT_DIFF;
  const bool wide = g.n_sph_wide > 0;
  const bool diff = !wide && all_diff && !(p->flags & SPT_FLAG_UNIFORM_SCATTER);
  SceneFacts s{};
  s.in_class[kSceneWide] = wide;
  s.in_class[kSceneGeneric] = !wide;
  s.in_class[kSceneSphDiff] = diff && g.n_sph > 0;
  s.in_class[kSceneRectDiff] = diff && g.n_sph == 0;
  s.in_class[kSceneHeadTopo] = diff && head_topology(g, light_pos);
  s.in_class[kSceneHeadRoom] = s.in_class[kSceneHeadTopo] && head_room_match(g);
  s.in_class[kSceneHeadRoomLight] = s.in_class[kSceneHeadRoom] && head_light_match(g);
  s.in_class[kSceneHeadLiteral] = s.in_class[kSceneHeadTopo] && head_literal_match(g);
  s.xz_light = light_pos >= 0 && prims[p->light_id].kind == SPT_RECT_XZ;
  // The params.
  EstimatorFacts e{};
  e.nee_prob = p->nee_prob;
  e.light_mode = p->light_mode;
  e.max_depth = p->max_depth;
  e.rr_depth = p->rr_depth;
  e.light_black = light_pos >= 0 && prim_pmax(prims[p->light_id]) == 0.0f;
  e.lref = p->rr_depth == kRefRrDepth && p->light_id == kRefLightId && p->light_x0 == kRefLx0 &&
           p->light_dx == (float)kRefLdxi && p->light_z0 == kRefLz0 && p->light_dz == (float)kRefLdzi &&
           p->light_y == kRefLy && p->light_area == kRefLarea;
  e.cam_fin = true;
  for (int i = 0; i < 12; ++i) e.cam_fin = e.cam_fin && std::isfinite(cam[i]);
  // axis-aligned camera (Cfg CAMAX 1): horizontal.y/z and vertical.x/z zero, origin nonzero (the
  // contract-v5 terms L = llc - origin and Au_x, Av_y nonzero: the zero products then vanish
  // exactly, see the kernel's camera ray)
  e.cam_axis = e.cam_fin && cam[7] == 0.0f && cam[8] == 0.0f && cam[9] == 0.0f && cam[11] == 0.0f &&
               cam[6] * (1.0f / (float)p->width) != 0.0f && cam[10] * (1.0f / (float)p->height) != 0.0f;
  for (int c = 0; c < 3; ++c) e.cam_axis = e.cam_axis && (cam[3 + c] - cam[c]) != 0.0f;
  e.leak_end = (p->flags & SPT_FLAG_REFERENCE_LEAKS) ? 0 : leak_end_of(prims, n_prims, g);
  // spt_params.flags SPT_FLAG_KERNEL_LEVEL (A/B and tests; never changes results): cap the
  // specialisation level. 0 = auto (the most specialised kernel the host can prove).
  const uint32_t klevel = (p->flags & SPT_FLAG_KERNEL_LEVEL_MASK) >> 8;
  const int cap = klevel == SPT_KERNEL_LEVEL_GENERIC   ? kLevelGeneric
                  : klevel == SPT_KERNEL_LEVEL_CORNELL ? kLevelCornell
                  : klevel == SPT_KERNEL_LEVEL_CONST   ? kLevelConst
                                                       : kLevelAuto;
  int kv = KV_COUNT;
  for (int i = 0; i < KV_COUNT && kv == KV_COUNT; ++i) {
    const KernelInfo& v = kKernelInfo[kPreference[i]];
    // (the sphere kernels' early resolve tests the uploaded light as an XZ rectangle)
    if (s.in_class[v.scene] && v.level <= cap && estimator_ok(v, e) &&
        (v.early != kEarlySphere || s.xz_light))
      kv = kPreference[i];
  }
  // (never KV_COUNT: every scene is wide or generic, and those two rows ask for nothing else)

  K.light_black = e.light_black ? 1 : 0;
  K.leak_end = e.leak_end;
  const EarlyKind early = kKernelInfo[kv].early;
  K.early_y0 = early == kEarlySphere ? early_sphere_y0(prims, n_prims, g) : INFINITY;
  // The uploaded-geometry HEAD-topology NEE kernels' early resolve (early_geo_proven): the room,
  // the light and two boxes with the margins early_geo_setup checks, the clauses it picks (oracle
  // c_find_early_clauses). Anything else: no clause, nothing resolved early.
  early_geo_setup(g, light_pos, early == kEarlyClauses, &K);
  // (read only by the UPLIGHT NEE kernels, whose box clauses early_geo_setup leaves unsatisfiable
  // unless the light plane lies >= 1 above the HEAD floor at +0: y_L >= 1, no sign bit)
  const float yl = early == kEarlyClauses ? g.rect[light_pos].k : 0.0f;
  std::memcpy(&K.ul_ybits, &yl, 4);
  return kv;
}

// Does the variant resolve shadow rays without a trace under these parameters? The literal HEAD NEE
// kernels always (early_nee_proven), the sphere NEE kernels with a finite threshold, the kernels
// with uploaded boxes when early_geo_setup found the scene inside its margins (a clause is set).
static int early_resolve_of(int kv, const KParams& K) {
  switch (kKernelInfo[kv].early) {
    case kEarlyLiteral: return 1;
    case kEarlySphere: return std::isfinite(K.early_y0) ? 1 : 0;
    case kEarlyClauses: return (K.er_span[0] | K.er_span[1] | K.er_span[2]) != 0 ? 1 : 0;
    case kEarlyNone: break;
  }
  return 0;
}

// ---- Launch sizing (spt_launch.h).
spt_status plan_launch(int n_cu, int variant_bpc, int kv, const spt_params* p, int32_t s_count,
                       int n_local_pix, KParams* Kp, LaunchPlan* plan) {
  KParams& K = *Kp;
  K.n_local_pix = n_local_pix;
  K.tile_rows = tile_rows_of(p); K.shard_index = p->shard_index; K.shard_count = p->shard_count;
  // Unit size: SPT_UNITS_PER_LANE (8) units per resident lane (C3: 96 samples); never changes
  // results (integer accumulation). Round 1 chose 16 (25.0 ms vs 26.0 ms at 8 units/lane, before
  // in-wave stealing); re-measured in round 4 with stealing, unit slots and two frames in flight
  // (profiles/r04_ab.txt session 6, 3 rounds): bench value 35.7 / 36.1 / 36.3 / 36.4 / 36.5
  // Gsamples/s at 48 / 64 / 80 / 96 / 112 samples per unit, isolated kernel 11.67 / 11.60 / 11.60 /
  // 11.68 / 11.70 ms -- fewer refills and retires, and the next frame fills the longer tail.
  int chunk = p->chunk;
  const double rays_per_sample = p->nee_prob > 0.0f ? 5.3 : 8.9;  // HEAD: NEE / cosine only
  const double lane_iters = (double)n_local_pix * s_count * rays_per_sample /
                            ((double)n_cu * variant_bpc * kBlock);
  const bool small_launch = lane_iters < SPT_SMALL_ITERS;
  // A short launch takes at most SPT_SMALL_BPC blocks per CU (half the chip's wave slots): its tail
  // is most of it, and the frame behind it (frames in flight) then runs beside it on the other half
  // instead of only in its tail. C2, round 5 (profiles/r05_blocks_per_cu_ab.json, 4 rounds): bench
  // value 17.9-18.8 -> 21.4-22.1 Gsamples/s, isolated kernel 2.88-2.95 -> 2.84-2.88 ms. Long launches
  // keep every slot (C3 at 4 blocks: isolated +8 %, value within 1 %).
  const int bpc = small_launch ? std::min(variant_bpc, SPT_SMALL_BPC) : variant_bpc;
  const double lanes = (double)n_cu * bpc * kBlock;  // resident lanes of THIS launch
  if (chunk <= 0) {
    if (small_launch) {
      // A short launch (C2: ~860 lane-iterations per lane): deal ~SPT_SMALL_UNITS units per lane
      // and let the in-wave stealing and guided grabs balance the rest (C2: chunk 23 -> 64,
      // 4.6 -> 4.0 ms; measured, scripts/ab_r02e.sh).
      const double units_per_pix = std::max(1.0, std::ceil(SPT_SMALL_UNITS * lanes / std::max(1, n_local_pix)));
      chunk = (int)std::ceil(s_count / units_per_pix);
    } else {
      // SPT_UNITS_PER_LANE units per resident lane (above)...
      const double per_pix = std::max(1.0, SPT_UNITS_PER_LANE * lanes / std::max(1, n_local_pix));
      chunk = (int)std::max(4.0, std::ceil(s_count / per_pix));
    }
    // ...but a unit should last >= ~200 lane-iterations: every unit costs a refill (~35 VALU +
    // ~40 SALU for the whole wave) and a retire (C2: 6 -> 23 samples per unit, 4.73 -> ~4.6 ms).
    chunk = std::max(chunk, (int)std::ceil(200.0 / rays_per_sample));
    chunk = std::min(chunk, s_count);
  }
  {
    const uint32_t waves = (uint32_t)(n_cu * bpc * (kBlock / 64));
    uint32_t sh = 1;  // 2^sh >= 2 x waves
    while ((1u << sh) < 2u * waves && sh < 31) ++sh;
    sh = std::min(31u, sh + (uint32_t)SPT_GUIDED_EXTRA);
    K.sh_guided = small_launch ? sh : 32u;  // guided grabs cost C3 ~1 % (A/B), help C2
  }
  K.chunk = chunk;
  K.steal_min = small_launch ? SPT_STEAL_MIN_SMALL : SPT_STEAL_MIN;
  const uint64_t n_chunks = ((uint64_t)s_count + chunk - 1) / chunk;
  const uint64_t n_units = n_chunks * (uint64_t)n_local_pix;
  if (n_units >= 0x80000000ull) return fail(SPT_ERR_INVALID_ARG, "too many work units; raise chunk");
  K.n_units = (uint32_t)n_units;
  // The young cut, for the variants whose row has it (spt_variants.h), at 8 blocks per CU only (the
  // measured shape): the sphere kernel (C5) lost 3.6 %, the uploaded-geometry kernels 0.5-2.4 % of
  // kernel time or ~1.5 % of pipelined value (profiles/r05_young_cut_ab.json)
  K.young_block = 0xFFFFFFFFu;
  K.young_cut = 0xFFFFFFFFu;
  if (!small_launch && bpc == 8 && kKernelInfo[kv].young_cut && SPT_YOUNG_CUT > 0) {
    K.young_block = (uint32_t)(SPT_YOUNG_RANK * n_cu);
    K.young_cut = (uint32_t)(n_units * (uint64_t)SPT_YOUNG_CUT / 1000u);
  }
  magic31((uint32_t)n_local_pix, &K.m_npix, &K.sh_npix);
  // pixel-order spreading: the largest K = 2^k <= SPT_SCRAMBLE_K dividing n_local_pix
  K.scr_k = 0;
  while ((1 << (K.scr_k + 1)) <= SPT_SCRAMBLE_K && n_local_pix % (1 << (K.scr_k + 1)) == 0) ++K.scr_k;
  K.scr_q = (uint32_t)n_local_pix >> K.scr_k;
  magic31((uint32_t)p->width, &K.m_w, &K.sh_w);
  magic31((uint32_t)K.tile_rows, &K.m_tile, &K.sh_tile);
  K.inv_spp = 1.0f / (float)p->spp;
  K.fix_scale = K.inv_spp * 2147483648.0f;
  K.inv_w = 1.0f / (float)p->width;
  K.inv_h = 1.0f / (float)p->height;
  for (int c = 0; c < 3; ++c) {  // camera of contract v5 (oracle c_path)
    K.cam_au[c] = K.cam[6 + c] * K.inv_w;
    K.cam_av[c] = K.cam[9 + c] * K.inv_h;
    K.cam_cu[c] = K.cam_au[c] * 0x1p-16f;
    K.cam_cv[c] = K.cam_av[c] * 0x1p-16f;
    K.cam_l[c] = K.cam[3 + c] - K.cam[c];
  }
  {  // light sample lattice of contract v5 (oracle c_wrap_sample)
    auto lattice = [](uint32_t dx, float x0, int* on, uint32_t* shift, float* scale, float* x0m1) {
      int a = 0;
      while (a < 32 && dx != 0 && !((dx >> a) & 1u)) ++a;
      *on = dx != 0 && a >= 1 && a <= 24;
      *shift = *on ? 7u + (uint32_t)a : 0u;
      *scale = std::ldexp(1.0f, a - 24);
      *x0m1 = x0 - 1.0f;
    };
    K.ldxi = p->light_mode == SPT_LIGHT_GLIBC_WRAP ? (uint32_t)p->light_dx : 0u;
    K.ldzi = p->light_mode == SPT_LIGHT_GLIBC_WRAP ? (uint32_t)p->light_dz : 0u;
    lattice(K.ldxi, p->light_x0, &K.lx_lattice, &K.lx_shift, &K.lx_scale, &K.lx0m1);
    lattice(K.ldzi, p->light_z0, &K.lz_lattice, &K.lz_shift, &K.lz_scale, &K.lz0m1);
  }
  plan->small_launch = small_launch;
  plan->bpc = bpc;
  plan->grid = n_cu * bpc;
  plan->n_chunks = (uint32_t)n_chunks;
  return SPT_OK;
}

int guide_lanes_per_pixel(int n_cu, int bpc, int n_local_pix, int32_t s_count) {
  const uint64_t lanes = (uint64_t)std::max(1, n_cu) * (uint64_t)std::max(1, bpc) * kBlock;
  int cap = 1;  // the window's sample count rounded up to a power of two
  while (cap < 64 && cap < s_count) cap <<= 1;
  int k = 1;
  while (k < cap && (uint64_t)std::max(1, n_local_pix) * (uint64_t)k < lanes) k <<= 1;
  return k;
}

}  // namespace spt

using namespace spt;

extern "C" int32_t spt_kernel_count(void) { return KV_COUNT; }

extern "C" const char* spt_kernel_name(int32_t id) {
  return id >= 0 && id < KV_COUNT ? kKernelInfo[id].name : nullptr;
}

extern "C" spt_status spt_select_kernel(const spt_prim* prims, int32_t n_prims, const spt_camera* cam,
                                        const spt_params* p, spt_kernel_choice* out) {
  if (!out) return fail(SPT_ERR_INVALID_ARG, "null out");
  SPT_TRY(validate(prims, n_prims, cam, p));
  std::unique_ptr<SceneGeo> g(new SceneGeo);
  int light_pos = -1;
  build_geo(prims, n_prims, g.get(), p->light_id, &light_pos);
  KParams K{};
  const int kv = select_variant(prims, n_prims, cam, p, *g, light_pos, &K);
  out->kernel = kv;
  out->leak_end = K.leak_end;
  out->early_resolve = early_resolve_of(kv, K);
  return SPT_OK;
}

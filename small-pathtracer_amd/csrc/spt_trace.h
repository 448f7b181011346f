// spt_trace.h — the trace layer of the device code: what answers "which primitive does this ray hit,
// and at which t" for the contract of the CPU oracle (oracle c_intersect / c_key / c_sphere), and the
// few pieces every kernel that traces needs around it. Device code only, no kernel:
//   * the opaque uniform pointers (cptr, cptr_at) and the launch's views of the scene (rects_of,
//     tests_of, unit_dirs_of);
//   * the nearest hit: Ray6, the keys, the rect / slab / sphere candidates, intersect_scene;
//   * what a vertex needs from the winner: hit_t, hit_plane_t; the light's own test light_accepts;
//   * a local pixel's Philox key and raster terms (div_magic, pixel_terms);
//   * the SGPR cap the tracing kernels are built under (SPT_NUM_SGPR).
// Included by spt_kernel.hip (render_kernel) and spt_guide.hip (guide_kernel); what only the render
// loop uses (lane states, the early-resolve predicates, the NEE weight, the pool) is spt_kernel.hip's.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

#include "../../include/spt.h"
#include "spt_device.h"
#include "spt_cornell.h"
#include "spt_kparams.h"

namespace spt {

#define SPT_CONST __attribute__((address_space(4)))

// Re-derive a wave-uniform pointer as opaque so uniform loads are re-issued (s_load) where used
// instead of being hoisted into long-lived SGPRs (which spill to VGPR lanes).
template <typename T>
__device__ __forceinline__ const SPT_CONST T* cptr(const T* p) {
  asm volatile("" : "+s"(p));
  return (const SPT_CONST T*)p;
}
// The same at a site of the render loop where a variant's literals may fold every use of the pointer
// away (CAMAX == 1, the LREF constants, light_slot_of of a CONSTGEO kernel): not volatile, so an
// unused one leaves no copy of the pointer pair behind (an s_mov_b64 per site and iteration). It
// takes the loop's counter, which changes every iteration, so it stays where it is written like the
// volatile form, and its site's number, so two sites are never merged into one long-lived pointer.
template <int SITE, typename T>
__device__ __forceinline__ const SPT_CONST T* cptr_at(const T* p, uint32_t it) {
  asm("" : "+s"(p) : "s"(it), "n"(SITE));
  return (const SPT_CONST T*)p;
}

// Rect geometry with literal operands: kCornellRects[i] at a compile-time i (spt_cornell.h).
struct CornellRectPtr {
  int i;
  __device__ constexpr CornellRectPtr operator+(int j) const { return CornellRectPtr{i + j}; }
  __device__ constexpr const CRect* operator->() const { return &kCornellRects[i]; }
};

// The ray-direction contract of the launch (oracle c_unit_dirs; Topo::DIRS).
template <class TP>
__device__ __forceinline__ bool unit_dirs_of(const KParams* Pg) {
  if constexpr (TP::DIRS >= 0) {
    (void)Pg;
    return TP::DIRS == 1;
  } else {
    return cptr(Pg)->unit_dirs != 0;
  }
}
template <class TP>
__device__ __forceinline__ auto rects_of(const SPT_CONST SceneGeo* G) {
  if constexpr (TP::CONSTGEO) return CornellRectPtr{0};
  else return G->rect + 0;
}

struct Ray6 { float oa, ia, db, ob, dc, oc; };
template <int AXIS>  // plane axis: 2 = z (XY rects), 1 = y (XZ), 0 = x (YZ)
__device__ __forceinline__ Ray6 ray6(f3 o, f3 d, float ix, float iy, float iz) {
  if (AXIS == 2) return Ray6{o.z, iz, d.x, o.x, d.y, o.y};
  if (AXIS == 1) return Ray6{o.y, iy, d.x, o.x, d.z, o.z};
  return Ray6{o.x, ix, d.y, o.y, d.z, o.z};
}

// ---- Nearest hit, contract v5 (round 4; oracle c_intersect / c_key). A candidate at t on the plane
// or sphere with grouped position pos is ranked by its KEY: the float bits of t with the low 6 bits
// replaced by pos (negatives, inf and NaN rank last; a plane's zero distance is -2^-149, plane_t,
// and a sphere without a root -0); the nearest hit is the smallest key. Per candidate that is one
// v_bitop3 and one v_min_u32 -- where rounds 1-4 compared keys and selected (t, position) through
// lane masks, a v_cmp -> s_and -> two v_cndmask chain per test. With the rest of contract v5 C3
// 13.55 -> 12.75 ms, and the fma'd -2^-149 below (no "minus one" before the key) 12.92 -> 12.42 ms
// on a slower box (A/B, profiles/r04_ab.txt sessions 2-4).
// A parallel pair's candidate is the smaller of its two planes' keys (the smaller positive t: the
// plane the rounds-1-4 pair rule chose); its in-plane test is evaluated at that plane's t. The
// winner's exact t is recomputed by whoever needs it (shading, NEE weight) from its plane or
// sphere: the same bits as in its key.
constexpr uint32_t kKeyNone = __builtin_bit_cast(uint32_t, 1e20f) | 63u;  // tmin = 1e20 (:324)
// A plane's distance (oracle c_plane_t): (k - o_a) * inv_a as one fma with -2^-149 -- the rounded
// product except at an exact rounding tie, and a zero distance (origin on the plane: :106, :328
// reject it) becomes -2^-149 and ranks last like every negative t, so the key needs no "minus one".
constexpr float kNegTiny = -0x1p-149f;
__device__ __forceinline__ float plane_t(float n, float inv) { return fmaf(n, inv, kNegTiny); }
__device__ __forceinline__ uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }
// (bits(t) | 63) ^ (63 - pos) as ONE v_bitop3 (0x36 = (S0 | S2) ^ S1)
template <int POS>
__device__ __forceinline__ uint32_t key_c(float t) {  // compile-time position (inline constant)
  uint32_t r;
  asm("v_bitop3_b32 %0, %1, %2, 63 bitop3:0x36" : "=v"(r) : "v"(__float_as_uint(t)), "n"(63 - POS));
  return r;
}
__device__ __forceinline__ uint32_t key_v(float t, uint32_t pos) {  // position in a VGPR
  uint32_t r;
  asm("v_bitop3_b32 %0, %1, %2, 63 bitop3:0x36" : "=v"(r) : "v"(__float_as_uint(t)), "v"(63u - pos));
  return r;
}
__device__ __forceinline__ uint32_t key_s(float t, uint32_t pos) {  // wave-uniform position (SGPR)
  uint32_t r;
  asm("v_bitop3_b32 %0, %1, %2, 63 bitop3:0x36" : "=v"(r) : "v"(__float_as_uint(t)), "s"(63u - pos));
  return r;
}

// One rect test (oracle c_intersect): a single (k0 == k1) or a parallel pair. KEYS: the per-plane
// key function for compile-time (CornellTestPtr) or LDS/scalar (GeoTest) geometry.
template <int J> struct CornellTestPtr {
  __device__ constexpr const CTest* operator->() const { return &kCornellTests.t[J]; }
};
// (AXB: the literal kernels' slots with the kind in bits 4 and 5, cornell_slot; KernelTraits::kAxisBits)
template <int J, bool PAIR, bool AXB>
__device__ __forceinline__ void plane_keys(CornellTestPtr<J>, float t0, float t1, uint32_t& kp) {
  constexpr int P0 = cornell_slot(kCornellTests.t[J].pos0, AXB), P1 = cornell_slot(kCornellTests.t[J].pos1, AXB);
  if constexpr (PAIR) kp = umin(key_c<P0>(t0), key_c<P1>(t1));
  else kp = key_c<P0>(t0);
}
template <int J, bool PAIR, bool AXB>  // (unused J, AXB: a runtime pointer, its positions the host's)
__device__ __forceinline__ void plane_keys(const GeoTest* g, float t0, float t1, uint32_t& kp) {
  kp = umin(key_v(t0, (uint32_t)g->pos0), key_v(t1, (uint32_t)g->pos1));
}
template <int J, bool PAIR, bool AXB>
__device__ __forceinline__ void plane_keys(const SPT_CONST GeoTest* g, float t0, float t1, uint32_t& kp) {
  kp = umin(key_v(t0, (uint32_t)g->pos0), key_v(t1, (uint32_t)g->pos1));
}
template <int J, bool PAIR, bool AXB = false, class GP>
__device__ __forceinline__ void rect_cand(GP g, const Ray6& r, uint32_t& tmin) {
  const float t0 = plane_t(g->k0 - r.oa, r.ia);
  float t1 = t0;
  uint32_t kb = __float_as_uint(t0), kp;
  if constexpr (PAIR) {
    t1 = plane_t(g->k1 - r.oa, r.ia);
    kb = umin(kb, __float_as_uint(t1));
  }
  plane_keys<J, PAIR, AXB>(g, t0, t1, kp);
  const float tb = __uint_as_float(kb);  // the chosen plane's t
  // in-plane offsets from the centre, a = d_b * t + (o_b - mid_b): the origin's offset is per ray
  // and shared by every rectangle with that centre (CSE'd across the unrolled tests)
  const float a = fmaf(r.db, tb, r.ob - g->ma), b = fmaf(r.dc, tb, r.oc - g->mb);
  const bool inb = (bool)((int)(fabsf(a) <= g->ha) & (int)(fabsf(b) <= g->hb));
  tmin = umin(tmin, inb ? kp : 0xFFFFFFFFu);
}
template <int J, bool AXB>
__device__ __forceinline__ void cornell_test(const Ray6* rays, uint32_t& tmin) {
  constexpr CTest T = kCornellTests.t[J];
  if constexpr (J != kCornellRoom[0] && J != kCornellRoom[1] && J != kCornellRoom[2] && !cornell_in_box(J))
    rect_cand<J, T.pos0 != T.pos1, AXB>(CornellTestPtr<J>{}, rays[T.axis], tmin);
}
// A box of contract v6 (oracle c_find_boxes / c_intersect): an XY pair Z (planes z), a YZ pair X
// (planes x) and an XZ top, standing on the room's floor F (the room's XZ pair, k0). Per axis the two
// planes' keys as signed integers -- for t >= 0 the integer order is the order of t, and every
// negative t is a negative integer -- give the slab interval [min, max]; entry = the largest start,
// exit = the smallest end, crossed iff entry <= exit. The candidate is the entry, or for an origin
// inside the box (negative entry) the exit face, as the per-face tests find it: as unsigned keys
// min(entry, exit). Per box 6 plane keys, 5 integer min/max, 3 xors (imax_of), one compare: the 4
// faces' and the top's in-plane compares and lane-mask selects are gone (trace 153 -> 131 VALU per
// wave-iteration).
__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }
// A slab's end is a ^ b ^ min(a, b): max(a, b) for every pair of 32-bit integers (the min is one of
// the two, and the xor leaves the other), so a NaN key goes through as it did. One full-rate v_bitop3
// where v_max_i32 issues at half rate (spt_device.h, xor3): three slots fewer per box.
__device__ __forceinline__ int imax_of(int a, int b, int mn) {
  return (int)xor3((uint32_t)a, (uint32_t)b, (uint32_t)mn);
}
__device__ __forceinline__ void box_keys(int kx0, int kx1, int kz0, int kz1, int ky0, int ky1,
                                         uint32_t& tmin) {
  const int nx = imin(kx0, kx1), nz = imin(kz0, kz1), ny = imin(ky0, ky1);
  const int en = imax(imax(nx, nz), ny);
  const int ex = imin(imin(imax_of(kx0, kx1, nx), imax_of(kz0, kz1, nz)), imax_of(ky0, ky1, ny));
  tmin = umin(tmin, en <= ex ? umin((uint32_t)en, (uint32_t)ex) : 0xFFFFFFFFu);
}
// The room of contract v6 as the same slab (from inside: the exit face, the nearest positive wall)
template <bool AXB>
__device__ __forceinline__ void cornell_room(const Ray6* rays, uint32_t& tmin) {
  constexpr CTest Z = kCornellTests.t[kCornellRoom[0]], Y = kCornellTests.t[kCornellRoom[1]];
  constexpr CTest X = kCornellTests.t[kCornellRoom[2]];
  const Ray6 &rz = rays[2], &ry = rays[1], &rx = rays[0];
  // The two planes at k = +0 (Front, Bottom): (0 - o) * inv - 2^-149 as ONE fma with a negated source
  // where the subtract and a v_fmaak stood. 0 - o is -o for every o but +0, where it is +0 and -o is
  // -0; fma(+-0, inv, -2^-149) is -2^-149 for either zero (NaN for an infinite or NaN inv, either
  // way), so the distance is the same bits.
  static_assert(__builtin_bit_cast(uint32_t, Z.k0) == 0u && __builtin_bit_cast(uint32_t, Y.k0) == 0u,
                "HEAD room: Front z = +0, Bottom y = +0");
  box_keys((int)key_c<cornell_slot(X.pos0, AXB)>(plane_t(X.k0 - rx.oa, rx.ia)), (int)key_c<cornell_slot(X.pos1, AXB)>(plane_t(X.k1 - rx.oa, rx.ia)),
           (int)key_c<cornell_slot(Z.pos0, AXB)>(plane_t(-rz.oa, rz.ia)), (int)key_c<cornell_slot(Z.pos1, AXB)>(plane_t(Z.k1 - rz.oa, rz.ia)),
           (int)key_c<cornell_slot(Y.pos0, AXB)>(plane_t(-ry.oa, ry.ia)), (int)key_c<cornell_slot(Y.pos1, AXB)>(plane_t(Y.k1 - ry.oa, ry.ia)),
           tmin);
}
template <int B, bool AXB>
__device__ __forceinline__ void cornell_box(const Ray6* rays, uint32_t& tmin) {
  constexpr CTest Z = kCornellTests.t[kCornellBoxes.t[B][0]], X = kCornellTests.t[kCornellBoxes.t[B][1]];
  constexpr CTest T = kCornellTests.t[kCornellBoxes.t[B][2]], F = kCornellTests.t[kCornellRoom[1]];
  const Ray6 &rz = rays[2], &ry = rays[1], &rx = rays[0];
  box_keys((int)key_c<cornell_slot(X.pos0, AXB)>(plane_t(X.k0 - rx.oa, rx.ia)), (int)key_c<cornell_slot(X.pos1, AXB)>(plane_t(X.k1 - rx.oa, rx.ia)),
           (int)key_c<cornell_slot(Z.pos0, AXB)>(plane_t(Z.k0 - rz.oa, rz.ia)), (int)key_c<cornell_slot(Z.pos1, AXB)>(plane_t(Z.k1 - rz.oa, rz.ia)),
           // (the floor's key as cornell_room spells it: the same value, CSE'd)
           (int)key_c<cornell_slot(F.pos0, AXB)>(plane_t(-ry.oa, ry.ia)), (int)key_c<cornell_slot(T.pos0, AXB)>(plane_t(T.k0 - ry.oa, ry.ia)),
           tmin);
}
template <bool AXB, int... B>
__device__ __forceinline__ void cornell_boxes(std::integer_sequence<int, B...>, const Ray6* rays,
                                              uint32_t& tmin) {
  (cornell_box<B, AXB>(rays, tmin), ...);
}
// The same for uploaded geometry: the room (rm[0] its XY pair, rm[1] XZ, rm[2] YZ) and a box (bx[0]
// the XY pair, bx[1] the YZ pair, bx[2] the top; fl the room's XZ pair, its k0 the floor)
template <class GT>
__device__ __forceinline__ void geo_room(GT rm, const Ray6& rz, const Ray6& ry, const Ray6& rx,
                                         uint32_t& tmin) {
  box_keys((int)key_v(plane_t(rm[2].k0 - rx.oa, rx.ia), (uint32_t)rm[2].pos0),
           (int)key_v(plane_t(rm[2].k1 - rx.oa, rx.ia), (uint32_t)rm[2].pos1),
           (int)key_v(plane_t(rm[0].k0 - rz.oa, rz.ia), (uint32_t)rm[0].pos0),
           (int)key_v(plane_t(rm[0].k1 - rz.oa, rz.ia), (uint32_t)rm[0].pos1),
           (int)key_v(plane_t(rm[1].k0 - ry.oa, ry.ia), (uint32_t)rm[1].pos0),
           (int)key_v(plane_t(rm[1].k1 - ry.oa, ry.ia), (uint32_t)rm[1].pos1), tmin);
}
template <class GT>
__device__ __forceinline__ void geo_box(GT bx, GT fl, const Ray6& rz, const Ray6& ry, const Ray6& rx,
                                        uint32_t& tmin) {
  box_keys((int)key_v(plane_t(bx[1].k0 - rx.oa, rx.ia), (uint32_t)bx[1].pos0),
           (int)key_v(plane_t(bx[1].k1 - rx.oa, rx.ia), (uint32_t)bx[1].pos1),
           (int)key_v(plane_t(bx[0].k0 - rz.oa, rz.ia), (uint32_t)bx[0].pos0),
           (int)key_v(plane_t(bx[0].k1 - rz.oa, rz.ia), (uint32_t)bx[0].pos1),
           (int)key_v(plane_t(fl->k0 - ry.oa, ry.ia), (uint32_t)fl->pos0),
           (int)key_v(plane_t(bx[2].k0 - ry.oa, ry.ia), (uint32_t)bx[2].pos0), tmin);
}
template <bool AXB, int... J>
__device__ __forceinline__ void cornell_tests(std::integer_sequence<int, J...>, const Ray6* rays,
                                              uint32_t& tmin) {
  (cornell_test<J, AXB>(rays, tmin), ...);
}

template <int N, class GT>  // the tests of one kind group, uploaded geometry (every test as a pair)
__device__ __forceinline__ void test_group(GT g, int n_rt, const Ray6& r, uint32_t& tmin) {
  if constexpr (N >= 0) {
#pragma unroll
    for (int j = 0; j < N; ++j) rect_cand<0, true>(g + j, r, tmin);
  } else {
    for (int j = 0; j < n_rt; ++j) rect_cand<0, true>(g + j, r, tmin);
  }
}

// One rectangle's own test (a single, as inside the trace: contract v5): t, whether its in-plane
// test at t- accepts, and the first in-plane offset there.
struct RectHit { float tt; bool inb; float a; };  // a: first in-plane offset from the centre
template <class GP>
__device__ __forceinline__ RectHit rect_eval(GP g, const Ray6& r) {
  const float tt = plane_t(g->k - r.oa, r.ia);
  const float a = fmaf(r.db, tt, r.ob - g->ma), b = fmaf(r.dc, tt, r.oc - g->mb);
  const bool ia = fabsf(a) <= g->ha, ib = fabsf(b) <= g->hb;
  return RectHit{tt, (bool)((int)ia & (int)ib), a};
}
// The uploaded light of the room-literal UPLIGHT kernels (a single XZ test at the HEAD light's grouped
// position, read from the uploaded scene through scalar loads): rect_cand's arithmetic for a single,
// with the position literal.
template <bool AXB, class GT>
__device__ __forceinline__ void light_cand(const GT& g, const Ray6& r, uint32_t& tmin) {
  const float t0 = plane_t(g.k0 - r.oa, r.ia);
  const float a = fmaf(r.db, t0, r.ob - g.ma), b = fmaf(r.dc, t0, r.oc - g.mb);
  const bool inb = (bool)((int)(fabsf(a) <= g.ha) & (int)(fabsf(b) <= g.hb));
  tmin = umin(tmin, inb ? key_c<cornell_slot(kCornellLightPos, AXB)>(t0) : 0xFFFFFFFFu);
}
// The same light's own test (rect_eval on a GeoTest): t and whether the in-plane test accepts.
template <class GT>
__device__ __forceinline__ RectHit rect_eval_test(const GT& g, const Ray6& r) {
  const float tt = plane_t(g.k0 - r.oa, r.ia);
  const float a = fmaf(r.db, tt, r.ob - g.ma), b = fmaf(r.dc, tt, r.oc - g.mb);
  const bool ia = fabsf(a) <= g.ha, ib = fabsf(b) <= g.hb;
  return RectHit{tt, (bool)((int)ia & (int)ib), a};
}
// A candidate at t with position pos can be the nearest hit at all: its key
// (bits(t) | 63) ^ (63 - pos) ranks below kKeyNone = bits(1e20) | 63, i.e. bits(t) <= kKeyNone for
// pos < 63 (one compare) and bits(t) < kKeyNone & ~63 for pos 63.
__device__ __forceinline__ bool key_valid(float t, uint32_t pos) {
  return pos < 63u ? __float_as_uint(t) <= kKeyNone : __float_as_uint(t) < (kKeyNone & ~63u);
}

template <class SP>
__device__ __forceinline__ float sphere_t(const SP& S, f3 o, f3 d) {
  // Sphere::intersect :229-239 in the reference's own form det = b^2 - op.op + r^2 (:233), as
  // fma(b, b, r^2 - op.op); nearest root beyond the fp32 epsilon. (Round 2: the cancellation-free
  // r^2 - |op - b d|^2 cost 2 more VALU per sphere: C5 at 256 spp 430.4 -> 406.5 ms.)
  const f3 op = mk(S.px - o.x, S.py - o.y, S.pz - o.z);
  const float bb = dot3(op, d);
  const float det = fmaf(bb, bb, S.rad2 - dot3(op, op));
  if (!(det >= 0.0f)) return -0.0f;  // no root: -0 ranks last (contract v5 key)
  // the root as det * rsq_nr2(det) (contract, oracle c_sphere): the IEEE sqrtf sequence costs ~18
  // issue slots, det * rsq_nr(det) 13 (round 2: C5 at 256 spp 452.8 -> 427.3 ms), two Newton steps
  // 10 (round 3: the root within 5e-6 relative, 3e-5 at r = 6, far below the 2e-3 epsilon);
  // det = 0 gives 0
  const float sd = det * rsq_nr2(det);
  const float t1 = bb - sd, t2 = bb + sd;
  return t1 > 2e-3f ? t1 : (t2 > 2e-3f ? t2 : -0.0f);
}

// A wide sphere (the 1e5 walls and the radius-600 light of the classic smallpt box) in fp64: the
// cancellation-free quadratic with explicit fma, IEEE double division and sqrt, the fp32 contract's
// epsilon; t rounded to float (oracle c_sphere_wide). The fp32-normalised direction is not exactly
// unit (|d|^2 = 1 + e, |e| ~ 1e-7), and a radius-1e5 quadratic that assumed |d| = 1 would carry an
// error e * b^2 ~ 1e3 in its discriminant (hit points off the wall by ~0.1: self-hits in rings), so
// the quadratic keeps a = d.d: t = k -+ sqrt(det / a), k = (op.d) / a, det = r^2 - |op - k d|^2.
__device__ __forceinline__ float sphere_t_wide(const SPT_CONST GeoSphD& S, f3 o, f3 d) {
  const double ox = S.px - (double)o.x, oy = S.py - (double)o.y, oz = S.pz - (double)o.z;
  const double dx = d.x, dy = d.y, dz = d.z;
  const double a = fma(dz, dz, fma(dy, dy, dx * dx));
  const double k = fma(oz, dz, fma(oy, dy, ox * dx)) / a;
  const double qx = fma(-k, dx, ox), qy = fma(-k, dy, oy), qz = fma(-k, dz, oz);
  const double det = S.rad2 - fma(qz, qz, fma(qy, qy, qx * qx));
  if (!(det >= 0.0)) return -0.0f;
  const double sd = sqrt(det / a);
  const double t1 = k - sd, t2 = k + sd;
  return (float)(t1 > 2e-3 ? t1 : (t2 > 2e-3 ? t2 : -0.0));
}
__device__ __forceinline__ float sphere_t_any(const SPT_CONST SceneGeo* G, int j, f3 o, f3 d) {
  if (G->sph[j].wide) return sphere_t_wide(G->sphd[j], o, d);  // wave-uniform (scalar load)
  return sphere_t(G->sph[j], o, d);
}

template <class TP>
__device__ __forceinline__ int n_of(int ct, int rt) { return ct >= 0 ? ct : rt; }

// The uploaded scene's rect tests are read from an LDS copy staged once per block (ds_read
// broadcasts into VGPRs) -- the north star's "geometry staged once into LDS". A/B (DESIGN.md
// section 4, round 2 at commit 407a07d): faster than scalar loads through the constant address
// space: generic kernel at C3 27.65 -> 26.26 ms, HEAD-topology kernel 19.1 -> 18.5 ms, C5 at
// 256 spp 460 -> 453.6 ms. Spheres stay on scalar loads (an LDS copy cost C5 1.4 %: four VGPRs per
// unrolled sphere). The HEAD scene itself runs with its bounds as instruction literals (15.5 ms).
// (the fp64 wide-sphere kernel keeps scalar loads: its VGPR budget is the tight one, 78 vs 90)
template <class TP>
__device__ __forceinline__ auto tests_of(const SPT_CONST SceneGeo* G, const GeoTest* lds) {
  constexpr bool kLds = !TP::WIDE;
  if constexpr (TP::CONSTGEO && !TP::UPBOX) {
    (void)G; (void)lds;
    return (const SPT_CONST GeoTest*)nullptr;  // the HEAD tests are literals (kCornellTests)
  } else if constexpr (kLds) {
    (void)G;
    return lds;
  } else {
    (void)lds;
    return G->test + 0;
  }
}
// The scene's room of contract v5 in uploaded geometry: SceneGeo.room_test[] (three GeoTests kept
// out of the per-kind test lists) and the box (host build_geo, oracle c_find_room).
// AXB (KernelTraits::kAxisBits; literal kernels): the keys carry cornell_slot's numbering, and so do
// the positions of the uploaded boxes' tests the kernel staged; id and pos_out are slots.
// MISS (KernelTraits::kMissEntry; literal leak-end kernels): a miss reports the "no hit" key's own
// low bits, slot 63, as its position and id, without the select.
template <class TP, bool AXB = false, bool MISS = false, class GP, class GT, class SP>
__device__ __forceinline__ bool intersect_scene(const SPT_CONST SceneGeo* G, GP rect, GT tests,
                                                SP sphs, const int* pos2idx, f3 o, f3 d, int& id,
                                                float& ia_hit, int& pos_out, f3& inv) {
  const float ix = rcp_nr(d.x), iy = rcp_nr(d.y), iz = rcp_nr(d.z);
  inv = mk(ix, iy, iz);
  uint32_t tmin = kKeyNone;
  if constexpr (TP::CONSTGEO) {
    const Ray6 rays[3] = {ray6<0>(o, d, ix, iy, iz), ray6<1>(o, d, ix, iy, iz),
                          ray6<2>(o, d, ix, iy, iz)};
    cornell_room<AXB>(rays, tmin);
    if constexpr (TP::UPBOX) {
      // the uploaded HEAD-topology tests (host-checked: n_txy 0, n_txz 1, n_tyz 0): the light, the
      // room's three pairs (its XZ pair's k0 the floor), then the two boxes' three tests each. The
      // room is literal (HEAD's, host-checked), the boxes come from LDS, the light is literal or
      // (UPLIGHT) read through scalar loads from the uploaded scene
      if constexpr (TP::UPLIGHT) light_cand<AXB>(G->test[0], rays[1], tmin);
      else cornell_tests<AXB>(std::make_integer_sequence<int, kCornellTests.n>{}, rays, tmin);  // the light
      geo_box(tests + 4, tests + 2, rays[2], rays[1], rays[0], tmin);
      geo_box(tests + 7, tests + 2, rays[2], rays[1], rays[0], tmin);
    } else {
      cornell_tests<AXB>(std::make_integer_sequence<int, kCornellTests.n>{}, rays, tmin);  // the light
      cornell_boxes<AXB>(std::make_integer_sequence<int, kCornellBoxes.n>{}, rays, tmin);
    }
  } else {
    const int ntxy = n_of<TP>(TP::NTXY, G->n_txy), ntxz = n_of<TP>(TP::NTXZ, G->n_txz);
    const int ntyz = n_of<TP>(TP::NTYZ, G->n_tyz);
    const Ray6 rz = ray6<2>(o, d, ix, iy, iz), ry = ray6<1>(o, d, ix, iy, iz), rx = ray6<0>(o, d, ix, iy, iz);
    if (G->has_room) {  // wave-uniform; the room tests follow the per-kind lists, then the boxes
      const int nt = ntxy + ntxz + ntyz;
      geo_room(tests + nt, rz, ry, rx, tmin);
      const int nbox = n_of<TP>(TP::NBOX, G->n_box);
      for (int b = 0; b < nbox; ++b) geo_box(tests + nt + 3 + 3 * b, tests + nt + 1, rz, ry, rx, tmin);
    }
    test_group<TP::NTXY>(tests, ntxy, rz, tmin);
    test_group<TP::NTXZ>(tests + ntxy, ntxz, ry, tmin);
    test_group<TP::NTYZ>(tests + ntxy + ntxz, ntyz, rx, tmin);
  }
  (void)rect;
  if constexpr (TP::SPH) {
    const int nsph = G->n_sph, nnar = nsph - G->n_sph_wide, base = G->n_xy + G->n_xz + G->n_yz;
    // unrolled by 4 so the scalar loads of several spheres are issued before one wait; 4, not 8:
    // the 32 SGPRs of 8 spheres pushed the SGPR-capped sphere kernel to 65 VGPRs (7 waves/SIMD);
    // at 4 it has 63 (8 waves): C5 at 256 spp 475 -> 467 ms. By hand, remainder first: the key's
    // inline asm is convergent, and LLVM does not runtime-unroll a loop that holds convergent code.
    auto sph_key = [&](int j) { tmin = umin(tmin, key_s(sphere_t(sphs[j], o, d), (uint32_t)(base + j))); };
    int j = 0;
    for (; j < (nnar & 3); ++j) sph_key(j);
    for (; j < nnar; j += 4) {
      sph_key(j);
      sph_key(j + 1);
      sph_key(j + 2);
      sph_key(j + 3);
    }
    if constexpr (TP::WIDE) {
      for (int j = nnar; j < nsph; ++j)  // wide spheres (fp64)
        tmin = umin(tmin, key_s(sphere_t_wide(G->sphd[j], o, d), (uint32_t)(base + j)));
    }
  }
  const bool hit = tmin < kKeyNone;
  int pos = (int)(tmin & 63u);  // (63 on a miss: a valid LDS index, the id is kept)
  // HEAD kernels: a miss reports the position of prim 0, whose id a missed path ray keeps (:373-374),
  // so the shading takes the hit's plane axis from the same two position compares as ia_hit.
  // MISS: a miss ends the path in the shading block that follows, and nothing the lane makes from the
  // hit's position or primitive is read after it but the emission its L takes, T * e: the lane reads
  // slot 63, which the kernel stages with zero emission, and adds T * 0 as it did with prim 0's
  static_assert(!MISS || TP::CONSTGEO, "MISS: a literal kernel");
  if constexpr (TP::CONSTGEO && !MISS) pos = hit ? pos : cornell_slot(kCornellPosOfPrim0, AXB);
  // 1/d of the hit rectangle's plane axis (the winner's t and its hit point, see the shading)
  const int nxy = TP::CONSTGEO ? kCornellNXY : n_of<TP>(TP::NXY, G->n_xy);
  const int nxz = TP::CONSTGEO ? kCornellNXZ : n_of<TP>(TP::NXZ, G->n_xz);
  // (the HEAD kernels select it where it is used, from the shading's own plane-axis masks)
  if constexpr (!TP::CONSTGEO) ia_hit = pos < nxy ? iz : (pos < nxy + nxz ? iy : ix);
  // HEAD kernels: the kernel's primitive ids ARE the grouped positions (s_prims is loaded in that
  // order), so no pos -> index lookup; otherwise an unconditional LDS read (no branch)
  int idn;
  if constexpr (TP::CONSTGEO) idn = pos;
  else idn = keep(pos2idx[pos]);
  if constexpr (MISS) id = idn;  // (no shadow ray of these kernels misses: none keeps a vertex's id)
  else id = hit ? idn : id;
  pos_out = pos;
  return hit;
}

// The winner's exact t (contract v5: the t its key was made from), for a hit on prims[id] = H at
// grouped position pos: a rectangle's (k - o_a) * inv_a, a sphere's nearest root (sphere_t on the
// same fp32 values as the trace's GeoSph: DevPrim w1..w4 = px, py, pz, r^2), a wide sphere's fp64
// root.
template <class TP>
__device__ __forceinline__ float hit_t(const DevPrim& H, int pos, f3 o, f3 d, float ia,
                                       const SPT_CONST SceneGeo* G) {
  if (H.kind == SPT_RECT_XY) return plane_t(H.w1 - o.z, ia);
  if (H.kind == SPT_RECT_XZ) return plane_t(H.w1 - o.y, ia);
  if (H.kind == SPT_RECT_YZ) return plane_t(H.w1 - o.x, ia);
  if constexpr (TP::WIDE) {
    const int j = pos - (G->n_xy + G->n_xz + G->n_yz);
    if (j >= G->n_sph - G->n_sph_wide) return sphere_t_wide(G->sphd[j], o, d);
  }
  return sphere_t(GeoSph{H.w1, H.w2, H.w3, H.w4, 0, 0, 0, 0}, o, d);
}

// NEE pre-test (light_sampling :363-369 + the shadow ray of :466): is the light itself accepted
// on the ray (x, dl)? Only then can the nearest hit be the light (:467), so only these rays are
// traced against the scene. Bit-identical to the light's own test inside intersect_scene().
template <class TP, class GP>
__device__ __forceinline__ bool light_accepts(const SPT_CONST KParams* P, const SPT_CONST SceneGeo* G,
                                              GP rect, f3 o, f3 d) {
  if constexpr (TP::LPOS >= 0) {
    constexpr int L = TP::LPOS;  // compile-time kind from the grouped position
    static_assert(TP::NXY >= 0 && TP::NXZ >= 0, "LPOS needs static group sizes");
    if constexpr (L < TP::NXY) {
      const RectHit h = rect_eval(rect + L, Ray6{o.z, rcp_nr(d.z), d.x, o.x, d.y, o.y});
      return h.inb & key_valid(h.tt, L);
    } else if constexpr (L < TP::NXY + TP::NXZ) {
      const RectHit h = rect_eval(rect + L, Ray6{o.y, rcp_nr(d.y), d.x, o.x, d.z, o.z});
      return h.inb & key_valid(h.tt, L);
    } else {
      const RectHit h = rect_eval(rect + L, Ray6{o.x, rcp_nr(d.x), d.y, o.y, d.z, o.z});
      return h.inb & key_valid(h.tt, L);
    }
  } else {
    const int lk = P->light_kind, L = P->light_pos;
    if (L < 0) return false;
    const int nrect = G->n_xy + G->n_xz + G->n_yz;
    if (lk == SPT_SPHERE)  // (light_pos: the index in sph[]; its grouped position follows the rects)
      return key_valid(TP::WIDE ? sphere_t_any(G, L, o, d) : sphere_t(G->sph[L], o, d), (uint32_t)(nrect + L));
    Ray6 r;
    if (lk == SPT_RECT_XY) r = Ray6{o.z, rcp_nr(d.z), d.x, o.x, d.y, o.y};
    else if (lk == SPT_RECT_XZ) r = Ray6{o.y, rcp_nr(d.y), d.x, o.x, d.z, o.z};
    else r = Ray6{o.x, rcp_nr(d.x), d.y, o.y, d.z, o.z};
    const RectHit h = rect_eval(rect + L, r);
    return h.inb & key_valid(h.tt, (uint32_t)L);
  }
}

// The hit point's plane distance (n / d_a of :103, n = k - o_a), as one Markstein correction of the
// trace's t = n * rcp_nr(d_a) (oracle c_hit_t): r = n - t*d_a exactly (fma), t + r * rcp. Equal to
// the IEEE quotient in all of 2e8 sampled cases; the contract spells it out so CPU and GPU agree
// by construction.
__device__ __forceinline__ float hit_plane_t(float n, float da, float ia, float t) {
  return fmaf(fmaf(-t, da, n), ia, t);
}

__device__ __forceinline__ uint32_t div_magic(uint32_t n, uint32_t m, uint32_t sh) {
  return (uint32_t)(((uint64_t)n * m) >> sh);
}

// A local pixel index (row-tile shard order) -> the Philox pixel key and camera raster terms.
// LIST (a launch over a pixel list, an adaptive film's pass): lp is the launch's virtual index and
// Q->pix_list[lp] the real local pixel. The translation happens here and nowhere else: the lane
// state, accum, the slots and the finalize order keep the virtual index. A per-lane vector load at
// the pool fill (or the per-lane set-up of the Topo::MAT kernels), never in the loop body.
template <bool LIST>
__device__ __forceinline__ void pixel_terms(const SPT_CONST KParams* Q, uint32_t lp, PxKey& pk,
                                            float& fx, float& fy) {
  if constexpr (LIST) lp = Q->pix_list[lp];
  const uint32_t w = (uint32_t)Q->width;
  const uint32_t lr = div_magic(lp, Q->m_w, Q->sh_w);
  const int px = (int)(lp - lr * w);
  const uint32_t T_ = (uint32_t)Q->tile_rows;
  const uint32_t tile = div_magic(lr, Q->m_tile, Q->sh_tile), within = lr - tile * T_;
  const int py = (int)((tile * (uint32_t)Q->shard_count + (uint32_t)Q->shard_index) * T_ + within);
  pk = philox_pixel_key((uint32_t)py * w + (uint32_t)px, Q->seed);
  // camera raster terms (x - 0.5), (h - y - 1 - 0.5) of :533-534, less 128 (jitter_fma)
  fx = ((float)px - 0.5f) - 128.0f;
  fy = ((float)(Q->height - py - 1) - 0.5f) - 128.0f;
}

// The kernels that trace (render_kernel, guide_kernel) cap their SGPRs at 80: with 81-96 SGPRs a CU
// admits only 7 blocks of 256 threads, not the 8 that the compiler's occupancy report and
// hipOccupancyMaxActiveBlocksPerMultiprocessor() claim (MI355X_MICROARCH "256-thread blocks are
// admitted per CU up to min(API, 8, floor(800 / (ceil(sgpr/16)*16 + 16)))"; measured on render_kernel
// with per-wave start times: the 8th block of every CU started only when the first ones retired; C3
// 16.2 -> 16.0 ms, C2 4.77 -> 4.60 ms). Under the cap the occupancy API is exact.
#ifndef SPT_NUM_SGPR
#define SPT_NUM_SGPR 80
#endif

}  // namespace spt

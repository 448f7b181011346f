// spt_kparams.h — what the kernels that trace (spt_kernel.hip, spt_guide.hip, spt_guide_light.hip; spt_trace.h) and their
// host side (spt_dispatch.cpp, spt_context.cpp) share: the uploaded scene and parameter structs, the launch constants and the
// tuning macros with their A/B history. Plain C++. The statistics words depend on the diagnostic
// build (spt_diag.h), so -DSPT_DIAG builds agree between host and device.
#pragma once
#include <stdint.h>

#include "spt_diag.h"

namespace spt {

constexpr int kMaxPrims = 64;
constexpr int kBlock = 256;
// Units fetched per queue atomic. Measured (1 GPU): 8/16/32 slower (C2 5.6/5.0/4.7 ms vs 4.6:
// atomics), 128/256 slower for C3 (16.7/17.3 vs 16.0 ms: work hoarded in one wave's pool when the
// queue drains) though faster for C2 (4.45 ms); a guided scheme (static first slice per wave, then
// shares of what is left, 16..256) was 6 % slower on C3-C5.
#ifndef SPT_GRAB
#define SPT_GRAB 64
#endif
constexpr uint32_t kGrab = SPT_GRAB;
// Guided grabs of short launches: left >> (log2(2 x waves) + SPT_GUIDED_EXTRA) units, at least
// SPT_GRAB_MIN. Round 3 (C2, 8 rounds on two boxes): 16 / +0 -> 8 / +1 cut the kernel 1.0-1.6 %;
// 8 / +0, 4 / +0, 16 / +1 and 4 / +2 did not (profiles/r03_ab.txt session 10).
#ifndef SPT_GRAB_MIN
#define SPT_GRAB_MIN 8
#endif
#ifndef SPT_GUIDED_EXTRA
#define SPT_GUIDED_EXTRA 1
#endif
constexpr uint32_t kGrabMin = SPT_GRAB_MIN;  // guided grabs never take fewer (bounds the queue atomics)
// Pool set-up through LDS (render_kernel, refill): the wave that grabs a pool computes the terms of
// all its units at once, lane i those of unit pool_next + i, into a region of LDS of its own, and a
// lane that takes a unit reads its entry where it used to compute it (the whole wave paid ~60
// issue slots for the 1.2 lanes an average refill serves). 0: every lane sets its own unit up, as
// rounds 1-6 did. The generic kernels (Topo::MAT: the REFR stack holds their LDS) always do.
#ifndef SPT_POOL_LDS
#define SPT_POOL_LDS 1
#endif
// An entry: two 16-byte halves, kept in two arrays so that both the fill (consecutive entries) and
// the fetch read and write whole 128-bit words at a 16-byte stride (no bank conflict). The entry
// of unit u is u mod 64: a pool is at most 64 consecutive units, one per lane of the fill (a build
// with a larger SPT_GRAB keeps the per-lane set-up).
constexpr bool kPoolLdsBuild = SPT_POOL_LDS != 0 && kGrab <= 64;
struct alignas(16) PoolEntryA { uint32_t s, qhi, qlo, lo; };  // first sample; the Philox pixel key (PxKey)
struct alignas(16) PoolEntryB { float fx, fy, fz; uint32_t s_end; };  // camera terms; end of the sample range
static_assert(sizeof(PoolEntryA) == 16 && sizeof(PoolEntryB) == 16, "pool entry layout");
// Launches with fewer lane-iterations per resident lane than SPT_SMALL_ITERS deal their units
// almost all at once (SPT_SMALL_UNITS per lane) and balance by stealing (host, plan_launch).
#ifndef SPT_SMALL_ITERS
#define SPT_SMALL_ITERS 2000.0
#endif
#ifndef SPT_SMALL_UNITS
#define SPT_SMALL_UNITS 1.5
#endif
#ifndef SPT_SMALL_BPC
#define SPT_SMALL_BPC 4  // resident blocks per CU of a short launch (host, plan_launch)
#endif
// Units per resident lane of a long launch (host, plan_launch): 8 since round 4 (was 16)
#ifndef SPT_UNITS_PER_LANE
#define SPT_UNITS_PER_LANE 8.0
#endif
// Young blocks of a long launch (host, plan_launch): the waves of the blocks a CU received
// last (blockIdx >= SPT_YOUNG_RANK x n_cu at 8 blocks per CU) take no new pool once SPT_YOUNG_CUT per
// mille of the units are handed out. The SIMD issues oldest-first, so these waves get the fewest
// slots (C3: the two youngest of a CU's 8 blocks do ~4 % of the work) and the units they hold end
// the launch. Round 5 A/B (profiles/r05_young_cut_ab.json): C3 isolated kernel -1.3 to -1.6 %,
// C4 -0.8 %, values flat; applied to the literal HEAD NEE kernels (and their any-camera forms) and
// the room-literal edited-scene NEE kernels (KV_UPBOX_NEE: -4 %; KV_UPLIGHT_NEE, round 6) only (the
// others lost). It assumes the dispatcher hands
// each CU its blocks in blockIdx order, so blockIdx >= SPT_YOUNG_RANK x n_cu are the blocks a CU
// received last; that holds only with every CU full at 8 blocks, so the host applies it at bpc == 8.
#ifndef SPT_YOUNG_CUT
#define SPT_YOUNG_CUT 300
#endif
#ifndef SPT_YOUNG_RANK
#define SPT_YOUNG_RANK 6
#endif
#ifndef SPT_SCRAMBLE_K
#define SPT_SCRAMBLE_K 8  // pixel-order spreading factor of the work units (1 = off; A/B in DESIGN.md §4)
#endif
// Unit slots: a unit's owner lane stores its three sums to the unit's own slot (plain stores, no
// atomics); only stolen ranges add into the per-pixel accumulator; finalize_slots_kernel sums both
// (rounds 1-2 added every unit's sums atomically)
#ifndef SPT_STEAL_MIN
#define SPT_STEAL_MIN 8  // unstarted samples a donor must hold (in-wave stealing; A/B in DESIGN.md §4)
#endif
#ifndef SPT_STEAL_MIN_SMALL
#define SPT_STEAL_MIN_SMALL 16  // the same for short launches (C2: +2-3 %, profiles/r04_ab.txt s. 9)
#endif
#ifdef SPT_WAVE_TIMES
constexpr int kStatWords = 32 + 3 * 32768;  // diagnostic: per-wave start, end, iterations
#else
constexpr int kStatWords = 32;
#endif
// stats[]: [0] waves that hit kMaxWaveIters, [1,8) path statistics (spt_stats order), [8] shadow
// rays that passed the light pre-test, [9] sphere vertices, [10] shadow rays of those resolved
// without a trace (early_nee_proven), [12,32) region stats (diagnostic build)
[[maybe_unused]] constexpr int kStatShadowTraced = 8, kStatSphereVertices = 9, kStatShadowProven = 10,
                               kStatRegion = 12;

// 64-byte device primitive. rect: w1..w5 = k, b1, b2, c1, c2 (in-plane bounds of the two free
// axes in (x,y,z) order); sphere: w1..w5 = px, py, pz, rad^2, 1/rad.
struct alignas(16) DevPrim {
  int kind;
  float w1, w2, w3, w4, w5;
  int refl;  // spt_refl
  float ip;  // 1/pmax, correctly rounded on the host (the RR reweighting f * (1/p) of :451)
  float ex, ey, ez, pmax;
  float cx, cy, cz;
  // Russian roulette as integers (host): INT_MIN when pmax == 0 (RR always applies, :448), else
  // ceil(pmax * 2^16) (0 for pmax <= 0, 2^16 for pmax >= 1), so that `u16 * 2^-16 < pmax` (:449,
  // with alive only for pmax > 0) is `(int)u16 < rr_t`: the same decision with no conversion
  int32_t rr_t;
};
static_assert(sizeof(DevPrim) == 64, "DevPrim layout");

// Intersection geometry, grouped by kind (XY, XZ, YZ rects, then spheres; index order inside a
// group) and read through the constant address space so every load in the intersect loop is a
// wave-uniform s_load (scalar cache broadcast) — never a per-lane memory access.
// rect bounds as |a - ma| <= ha, |b - mb| <= hb (c_rect_mid in the oracle): per axis one
// subtract + one compare, each reading a single SGPR (the VALU constant-bus limit on gfx950).
struct GeoRect { float k, ma, ha, mb, hb; int idx; int pad0, pad1; };   // 32 B
struct GeoSph { float px, py, pz, rad2; int idx; int wide, pad1, pad2; };  // 32 B
// fp64 geometry of a wide sphere (radius >= SPT_WIDE_SPHERE_RADIUS: the 1e5 walls of the classic
// smallpt box), tested in double (oracle c_sphere_wide).
struct GeoSphD { double px, py, pz, rad2; };
// A rect test of the contract (oracle c_test): a parallel pair (k0 < k1, shared bounds) or a single
// (k0 == k1, pos0 == pos1); pos* are grouped positions in rect[].
struct GeoTest { float k0, k1, ma, ha, mb, hb; int pos0, pos1; };      // 32 B
struct SceneGeo {
  int n_xy, n_xz, n_yz, n_sph;
  int n_txy, n_txz, n_tyz, n_sph_wide;  // rect tests per kind; wide spheres = the last n_sph_wide
  // contract v5's room (oracle c_find_room): its three pair tests follow the per-kind lists in
  // test[] (XY, XZ, YZ); box = mid, half + 2^-8 for x, y, z
  int has_room, n_box, pad_[2];  // n_box: boxes of contract v6 (their tests follow the room's)
  float pad2_[8];
  GeoRect rect[kMaxPrims];  // [0,n_xy) XY, [n_xy, n_xy+n_xz) XZ, then YZ
  GeoSph sph[kMaxPrims];
  GeoSphD sphd[kMaxPrims];
  GeoTest test[kMaxPrims];  // [0,n_txy) XY, then XZ, then YZ (room tests excluded), then the room
};

struct KParams {  // in device memory, read through a laundered constant-space pointer
  const DevPrim* prims;
  const SceneGeo* geo;
  int n_prims;
  float cam[12];  // origin, lower_left_corner, horizontal, vertical
  int width, height, spp;  // spp: the whole image's sample count (fix_scale), not the launch's
  // the launch's sample window [s_base, s_base + s_count) of those spp samples (s_lim = its end):
  // one-shot renders launch [0, spp), a film pass (spt_film.hip) any window
  uint32_t s_base, s_count, s_lim;
  uint32_t seed;
  float nee_prob;
  int rr_depth, max_depth, light_id;
  float lx0, ldx, lz0, ldz, ly, larea;
  int light_mode;
  uint32_t ldxi, ldzi;
  int tile_rows, shard_index, shard_count;
  int chunk, n_local_pix;
  uint32_t n_units;
  // n / d = (n * m) >> sh for every n < 2^31 (Granlund-Montgomery, host-computed): the refill's
  // divisions by n_local_pix, width and tile_rows without the ~25-instruction integer divide.
  uint32_t m_npix, sh_npix, m_w, sh_w, m_tile, sh_tile;
  // Guided grabs (small launches only, sh_guided < 32): a wave takes min(kGrab, max(units its
  // lanes need, kGrabMin, left >> sh_guided)) units per queue atomic, left = units not yet handed
  // out, so no wave hoards a full pool while the queue runs dry. sh_guided = 32: always kGrab.
  uint32_t sh_guided;
  // young blocks (SPT_YOUNG_CUT): blockIdx >= young_block take no new pool once the queue is at
  // young_cut; young_block = UINT32_MAX: off
  uint32_t young_block, young_cut;
  uint32_t scr_k, scr_q;  // pixel-order spreading of the units: K = 2^scr_k, scr_q = npix / K
  float inv_spp, inv_w, inv_h;
  float fix_scale;  // inv_spp * 2^31 (fix31)
  // camera of contract v5 (jitter_f): Au, Av, Cu = Au 2^-16, Cv = Av 2^-16, L = llc - origin per axis
  float cam_au[3], cam_av[3], cam_cu[3], cam_cv[3], cam_l[3];
  // light sample of contract v5 (oracle c_wrap_sample): GLIBC_WRAP with dx = 2^a odd, 1 <= a <= 24:
  // x0 - 1 + (r >> (7 + a)) 2^(a - 24); else (lattice 0) the rounds-1-4 wrapped multiply
  int lx_lattice, lz_lattice;
  uint32_t lx_shift, lz_shift;
  float lx_scale, lz_scale, lx0m1, lz0m1;
  // Shadow-ray specialisation: when the light is black (c == 0, HEAD :294) a path that reaches it
  // always ends there (RR with p == 0, :448), so the NEE test only needs "is the nearest hit the
  // light" — an occlusion query without id bookkeeping.
  int light_black, light_kind, light_pos;
  int scatter_uniform;  // SPT_FLAG_UNIFORM_SCATTER
  int leak_end;         // contract v6: a leaked path ends at its first miss (host leak_end_of)
  uint32_t steal_min;   // SPT_STEAL_MIN or, for a short launch, SPT_STEAL_MIN_SMALL
  // Sphere NEE kernel: vertices above early_y0 (every sphere's top + 1) in the HEAD room resolve
  // their light-accepted shadow rays early (early_room_proven); +inf when the host cannot prove it
  float early_y0;
  // The uploaded-geometry HEAD-topology NEE kernel's early resolve (early_geo_proven): per box, a
  // vertex at or above eb_top[b] or with sgn * x[axis] <= eb_bnd[b] (axis x, or z where eb_z[b]) has
  // a shadow segment that cannot meet the box; eb_top = +inf and eb_bnd = -inf: no clause (the
  // host could not prove one, or the predicate is off)
  float eb_top[2], eb_sgn[2], eb_bnd[2];
  uint32_t eb_z[2];
  // ... and its room clause (early_geo_setup): the vertex in the room's box below the light plane,
  // per axis (bits(v) - er_lo) <= er_span on the float bits (HEAD: x in [1, 99], y in [0, 81.5),
  // z in [0, 170], the literal early_room_ok); er_lo = 0, er_span = 0 with no clause
  uint32_t er_lo[3], er_span[3];
  uint32_t ul_ybits;  // the room-literal light-uploaded kernel's y bound: bits(y) < bits(y_L)
  int unit_dirs;  // oracle c_unit_dirs: the scene has a sphere or a REFR primitive
  float nee_c;    // light_area / pi rounded once (the free-scale NEE weight, nee_weight)
  unsigned long long* accum;  // [n_local_pix][3] 1.31 fixed point (stolen ranges; every unit without slots)
  unsigned long long* slots;  // [n_units][3] one owner store per unit, unit order (unit slots)
  uint32_t* queue;            // [0] = next unit
  unsigned long long* stats;  // [8]
  // A launch over a pixel list (an adaptive film's pass, spt_film.hip): local pixel lp of the launch
  // is the real local pixel pix_list[lp] (ascending, row-tile shard order), n_local_pix = the list's
  // length. nullptr: the launch's pixels are the shard's, as ever. Read in pixel_terms() only.
  const uint32_t* pix_list;
  // A guide launch (guide_kernel; appended, so no offset the render kernels read moves): the guide's
  // records int64[n_local_pix][8] and log2 of the lanes that share a pixel.
  long long* guide_rec;
  uint32_t guide_kshift;
  // A light-guide launch (light_guide_kernel; appended likewise): the records int64[n_local_pix][4] and
  // log2 of the lanes that share a pixel. It reads the light's fields above (light_id, lx0 .. larea,
  // nee_c) as a render does.
  uint32_t light_kshift;
  long long* light_rec;
};

}  // namespace spt

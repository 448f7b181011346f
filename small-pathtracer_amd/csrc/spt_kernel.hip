// spt_kernel.hip — MI355X (gfx950) render kernel for the smallpt per-pixel sampling loop. The file
// holds render_kernel with what only the render loop uses (lane states, the early-resolve predicates,
// the NEE weight, the pool helpers), finalize_slots_kernel, the two tables of render_kernel's
// instantiations and the three launchers the host side needs (the end of the file). The trace it
// calls is spt_trace.h, shared with the guide kernel (spt_guide.hip). The C ABI of include/spt.h is
// spt_dispatch.cpp (scene grouping, kernel choice, launch sizing: no HIP) and spt_context.cpp
// (contexts and launches).
//
// Replaces the reference's smallpt.cpp:528-542 (pixel x sample loop) and :419-480
// (recursive radiance()) with one persistent-lane kernel:
//   * one lane = one pixel-sample path at a time; radiance()'s recursion is an iterative bounce
//     loop in registers (T = throughput, L = radiance so far);
//   * work units = (pixel, chunk of samples); a wave pulls units from a global atomic queue and
//     hands them to its idle lanes with a ballot + mbcnt prefix sum, so lanes whose paths end by
//     Russian roulette / light hits immediately start the next sample; once the queue is dry an
//     idle lane takes the upper half of a busy lane's unstarted samples (in-wave stealing);
//   * the scene (<= 64 primitives) never costs a per-lane HBM read in intersect() :323-335: the
//     reference's HEAD scene is compiled into the instruction stream, other scenes' rect tests are
//     staged once per block into LDS (broadcast reads) and their spheres read with wave-uniform
//     scalar loads; the per-lane lookups of the hit primitive (material) come from LDS;
//   * a NEE shadow ray is traced only if the light's own test accepts it; in the reference's room
//     the HEAD NEE kernel resolves most of those at once, where an exact geometric predicate
//     proves that nothing lies between the vertex and the light (early_nee_proven);
//   * Philox4x32-7 counter RNG keyed by (seed; pixel, sample, vertex, stream);
//   * per-pixel accumulation in 1.31 fixed point with 64-bit integer atomics: exact, independent
//     of unit size, lane order, queue order, stealing and GPU count.
#include <hip/hip_runtime.h>

#include <utility>

#include "../../include/spt.h"
#include "spt_device.h"
#include "spt_cornell.h"
#include "spt_diag.h"
#include "spt_kparams.h"
#include "spt_variants.h"
#include "spt_launch.h"
#include "spt_trace.h"

#define SPT_STR_(x) #x
#define SPT_XSTR(x) SPT_STR_(x)

namespace spt {

// Lane states of the render loop (render_kernel). The generating states are Cam, Cos, Spec in this
// order, and the states that hold a ray are ls >= kPath, in both numberings:
//   GEN_FIRST: Cam 0, Cos 1, Spec 2, Idle 3, so that the generate guard is ONE compare with an inline
//   constant, ls < kIdle, and the camera lanes' mask one subtract (ls - 1);
//   else Idle 0, Cam 1, Cos 2, Spec 3 (guard: ls - kCam < 3u, an add and a compare), the numbering of
//   the variants that the other one costs registers (KernelTraits::kGenStatesFirst).
template <bool GEN_FIRST>
struct LaneStates {
  static constexpr uint32_t kCam = GEN_FIRST ? 0 : 1;   // next: a camera ray (a new sample; retire the unit at s_end)
  static constexpr uint32_t kCos = kCam + 1;            // next: the cosine continuation of the last vertex
  static constexpr uint32_t kSpec = kCam + 2;           // next: a path ray whose direction is already set (SPEC/REFR)
  static constexpr uint32_t kIdle = GEN_FIRST ? 3 : 0;  // no work unit
  static constexpr uint32_t kPath = 4;    // a path ray is set: trace it, shade its vertex
  static constexpr uint32_t kShadow = 5;  // a NEE shadow ray toward the light is set: trace, resolve
  static constexpr uint32_t kTerm = 6;    // the path ended at this vertex (within an iteration)
  static constexpr uint32_t kEarly = 7;   // a NEE shadow ray proven to reach the light (early_nee_proven)
  // the lanes that generate a ray (kCam, kCos, kSpec)
  static __device__ __forceinline__ bool generates(uint32_t ls) {
    if constexpr (GEN_FIRST) return ls < kIdle;
    else return ls - kCam < 3u;
  }
};
// Exit condition every wave reaches even if a path never terminated: a C3 wave runs ~4e3
// iterations and a 1-GPU C5 wave ~3e6; stats[0] counts waves that hit the cap.
constexpr uint32_t kMaxWaveIters = 1u << 26;

template <class CF> __device__ __forceinline__ int light_id_of(const SPT_CONST KParams* P) {
  if constexpr (CF::LREF == 1) return kRefLightId; else return P->light_id;
}
// The light's id in the kernel's primitive numbering: its grouped position in the HEAD kernels
// (s_prims is loaded by slot there, cornell_slot; intersect_scene), its prims[] index elsewhere
template <class TP, class CF> __device__ __forceinline__ int light_slot_of(const SPT_CONST KParams* P) {
  if constexpr (TP::CONSTGEO) return cornell_slot(kCornellLightPos, KernelTraits<TP, CF>::kAxisBits);
  else return light_id_of<CF>(P);
}
template <class CF> __device__ __forceinline__ int rr_depth_of(const SPT_CONST KParams* P) {
  if constexpr (CF::LREF == 1) return kRefRrDepth; else return P->rr_depth;
}
// The plane axis of the hit at grouped position pos (0 <= pos <= 63) in the literal HEAD kernels, as
// two lane masks (spt_device.h, mask_lt): xy = pos is an XY rect, xyxz = an XY or an XZ one. What the
// axis picks -- o_a, d_a, 1/d_a, the NEE weight's |dl_a| -- is then two full-rate bit selects, and the
// normal three ands, where the compares' SGPR-pair masks fed half-rate VOP3 selects.
// AXB (KernelTraits::kAxisBits): pos is a slot with the kind in its bits (cornell_slot), and the masks
// are yz = bit 5 and xz = bit 4 spread over the word, one v_bfe_i32 each where mask_lt is a subtract and
// a shift. The picks and the normal keep their instruction counts with the masks' roles restated: x
// under yz, else y under xz, else z. (Slot 63, a miss of the kMissEntry kernels, sets both: nothing
// reads what that lane picks.)
struct AxisMasks { uint32_t xy, xyxz, yz, xz; };  // (AXB: yz, xz; else xy, xyxz)
template <bool AXB>
__device__ __forceinline__ AxisMasks axis_masks(int pos) {
  if constexpr (AXB) return AxisMasks{0, 0, bit_mask<kAxisBitYZ>((uint32_t)pos), bit_mask<kAxisBitXZ>((uint32_t)pos)};
  else return AxisMasks{mask_lt<kCornellNXY>(pos), mask_lt<kCornellNXY + kCornellNXZ>(pos), 0, 0};
}
template <bool AXB>
__device__ __forceinline__ float axis_pick(AxisMasks m, float z, float y, float x) {
  if constexpr (AXB) return bself(m.yz, x, bself(m.xz, y, z));
  else return bself(m.xy, z, bself(m.xyxz, y, x));
}

// An event counter takes the lanes of mask m, at a convergent point of the render loop. Wave-uniform
// (c in an SGPR): the mask's population. Per lane (KernelTraits::kLaneEvents; c in a VGPR, summed over
// the wave at the end): ONE v_addc_co_u32 with the mask as its carry-in (LLVM spells c + (b ? 1 : 0)
// as a v_cndmask and a v_add).
template <bool LANE>
__device__ __forceinline__ void count_lanes(uint32_t& c, uint64_t m) {
  if constexpr (LANE) asm("v_addc_co_u32_e64 %0, vcc, 0, %0, %1" : "+v"(c) : "s"(m) : "vcc");
  else c += (uint32_t)__popcll(m);
}

// Early NEE resolve (the HEAD NEE kernel: compile-time HEAD geometry, the reference's light
// constants, black light). A shadow ray (x, dl) whose light test accepts (t_L, crossing
// x_L = 50 + a) cannot meet any primitive before the light when x satisfies the conditions below,
// so intersect() (:323-335, oracle c_intersect) would return the light with t = t_L, bit for bit:
// the lane resolves it in the iteration that sampled it instead of tracing it in the next one.
//   * room: 1 <= x <= 99, 0 <= z <= 170, 0 <= y < 81.5. The room's slab candidate is then its exit
//     wall, never the one the vertex lies on (a vertex rounded outside its wall keeps its self-hit:
//     traced), and that wall lies >= 31 units beyond the light crossing in x (the light spans x
//     32..68), >= 63 in z (z 63..96); the ceiling is 0.1 above the light plane.
//   * short box (x, z in [63, 88], y <= 25): y >= 25 (the ray rises: the slab's y interval ends at
//     t <= 0, so the box's candidate is negative), or x <= 63 and x_L < 63 (x stays below 63 along
//     the segment but at its start; a vertex exactly on the x = 63 face has t = -2^-149 there;
//     x_L < 63 always holds below y = 25, see early_nee_proven).
//   * tall box (x in [12, 42], z in [32, 62], y <= 50): y >= 50, or z >= 62 (z stays at or above 62
//     along the segment -- the light's z >= 63 -- and reaches 62 only at t <= 0: the box's z slab
//     ends behind the origin). Round 4: >= and <= where rounds 2-3 kept a 0.01 margin; a vertex on
//     a box face often lies exactly on its plane: +8.5 % resolved shadow rays, 0 contradictions.
// Faces crossed beyond t_L fail their y bounds (y > 81.5 there) or lose to the light on t. The
// oracle restates the predicate and checks it against its own intersect() (spt_oracle_proof_*,
// tests/test_oracle.py); it covers ~77 % of the shadow rays that reach the light at C3.
// (Compares on float bits: every bound here is a positive literal, so a coordinate with the sign
// bit set -- negative, or -0.0 -- compares above it, fails and is traced; no signed zero reaches a
// bound. The bounds that come from a scene are early_geo_setup's, which takes a zero as +0.0.)
__device__ __forceinline__ int early_room_ok(f3 x) {
  return (int)(__float_as_uint(x.x) - __float_as_uint(1.0f) <=
               __float_as_uint(99.0f) - __float_as_uint(1.0f)) &
         (int)(__float_as_uint(x.z) <= __float_as_uint(170.0f)) &
         (int)(__float_as_uint(x.y) < __float_as_uint(81.5f));  // +0 <= v: no sign bit
}
// Sphere scenes in the HEAD room (the sphere NEE kernel, C5): with every sphere's top below
// y0 - 1, a vertex above y0 whose shadow ray goes up (dl.y > 0) cannot meet a sphere for t > 0:
// the real intersections lie at t <= -1, and the fp32 quadratic's rounding (|det| error < 0.02
// for |op| < 200) cannot lift a root above the 2e-3 epsilon. The room as above.
__device__ __forceinline__ bool early_room_proven(f3 x, float y0) {
  return (early_room_ok(x) & (int)(x.y > y0)) != 0;
}
// (Round 4: the short box's "x_L < 63" is implied below y = 25: the reference's wrapped light
// samples lie at x in [31, 33), and the crossing of y = 81.5 lies within 0.1 / (81.6 - y) < 0.0018
// of the way back to the vertex, so x_L < 33.2 there. One compare fewer; the same predicate.)
// The same proof for an edited rect[] of the HEAD topology (the uploaded-geometry kernels; round 6:
// the room and the light may be edited as well): the vertex in the room's box below the light plane
// (early_room_ok_k: the room's exit face lies beyond the light crossing, the host checks the light's
// margins to the walls and the ceiling), each box standing on the floor >= 0.5 below the light
// plane with a clause the host picks from the reference's wrapped light samples (x in [31, 33),
// z in [62, 64), y 81.6; the light plane at most 81.5, so the crossing lies on the segment to the
// sample): a box with x0 >= 33 is clear for a vertex with x <= x0 (the segment to the light stays at
// x <= x0) -- the HEAD short box's clause --, x1 <= 31 for x >= x1, z0 >= 64 for z <= z0, z1 <= 62
// for z >= z1 (the HEAD tall box's); and every box for a vertex at or above its top.
// The oracle restates the choice (c_find_early_clauses) and checks every claim (test_oracle.py).
// The room clause of an edited scene (room and light from KParams, host early_geo_setup): the same
// compares as early_room_ok with the bounds in SGPRs.
__device__ __forceinline__ int early_room_ok_k(f3 x, const SPT_CONST KParams* P) {
  return (int)(__float_as_uint(x.x) - P->er_lo[0] <= P->er_span[0]) &
         (int)(__float_as_uint(x.y) - P->er_lo[1] <= P->er_span[1]) &
         (int)(__float_as_uint(x.z) - P->er_lo[2] <= P->er_span[2]);
}
// ROOM: 0 = the literal HEAD room and light plane (early_room_ok; the boxes-only-uploaded kernels),
// 1 = the literal room with the light plane's bound from KParams (UPLIGHT), 2 = everything from
// KParams (the uploaded-geometry kernels)
template <int ROOM>
__device__ __forceinline__ bool early_geo_proven(f3 x, const SPT_CONST KParams* P) {
  int ok;
  if constexpr (ROOM == 0) {
    ok = early_room_ok(x);
  } else if constexpr (ROOM == 1) {
    ok = (int)(__float_as_uint(x.x) - __float_as_uint(1.0f) <= __float_as_uint(99.0f) - __float_as_uint(1.0f)) &
         (int)(__float_as_uint(x.z) <= __float_as_uint(170.0f)) & (int)(__float_as_uint(x.y) < P->ul_ybits);
  } else {
    ok = early_room_ok_k(x, P);
  }
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const float v = P->eb_z[b] ? x.z : x.x;
    ok &= (int)(x.y >= P->eb_top[b]) | (int)(v * P->eb_sgn[b] <= P->eb_bnd[b]);
  }
  return ok != 0;
}
__device__ __forceinline__ bool early_nee_proven(f3 x) {
  const int room = early_room_ok(x);
  const int short_box = (int)(x.y >= 25.0f) | (int)(x.x <= 63.0f);
  const int tall_box = (int)(x.y >= 50.0f) | (int)(x.z >= 62.0f);
  return (room & short_box & tall_box) != 0;
}

// Diagnostic build (-DSPT_REGION_STATS): per code region, wave executions and active lanes,
// counted with wave-uniform SALU ballots and flushed once per wave to stats[8 + 2*region].
#ifdef SPT_REGION_STATS
constexpr int kRegions = 10;
#define SPT_REGION(R) (reg_flags |= 1u << (R))  // per lane; ballot-counted at the loop end
#else
#define SPT_REGION(R) \
  do {                \
  } while (0)
#endif

// n / d of the contract where it only weights a sample (the NEE pdf; oracle c_div): n * rcp_nr(d).
__device__ __forceinline__ float div_nr(float n, float d) { return n * rcp_nr(d); }

// PDF_inverse * BRDF of :471-472 for a NEE shadow ray (x, d) whose nearest hit is the light at t
// (oracle c_nee_weight). Unit directions: |area d.y / t^2| |d.nl / pi| as written. Free-scale: d is
// light_vec (:367) itself, not normalised; with dl = d/|d| and the distance t|d| the same quantity
// is (area/pi) |d.y| |d.nl| / (t^2 (d.d)^2): no square root, and the normalize of the shadow
// direction (18 VALU per vertex) is gone.
__device__ __forceinline__ float nee_weight(bool unit, f3 d, f3 nl, float t, float larea, float nee_c) {
  if (unit) {
    const float pdf = fabsf(div_nr(larea * d.y, t * t));            // :471
    const float brdf = fabsf(dot3(d, nl) * 0.318309886183790672f);  // :472
    return pdf * brdf;
  }
  const float num = fabsf(d.y) * fabsf(dot3(d, nl));
  const float vv = dot3(d, d);
  return (num * nee_c) * rcp_nr((t * t) * (vv * vv));
}
constexpr float kRefNeeC = (float)(1296.0 / 3.14159265358979323846);  // kRefLarea / pi

// The camera ray of contract v5 (oracle c_path, :533-536): per component c
//   v_c = fma(Fv, Cv_c, fma(Fu, Cu_c, P_c)),  Fu = 2^23 + ju, Fv = 2^23 + jv,
// with ju, jv the 16-bit jitter draws (the float with bits 0x4B000000 | j is 2^23 + j exactly),
// Cu_c = hor_c (1/w) 2^-16, Cv_c = ver_c (1/h) 2^-16 per launch and the per-pixel
// P_c = fma(Au_c, fx, fma(Av_c, fy, llc_c - origin_c)), Au_c = hor_c (1/w), Av_c = ver_c (1/h),
// fx = (x - 0.5) - 128, fy = (h - y - 1 - 0.5) - 128 (the -128 cancels 2^23 2^-16 in Fu Cu).
// The axis-aligned camera kernels keep P_x, P_y per work unit: one fma per component per ray
// (rounds 1-4: the jitter sum, a scale, an fma and a subtract per component). Fu, Fv are jitter_f
// (spt_device.h).

// Orders one wave's own LDS accesses: what its lanes wrote before this point is what any of its
// lanes reads after it. No instruction on gfx950 (a wave's LDS operations complete in order); it
// binds the compiler.
__device__ __forceinline__ void wave_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t lane_rank(uint64_t mask) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                   __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// A unit index -> its (spread) local pixel, as the refill maps it (chunk-major units, pixel order
// spread by scr_k).
__device__ __forceinline__ uint32_t unit_pixel(const SPT_CONST KParams* Q, uint32_t u) {
  const uint32_t r = u - div_magic(u, Q->m_npix, Q->sh_npix) * (uint32_t)Q->n_local_pix;
  return (r & ((1u << Q->scr_k) - 1u)) * Q->scr_q + (r >> Q->scr_k);
}

// One lane = one pixel-sample path at a time, and every iteration traces exactly ONE ray per lane
// with the same nearest-hit loop (intersect :323-335): either the path ray toward the next vertex
// or, after a NEE event whose light sample passes light_accepts(), the shadow ray of :466. The
// wave never runs an occlusion test for lanes that have none (the light pre-test rejects ~75% of
// the NEE samples at HEAD); a lane whose shadow ray is pending simply skips the ray-generation and
// shading blocks of that iteration. Per lane the arithmetic is exactly the counter-mode contract
// (oracle c_path): only the schedule differs.
//   iteration: [refill idle lanes] -> [generate: cosine continuation and camera ray, one Philox
//   call, shared normalize] -> [trace] -> [resolve a shadow ray] -> [shade a vertex: RR, NEE
//   pre-test] -> [path end: accumulate; retire the unit after its last sample].
// The lane state is one VGPR word (kSt*) and the small blocks are branch-free: the loop is bound
// by instruction issue, and LLVM's exec-mask bookkeeping for loop-carried booleans and short
// branches was SALU work on the CU's single scalar unit.
template <class TP, class CF, bool LIST = false>
// SGPRs capped at 80 (SPT_NUM_SGPR, spt_trace.h: the cap, and why a CU then admits 8 blocks)
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_num_sgpr(SPT_NUM_SGPR)))
// The sphere kernels and the estimator-specialised rect kernels allocate for 8 waves/SIMD
// explicitly: the sphere NEE kernel otherwise takes 65 VGPRs (7 waves), the HEAD NEE kernel 65 with
// the round-2 Philox key (philox_pixel_key), the uploaded-geometry HEAD-topology ones 65; with the
// hint all fit 64 with no spills
__attribute__((amdgpu_waves_per_eu((TP::SPH && !TP::MAT && !TP::WIDE) || (!TP::SPH && !TP::MAT && CF::NEE >= 0) ? 8 : 1)))
render_kernel(const KParams* __restrict__ Pg) {
  __shared__ DevPrim s_prims[kMaxPrims];
  __shared__ int s_pos2idx[kMaxPrims];  // grouped position -> primitive index
  __shared__ GeoTest s_test[(TP::CONSTGEO && !TP::UPBOX) || TP::WIDE ? 1 : kMaxPrims];
  // Pending REFR refraction children (:494-495 at depth <= 2), two per lane at most (MAT only):
  // o, d, T, depth, branch.
  struct Node { float o[3], d[3], T[3]; int depth; uint32_t branch; };
  __shared__ Node s_stack[TP::MAT ? kBlock * 2 : 1];
  // Sphere vertices shaded, per wave (SPH only). They are counted inside the divergent shading
  // block, where a wave-uniform register would turn per-lane (a ballot there sees only the active
  // lanes); one LDS add per wave (the atomic optimizer folds the lanes) keeps it out of the VGPRs.
  // (The shaded primitive's kind is told apart there by three rectangle compares; a sphere is what
  // is left, so there is no compare of its own to take to a convergent ballot.)
  __shared__ uint32_t s_nsph[TP::SPH ? kBlock / 64 : 1];
  if (TP::SPH && threadIdx.x < kBlock / 64) s_nsph[threadIdx.x] = 0;
  // The set-up of the units of each wave's pool (spt_kparams.h, SPT_POOL_LDS): 64 entries per wave,
  // written and read by that wave alone. The generic kernels keep the per-lane set-up: the REFR
  // stack fills their LDS (5 blocks per CU), and 8 KB more would cost them a block.
  constexpr bool kPoolLds = kPoolLdsBuild && !TP::MAT;
  __shared__ PoolEntryA s_pool_a[kPoolLds ? kBlock : 1];
  __shared__ PoolEntryB s_pool_b[kPoolLds ? kBlock : 1];
  // The block's staging. guide_kernel (spt_guide.hip) pastes this loop, and its guide_vertex and
  // guide_chain_step restate the two blocks below that name them: the inline forms stay here because
  // every shared function tried moved these kernels' listings (staging: all 52 instantiations; the
  // normals: the 10 sphere ones by up to 17 lines; the hit point and reflect/refract: the generic and
  // wide ones by 15 to 17, the wide one at its 80-VGPR limit). tools/isa_same.py is the check.
  {
    const SPT_CONST KParams* P = cptr(Pg);
    const SPT_CONST SceneGeo* G = cptr(P->geo);
    const int nrect = G->n_xy + G->n_xz + G->n_yz;
    for (int i = threadIdx.x; i < P->n_prims; i += kBlock) {
      // HEAD geometry (every primitive a rectangle): s_prims by the grouped position's slot
      s_prims[TP::CONSTGEO ? cornell_slot(i, KernelTraits<TP, CF>::kAxisBits) : i] =
          P->prims[TP::CONSTGEO ? G->rect[i].idx : i];
      s_pos2idx[i] = i < nrect ? G->rect[i].idx : G->sph[i - nrect].idx;
      if ((!TP::CONSTGEO || TP::UPBOX) && !TP::WIDE && i < G->n_txy + G->n_txz + G->n_tyz + 3 * G->has_room + 3 * G->n_box) {
        const SPT_CONST GeoTest& q = G->test[i];
        // (the uploaded boxes of the room-literal kernels: their positions as the kernel's slots)
        constexpr bool kSlots = TP::CONSTGEO && KernelTraits<TP, CF>::kAxisBits;
        s_test[i] = GeoTest{q.k0, q.k1, q.ma, q.ha, q.mb, q.hb, cornell_slot(q.pos0, kSlots), cornell_slot(q.pos1, kSlots)};
      }
    }
    // the entry a miss reads (kMissEntry): no emission, so its T * e is the +0 prim 0's was
    if (KernelTraits<TP, CF>::kMissEntry && threadIdx.x == 63) s_prims[63] = DevPrim{};
  }
  __syncthreads();

  const uint32_t lane = __lane_id();
  using St = LaneStates<KernelTraits<TP, CF>::kGenStatesFirst>;
  constexpr uint32_t kStIdle = St::kIdle, kStCam = St::kCam, kStCos = St::kCos, kStSpec = St::kSpec,
                     kStPath = St::kPath, kStShadow = St::kShadow, kStTerm = St::kTerm, kStEarly = St::kEarly;
  // ---- per-lane state
  // The lane's state is ONE integer in a VGPR (kSt*), not a set of booleans: LLVM keeps loop-carried
  // booleans as 64-bit lane masks and merges each one at every join of the divergent blocks with an
  // s_andn2/s_and/s_or triple, and SALU issue bounds this loop (one scalar unit per CU; a marginal
  // SALU instruction costs ~3x a marginal VALU one here). A VGPR state is
  // written under exec and needs no merge.
  uint32_t ls = kStIdle;
  uint32_t branch = 0;    // path-tree position of a REFR split (counter word 2 bits 24+; MAT only)
  int sp = 0;             // pending refraction children in s_stack (MAT only)
  uint32_t lp = 0, s = 0, s_end = 0;
  PxKey pk = PxKey{0, 0, 0};  // Philox round-1/2 terms of the unit's pixel (philox_pixel_key)
  // dp1: vertices of the current path so far plus one (1 until its first) -- the Philox vertex
  // counter of the ray generated next, with no add per call
  int dp1 = 1, vid = 0;
  // camera raster terms of the unit's pixel, fx = (x - 0.5) - 128, fy = (h - y - 1 - 0.5) - 128;
  // the axis-aligned camera kernels hold P_x, P_y (jitter_f) here instead
  float fx = 0.0f, fy = 0.0f;
  float fz = 0.0f;  // CAMAX 2: P_z (fx, fy hold P_x, P_y)
  unsigned long long acc0 = 0, acc1 = 0, acc2 = 0;
  // o starts at the camera (the first ray of every sample is a camera ray; the path end resets it)
  f3 o = mk(cptr(Pg)->cam[0], cptr(Pg)->cam[1], cptr(Pg)->cam[2]);
  f3 d = mk(0, 0, 1), T = mk(1, 1, 1), L = mk(0, 0, 0), nl = mk(0, 1, 0);
  float w_nee = 0.0f;  // HEAD NEE kernel: the NEE weight of the lane's shadow ray, from its vertex
  u4 r = u4{0, 0, 0, 0};  // Philox words of the vertex the pending path ray leads to
  // ---- wave-uniform state
  // Camera and fixed-point constants of the axis-aligned camera kernels, loaded once and held in
  // SGPRs (each scalar reload in the loop is a wait for the wave).
  struct CamK { float o0, o1, o2, aux, avy, cux, cvy, lx, ly, lz, fs; };
  CamK ck{};
  if constexpr (CF::CAMAX == 1) {
    const SPT_CONST KParams* C = cptr(Pg);
    ck = CamK{C->cam[0], C->cam[1], C->cam[2], C->cam_au[0], C->cam_av[1], C->cam_cu[0],
              C->cam_cv[1], C->cam_l[0], C->cam_l[1], C->cam_l[2], C->fix_scale};
  }
  // CAMAX 2 (any camera): origin, Cu, Cv and the fixed-point scale in SGPRs (Au, Av, L are read at
  // the refill only)
  struct CamG { float o0, o1, o2, cu0, cu1, cu2, cv0, cv1, cv2, fs; };
  CamG cg{};
  if constexpr (CF::CAMAX == 2) {
    const SPT_CONST KParams* C = cptr(Pg);
    cg = CamG{C->cam[0], C->cam[1], C->cam[2], C->cam_cu[0], C->cam_cu[1], C->cam_cu[2],
              C->cam_cv[0], C->cam_cv[1], C->cam_cv[2], C->fix_scale};
  }
  // The terms of unit u (chunk-major units, pixel order spread by scr_k): its sample range, the
  // Philox key and the camera terms of its pixel. One lane's set-up of its own unit, or lane i's of
  // unit pool_next + i at the pool fill: the same arithmetic either way.
  auto unit_setup = [&](uint32_t u, uint32_t& us, uint32_t& us_end, PxKey& upk, float& ufx, float& ufy,
                        float& ufz) {
    const SPT_CONST KParams* Q = cptr(Pg);
    const uint32_t npix = (uint32_t)Q->n_local_pix;
    const uint32_t j = div_magic(u, Q->m_npix, Q->sh_npix);  // chunk-major
    uint32_t up = u - j * npix;
    // Spread the pixel order (scr_k > 0): unit pixel lp = b * K + a -> a * (npix / K) + b, so a
    // wave's run of consecutive units samples the whole image instead of one row segment, and
    // per-wave work varies less (the image does not change: every pixel-sample is still done
    // once and summed in integers)
    up = (up & ((1u << Q->scr_k) - 1u)) * Q->scr_q + (up >> Q->scr_k);
    us = Q->s_base + j * (uint32_t)Q->chunk;  // absolute sample index: the Philox sample word
    us_end = min(us + (uint32_t)Q->chunk, Q->s_lim);
    pixel_terms<LIST>(Q, up, upk, ufx, ufy);
    if constexpr (CF::CAMAX == 1) {  // the per-pixel P_x, P_y of the camera ray (jitter_f)
      ufx = fmaf(ck.aux, ufx, ck.lx);
      ufy = fmaf(ck.avy, ufy, ck.ly);
    } else if constexpr (CF::CAMAX == 2) {  // P_c = fma(Au_c, fx, fma(Av_c, fy, L_c)), c = x, y, z
      const float rx = ufx, ry = ufy;
      ufx = fmaf(Q->cam_au[0], rx, fmaf(Q->cam_av[0], ry, Q->cam_l[0]));
      ufy = fmaf(Q->cam_au[1], rx, fmaf(Q->cam_av[1], ry, Q->cam_l[1]));
      ufz = fmaf(Q->cam_au[2], rx, fmaf(Q->cam_av[2], ry, Q->cam_l[2]));
    }
  };
  // the wave's region of s_pool_a / s_pool_b starts at its first thread's index (wave-uniform)
  const uint32_t pool_lds = kPoolLds ? (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x & ~63u)) : 0u;
  uint32_t pool_next = 0, pool_end = 0, grab_at = 0;  // grab_at: the wave's last queue position
  bool exhausted = false, capped = false;  // capped: the runaway guard ended the wave
  // Wave-uniform event counters (SGPRs), fed by ballots at convergent points of the loop: per-lane
  // counters incremented inside the divergent blocks cost ~40 VGPRs of copies.
  // (vertices = path rays + NEE light hits: every path ray shades a vertex, hit or miss, and a
  // shadow ray that reaches the light shades the light's)
  // n_gen (kernels without SPEC/REFR): the path rays, counted as the lanes that generate one. Each
  // is a sample's camera ray or a cosine continuation, so the cosine rays are n_gen less the launch's
  // samples, taken off once at the end. The generic kernel counts n_path and n_cos themselves.
  uint32_t n_path = 0, n_cos = 0, n_gen = 0;
  // The events from the trace to the path end are counted the same way. That region runs under a
  // wave-uniform guard (some lane traces), not a divergent one, so its top level is convergent and a
  // counter updated there stays in an SGPR: each event's lane mask is a compare the region needs
  // anyway, taken by a ballot where it is final (s_and / s_bcnt1 / s_add, no VALU, no VGPR).
  //   n_miss:   path rays that hit nothing        n_hit:   traced shadow rays that reach the light
  //   n_shadow: shadow rays resolved (traced, and in the early-resolve kernels proven)
  //   n_early:  shadow rays proven to reach the light without a trace (stats[kStatShadowProven])
  // (Per lane in the kLaneEvents variants, spt_variants.h: the same masks at the same points, each
  // added to the lanes it holds, and the wave's lanes summed at the end.)
  uint32_t n_miss = 0, n_hit = 0, n_shadow = 0, n_early = 0;
  // What the variant's types imply (spt_variants.h, where the host reads the same values).
  using KT = KernelTraits<TP, CF>;
  static_assert(!TP::MAT || TP::SPH, "the generic kernels count their misses in the sphere shading branch");
  constexpr bool kNeeByIdentity = KT::kNeeByIdentity, kEarlyNee = KT::kEarlyNee,
                 kEarlySph = KT::kEarlySph, kEarlyGeo = KT::kEarlyGeo, kEarly = KT::kEarly,
                 kLaneEvents = KT::kLaneEvents;
  // NEE samples taken (the run-time estimator's kernels): per lane, incremented in place inside the
  // nested shading branches and summed once at the end. Its predicate (a DIFF vertex, the sample
  // drawn, the path alive) exists only there; carried to a convergent ballot it cost 3 VALU.
  uint32_t l_nee = 0;
#ifdef SPT_REGION_STATS
  uint32_t reg_exec[kRegions] = {}, reg_lanes[kRegions] = {};
  uint32_t reg_flags = 0;
#endif

#ifdef SPT_WAVE_TIMES  // diagnostic build: per-wave residency (100 MHz real-time counter)
  const unsigned long long wave_t0 = __builtin_amdgcn_s_memrealtime();
  uint32_t wave_iters = 0;
#endif
  // The loop's two exits share one scalar condition at the back edge. `left` counts the iterations
  // down to the runaway guard, in every iteration whatever the lanes hold: a wave whose paths never
  // end leaves after kMaxWaveIters with its work dropped (`capped`). A wave that finds no lane with
  // work sets left = 1 (`live` tells the two apart): it runs the rest of that iteration with every
  // block's lane mask empty and leaves at the same branch. (A lane-mask flag broken out of the
  // nested refill branch was built, inverted and re-tested in every iteration: ~7 SALU.)
  uint32_t left = kMaxWaveIters;
  // (The sphere kernel with the run-time estimator, at 64 VGPRs, spills one with the exit at the back
  // edge alone: it tests `live` after the refill as well and skips the empty pass.)
  constexpr bool kExitAtRefill = TP::SPH && !TP::MAT && CF::NEE < 0;
  bool live = true;  // wave-uniform: some lane holds work
  for (;;) {
    [[maybe_unused]] const uint32_t iter = kMaxWaveIters - left;  // (the diagnostic builds' count)
#ifdef SPT_WAVE_TIMES
    wave_iters = iter;
#endif
    const SPT_CONST KParams* P = cptr_at<0>(Pg, left);
    SPT_REGION(0);  // loop iteration
    // 1) (a unit is retired at the end of its last sample, in the path-end block below)
    // 2) refill idle lanes from the wave's pool (ballot + mbcnt prefix sum), pool from the queue.
    //    Everything up to the exit test runs only when some lane is idle: most iterations
    //    skip it with one wave-uniform branch (round 4: the loop-head bookkeeping was ~12 SALU per
    //    iteration when no lane needed a unit).
    const uint64_t need = __ballot(ls == kStIdle);
    if (need != 0) {
    // One pass, no loop: the idle lanes take what the pool holds, a fresh one if it is empty. When
    // the pool's last units do not serve every idle lane, the others take theirs from the next pool
    // in the next iteration. (A loop that served them at once carried the eight unit registers
    // through its phis: 16 v_mov per refill around a body that changes them for one lane in fifty.
    // Its second pass cannot be folded into one fetch after the loop either: a full pool's fill
    // writes all 64 entries, the ones that lanes served from the old pool have yet to read among
    // them.)
    if (!exhausted) {
      SPT_REGION(2);
      const SPT_CONST KParams* Q = cptr(Pg);
      if (pool_next >= pool_end) {
        uint32_t want = kGrab;
        if (Q->sh_guided < 32u) {
          const uint32_t rest = Q->n_units - min(grab_at, (uint32_t)Q->n_units);
          want = min(kGrab, max(max((uint32_t)__popcll(need), kGrabMin), rest >> Q->sh_guided));
        }
        // a young block's wave (SPT_YOUNG_CUT) past the cut takes no new pool: its lanes finish and
        // split what they hold (in-wave stealing) and the wave leaves
        bool open = true;  // the queue has a pool for this wave
        if (blockIdx.x >= Q->young_block) {
          uint32_t q = 0;
          if (lane == 0) q = __hip_atomic_load(Q->queue, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          q = __builtin_amdgcn_readfirstlane(q);
          open = q < Q->young_cut;
        }
        if (open) {
          uint32_t b = 0;
          if (lane == 0) b = atomicAdd(Q->queue, want);
          b = __builtin_amdgcn_readfirstlane(b);
          grab_at = b + want;
          open = b < Q->n_units;
          if (open) {
            pool_next = b;
            pool_end = min(b + want, Q->n_units);
            if constexpr (kPoolLds) {
              // Fill: lane i sets up unit b + i into entry (b + i) mod 64, all lanes at once (the
              // branch is wave-uniform). The region is the wave's own, so the order that matters is
              // this wave's: its earlier fetches before these writes, these writes before its later
              // fetches.
              wave_lds_order();
              const uint32_t u = b + lane;
              if (u < pool_end) {
                uint32_t us, us_end;
                PxKey upk;
                float ufx, ufy, ufz = 0.0f;
                unit_setup(u, us, us_end, upk, ufx, ufy, ufz);
                s_pool_a[pool_lds + (u & 63u)] = PoolEntryA{us, upk.qhi, upk.qlo, upk.lo};
                // (the third word: P_z where the kernel holds one, else the owner's lp = u | 2^31,
                // so that every kernel reads the entry as two whole 128-bit words)
                if constexpr (CF::CAMAX != 2) ufz = __uint_as_float(u | 0x80000000u);
                s_pool_b[pool_lds + (u & 63u)] = PoolEntryB{ufx, ufy, ufz, us_end};
              }
              wave_lds_order();
            }
          }
        }
        exhausted = !open;
      }
      if (!exhausted) {
        const uint32_t rank = lane_rank(need);
        const uint32_t avail = pool_end - pool_next;
        if (ls == kStIdle && rank < avail) {
          const uint32_t u = pool_next + rank;
          if constexpr (kPoolLds) {  // the entry the fill wrote for unit u
            const PoolEntryA ea = s_pool_a[pool_lds + (u & 63u)];
            const PoolEntryB eb = s_pool_b[pool_lds + (u & 63u)];
            s = ea.s;
            pk = PxKey{ea.qhi, ea.qlo, ea.lo};
            fx = eb.fx;
            fy = eb.fy;
            s_end = eb.s_end;
            // the owner keeps its unit index: the sums go to the unit's slot
            if constexpr (CF::CAMAX == 2) {
              fz = eb.fz;
              lp = u | 0x80000000u;
            } else {
              lp = __float_as_uint(eb.fz);
            }
          } else {
            unit_setup(u, s, s_end, pk, fx, fy, fz);
            lp = u | 0x80000000u;
          }
          ls = kStCam;
        }
        pool_next += min((uint32_t)__popcll(need), avail);
      }
    }
    // 2b) the queue is dry: an idle lane takes the upper half of a busy lane's unstarted samples
    //     (same pixel; each flushes its own sums and the accumulation is integer, so the image is
    //     unchanged). A wave's tail is then ~one path instead of ~one unit. Pairs are made by a
    //     scalar loop over the lane masks (readlane + a per-lane select), only in the tail.
    if (exhausted) {
      uint64_t idle = __ballot(ls == kStIdle);
      if (idle != 0) {
        const uint32_t cur = s + (ls == kStCam ? 0u : 1u);  // first unstarted sample
        // donors: lanes with more unstarted samples than the one they start next, and at least
        // steal_min of them (every stolen range flushes its own sums: memory-side atomics)
        const uint32_t smin = cptr(Pg)->steal_min;
        uint64_t dm = __ballot(ls != kStIdle && s_end > cur + (ls == kStCam ? 1u : 0u) &&
                               s_end >= cur + smin);
        while (idle != 0 && dm != 0) {
          const int il = __builtin_ctzll(idle), dl = __builtin_ctzll(dm);
          idle &= idle - 1;
          dm &= dm - 1;
          const uint32_t dcur = (uint32_t)__builtin_amdgcn_readlane((int)cur, dl);
          const uint32_t dend = (uint32_t)__builtin_amdgcn_readlane((int)s_end, dl);
          const uint32_t mid = dcur + (dend - dcur) / 2u;  // donor keeps [.., mid), taker [mid, dend)
          uint32_t d_lp = (uint32_t)__builtin_amdgcn_readlane((int)lp, dl);
          if (d_lp >> 31)  // an owner donor holds its unit index: the taker adds by pixel
            d_lp = unit_pixel(cptr(Pg), d_lp & 0x7FFFFFFFu);
          const uint32_t d_qhi = (uint32_t)__builtin_amdgcn_readlane((int)pk.qhi, dl);
          const uint32_t d_qlo = (uint32_t)__builtin_amdgcn_readlane((int)pk.qlo, dl);
          const uint32_t d_lo = (uint32_t)__builtin_amdgcn_readlane((int)pk.lo, dl);
          const float d_fx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(fx), dl));
          const float d_fy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(fy), dl));
          float d_fz = 0.0f;
          if constexpr (CF::CAMAX == 2) d_fz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(fz), dl));
          const bool tk = lane == (uint32_t)il;  // the taker
          s_end = tk ? dend : (lane == (uint32_t)dl ? mid : s_end);
          s = tk ? mid : s;
          lp = tk ? d_lp : lp;
          pk.qhi = tk ? d_qhi : pk.qhi;
          pk.qlo = tk ? d_qlo : pk.qlo;
          pk.lo = tk ? d_lo : pk.lo;
          fx = tk ? d_fx : fx;
          fy = tk ? d_fy : fy;
          if constexpr (CF::CAMAX == 2) fz = tk ? d_fz : fz;
          ls = tk ? kStCam : ls;
        }
      }
    }
    if (__ballot(ls != kStIdle) == 0) {  // no lane has work: the last iteration (the back edge)
      live = false;
      left = 1;
    }
    }
    if constexpr (kExitAtRefill) {
      if (!live) break;
    }
    // The generating lanes (the compare is the generate block's own), or in the generic kernel, whose
    // SPEC/REFR rays generate too, the cosine ones (a v_cmp of their own).
    if constexpr (TP::MAT) n_cos += (uint32_t)__popcll(__ballot(ls == kStCos));
    else n_gen += (uint32_t)__popcll(__ballot(St::generates(ls)));

    // 3) generate the path ray (kStCam, kStCos, kStSpec): the cosine continuation from the last
    //    vertex (random_scattering :337-347, its xi from that vertex's Philox words) or the camera
    //    ray of a new sample (:533-536, jitter from the low bytes of vertex 1's words), one Philox
    //    call for the vertex the ray leads to, one normalize for both. Both directions are computed
    //    for every generating lane and selected: a wave nearly always holds lanes of both kinds, so
    //    branches would save no VALU and cost their exec-mask SALU.
    if (St::generates(ls)) {
      [[maybe_unused]] const bool cam = ls == kStCam;
      if (ls != kStSpec) SPT_REGION(cam ? 3 : 8);
      const bool unit = unit_dirs_of<TP>(Pg);
      f3 v = cosine_vec<!TP::SPH, KT::kFunnelFloats>(nl, r.z, r.w, TP::MAT && cptr(Pg)->scatter_uniform != 0, unit);
      // the vertex this ray leads to: dp1 (1 for a new sample's camera ray)
      const uint32_t ctr2 = (uint32_t)dp1 | (TP::MAT ? branch << 24 : 0u);
      r = philox_px(pk, s, ctr2);
      {
        const SPT_CONST KParams* C = cptr_at<1>(Pg, left);
        f3 vc;
        const float Fu = jitter_f(r.x, r.y), Fv = jitter_f(r.z, r.w);
        if constexpr (CF::CAMAX == 1) {
          // the zero terms vanish exactly: fma(F, +-0, y) == y and fma(+-0, f, L) == L for the
          // nonzero y, L the host checks (cam_axis)
          vc = mk(fmaf(Fu, ck.cux, fx), fmaf(Fv, ck.cvy, fy), ck.lz);
        } else if constexpr (CF::CAMAX == 2) {  // the general form with P_c per unit
          vc = mk(fmaf(Fv, cg.cv0, fmaf(Fu, cg.cu0, fx)), fmaf(Fv, cg.cv1, fmaf(Fu, cg.cu1, fy)),
                  fmaf(Fv, cg.cv2, fmaf(Fu, cg.cu2, fz)));
        } else {
          float vv[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const float Pc = fmaf(C->cam_au[c], fx, fmaf(C->cam_av[c], fy, C->cam_l[c]));
            vv[c] = fmaf(Fv, C->cam_cv[c], fmaf(Fu, C->cam_cu[c], Pc));
          }
          vc = mk(vv[0], vv[1], vv[2]);
        }
        // (Round 22 priced the mask form at the compare form's 108 slots. With the camera lanes' state
        // 0 the mask is one subtract, and a VOP2 select takes an SGPR only as its first source, so the
        // compare form copied the axis-aligned camera's z into a VGPR in every iteration: the mask
        // form is one VALU fewer. The generic kernels, whose generating lanes may be kStSpec, and
        // the variants the mask costs a register keep the compare: KernelTraits::kCamMask.)
        if constexpr (KT::kCamMask) {
          // Without SPEC/REFR a generating lane is kStCam (0) or kStCos (1): ls - 1 is the camera
          // lanes' mask, and the select three bit selects (bsel: the select, bit for bit). The
          // axis-aligned camera's z is wave-uniform and goes in as the SGPR it is held in.
          static_assert(kStCam == 0 && kStCos == 1, "the camera lanes' mask is ls - 1");
          const uint32_t cm = keep(ls - 1u);
          float vz;
          if constexpr (CF::CAMAX == 1) vz = __uint_as_float(bsel_s(cm, __float_as_uint(ck.lz), __float_as_uint(v.z)));
          else vz = bself(cm, vc.z, v.z);
          v = mk(bself(cm, vc.x, v.x), bself(cm, vc.y, v.y), vz);  // o: set at the path end
        } else {
          v = mk(cam ? vc.x : v.x, cam ? vc.y : v.y, cam ? vc.z : v.z);
        }
      }
      const f3 dn = normalize_dir(v, unit);  // rsq_nr1 in the free-scale contract (v7)
      if constexpr (TP::MAT) {  // a SPEC/REFR direction is set already
        const bool kd = ls == kStSpec;
        d = mk(kd ? d.x : dn.x, kd ? d.y : dn.y, kd ? d.z : dn.z);
      } else {
        d = dn;
      }
      ls = kStPath;
    }
    // (opaque here: LLVM knows that a lane which skips the trace below is idle and would feed the
    // state's phi a zero of its own, a v_mov and a second register for the state word)
    ls = keep(ls);

    // Path rays: counted here by the generic kernel only (the others: n_gen, above).
    if constexpr (TP::MAT) n_path += (uint32_t)__popcll(__ballot(ls == kStPath));
    // (The generic kernels, kLaneEvents and at 78+ VGPRs, keep the forms they had: this ballot for the
    // shadow rays, and below the light hits and misses added per lane inside the divergent blocks.
    // With their counts at the region's top level they took 1 to 14 more VGPRs.)
    if constexpr (TP::MAT) n_shadow += (uint32_t)__popcll(__ballot(ls == kStShadow));
    // Everything from the trace to the path end runs when some lane holds a ray (kStPath or
    // kStShadow): a wave-uniform guard. Only idle lanes hold none here, and under the guard they run
    // the trace too, on their stale finite o and d: a VALU instruction costs the wave the same
    // whatever its lane mask. What they compute lands in locals (id, hit, hpos, inv); every block
    // below keeps its own state guard, which an idle lane fails, so it writes no loop-carried state;
    // and every event mask is and-ed with a state compare, so nothing of theirs is counted. In the
    // last, empty iteration no lane traces and the region is skipped as before.
    // (The kLaneEvents variants keep the divergent guard: the lanes that hold a ray.)
    const uint64_t raym = kLaneEvents ? 0 : __ballot(ls >= kStPath);  // the lanes that hold a ray
    if (kLaneEvents ? ls >= kStPath : raym != 0) {
      // 4) trace the lane's ray (path ray: hittingPoint :371-377; shadow ray: :466).
      if (ls >= kStPath) SPT_REGION(4);
#ifdef SPT_PROBE_SALU  // diagnostic build SPT_DIAG=3: N extra SALU per wave-iteration (issue cost)
      { uint32_t z_ = iter; asm volatile(".rept " SPT_XSTR(SPT_PROBE_SALU) "\n s_add_u32 %0, %0, 1\n .endr" : "+s"(z_)); }
#endif
#ifdef SPT_PROBE_VALU  // diagnostic build SPT_DIAG=4: N extra VALU per wave-iteration
      { float z_ = o.x; asm volatile(".rept " SPT_XSTR(SPT_PROBE_VALU) "\n v_add_f32 %0, 1.0, %0\n .endr" : "+v"(z_)); }
#endif
      const SPT_CONST SceneGeo* G = TP::CONSTGEO && !TP::UPLIGHT ? nullptr : cptr(P->geo);
      // intersect() leaves id untouched on a miss (:323-335): a shadow ray keeps its vertex's id. The
      // early-resolve HEAD kernel needs no vertex id: its light is black, so no vertex on the light
      // takes a NEE sample, and a missed shadow ray's id (prim 0's) is not the light's either way.
      int id = (!kEarlyNee && ls == kStShadow) ? vid : 0;
      float t = 0.0f, ia_hit = 0.0f;
      int hpos;
      f3 inv;  // 1/d per axis (rcp_nr), the trace's
      // (the early-resolve kernels trace a shadow ray only when the light accepts it: it never misses)
      bool hit = intersect_scene<TP, KT::kAxisBits, KT::kMissEntry>(G, rects_of<TP>(G), tests_of<TP>(G, s_test), G->sph, s_pos2idx, o, d,
                                     id, ia_hit, hpos, inv);
      // the hit's plane axis (the literal rect-only kernels), made once here for the shading too
      constexpr bool kAxb = KT::kAxisBits;
      [[maybe_unused]] const AxisMasks am = axis_masks<kAxb>(TP::CONSTGEO ? hpos : 0);
      if constexpr (TP::CONSTGEO) ia_hit = axis_pick<kAxb>(am, inv.z, inv.y, inv.x);

      // 5) resolve a shadow ray: the light is reached iff the nearest hit is the light (:467). Then
      //    the light is the next vertex (shaded in the common block below, T = T*f*weight); else the
      //    cosine sample follows (:468-469, T = T*f). The weight is computed for every shadow lane
      //    and applied as T*1 (exact) where the light is not reached: no branch. (The HEAD NEE
      //    kernel resolves in 5') below instead, after the shading block.)
      bool traced_shadow = ls == kStShadow;
      uint64_t tsm;  // the same as a lane mask
      // A lane is idle, kStPath or kStShadow here and, where nothing resolves before the shading, up
      // to the shade guard: the shadow lanes are the trace guard's lanes less the shade guard's, an
      // s_andn2 of two ballots the loop takes anyway (KernelTraits::kStateMasks). (With the shade
      // guard taken from the generate guard's ballot as well, whose lanes are the kStPath ones, the
      // listing gained an instruction: the mask came back to the lanes through a VGPR.)
      if constexpr (KT::kStateMasks) tsm = raym & ~__ballot(ls == kStPath);
      else tsm = __ballot(ls == kStShadow);
      if constexpr (kEarly) {
        // as a lane mask taken here: compared where 5') reads it, the state word of before the
        // shading stays live beside the new one (two v_mov per iteration)
        asm volatile("" : "+s"(tsm));
        traced_shadow = __builtin_amdgcn_inverse_ballot_w64(tsm);
      }
      // (a cosine-only kernel, CF::NEE == 0, never sets a shadow ray: no resolve block at all)
      if constexpr (!kEarly && CF::NEE != 0) {
      // Skipped as a whole, on the scalar mask, when no lane resolves: the light's slot is a scalar
      // load in the run-time estimator's kernels. (The kLaneEvents variants' guard is the block's own.)
      if (kLaneEvents || tsm != 0) {
      const SPT_CONST KParams* D = cptr_at<2>(Pg, left);
      bool lh = false;
      if constexpr (!TP::MAT) {
        // the light compare at the top level, where its mask and the shadow lanes' can be counted
        // (each mask the ballot of one compare, combined on the scalar unit: the ballot of a combined
        // boolean is built through a VGPR, a v_cndmask and a v_cmp each)
        lh = id == light_slot_of<TP, CF>(D);
        count_lanes<kLaneEvents>(n_shadow, tsm);
        count_lanes<kLaneEvents>(n_hit, tsm & __ballot(lh));
      }
      if (traced_shadow) {
        SPT_REGION(6);
        if constexpr (TP::MAT) {  // (in place, as they were: see above)
          lh = id == light_slot_of<TP, CF>(D);
          count_lanes<true>(n_hit, __ballot(lh));
        }
        if (lh) SPT_REGION(7);
        const float larea = CF::LREF == 1 ? kRefLarea : D->larea;
        const float nee_c = CF::LREF == 1 ? kRefNeeC : D->nee_c;
        t = hit_t<TP>(s_prims[id], hpos, o, d, ia_hit, G);  // the light's t (the winner's)
        const float w = lh ? nee_weight(unit_dirs_of<TP>(Pg), d, nl, t, larea, nee_c) : 1.0f;
        T = mk(T.x * w, T.y * w, T.z * w);  // T holds T*f of the shading vertex
        // A black light (HEAD :294) ends the path there by RR with p == 0 (:448-453) without a
        // random draw; anything else is shaded with that vertex's own Philox words.
        if (CF::BLACK != 1 && lh && !(hit && s_prims[id].pmax == 0.0f))
          r = philox_px(pk, s, (uint32_t)dp1 | (TP::MAT ? branch << 24 : 0u));
        ls = lh ? kStPath : kStCos;
      }
      }
      }

      // The light compare on the trace's final id, once for the whole iteration (kStateMasks): the
      // shading's NEE candidates and the resolve's light hits read the same mask.
      [[maybe_unused]] uint64_t idlm = 0;
      if constexpr (KT::kStateMasks) idlm = __ballot(id == light_slot_of<TP, CF>(cptr_at<5>(Pg, left)));

      // 6) shade a vertex (:422, :444-480).
      const bool shade = ls == kStPath;
      // A vertex with no hit is a miss: a path ray's, or in the kernels that resolve above the shadow
      // ray's of a vertex on the light, which keeps its id. (In the early-resolve kernels a traced
      // shadow ray always meets the light, whose test in the trace is the pre-test's, bit for bit.)
      // The block's own guard and the trace's compare.
      if constexpr (!TP::MAT) count_lanes<kLaneEvents>(n_miss, __ballot(shade) & ~__ballot(hit));
      if (shade) {
        SPT_REGION(5);
        const DevPrim& H = s_prims[id];
        const int kind = H.kind;
        f3 x;
        f3 gn = mk(0, 0, 0);
        if constexpr (!TP::SPH) {
          // Rect-only scenes, branch-free: the plane axis of the hit kind selects (o_a, d_a); the
          // hit point re-derives t = (k - o_a) / d_a as the reference does (:103) and
          // the normal is the axis, oriented against the ray (:123,:166,:209).
          float oa, da, ia = ia_hit;
          if constexpr (TP::CONSTGEO) {  // the axis from the position: bit selects (axis_masks)
            oa = axis_pick<kAxb>(am, o.z, o.y, o.x);
            da = axis_pick<kAxb>(am, d.z, d.y, d.x);
          } else {
            const bool kxy = kind == SPT_RECT_XY, kxz = kind == SPT_RECT_XZ;
            oa = kxy ? o.z : (kxz ? o.y : o.x);
            da = kxy ? d.z : (kxz ? d.y : d.x);
          }
          const float n_ = H.w1 - oa;
          const float tr = hit_plane_t(n_, da, ia, plane_t(n_, ia));  // the winner's t, corrected
          x = mk(keep(o.x + d.x * tr), keep(o.y + d.y * tr), keep(o.z + d.z * tr));
          // a miss vertex is the origin (:373-374); a leaked path ending at its miss (the LEAK == 1
          // kernels, see below) never reads it
          if constexpr (CF::LEAK != 1) x = hit ? x : mk(0, 0, 0);
          // The normal's sign: 1 against a ray that runs down the axis, else -1. In the literal
          // leak-end kernels as ONE bit operation, 1.0 with the inverse of da's sign bit. The two forms
          // differ only at da = -0.0 (the compare says -1, the bits +1), and no vertex whose nl is read
          // has a zero da: a plane the ray runs parallel to has rcp_nr(+-0) = NaN for its distance and
          // is not hit (spt_device.h), and a miss ends a leaked path here (term, LEAK == 1), after
          // which the lane's next ray is a camera ray, whose select drops the cosine direction made
          // from nl, or none at all. A NaN da is the same: no hit on that axis.
          float sg;
          if constexpr (TP::CONSTGEO && CF::LEAK == 1) sg = __uint_as_float(sign_against(__float_as_uint(da)));
          else sg = da < 0.0f ? 1.0f : -1.0f;
          if constexpr (TP::CONSTGEO) {
            // sg on the hit's axis, +0 on the other two, as the selects gave: sg & ~(xy | xz),
            // sg & (xy | xz) & ~xy, sg & xy
            const uint32_t sb = __float_as_uint(sg);
            // (kAxisBits: sg & yz, sg & xz, sg & ~yz & ~xz)
            if constexpr (kAxb)
              nl = mk(__uint_as_float(sb & am.yz), __uint_as_float(sb & am.xz), __uint_as_float(band_nor(sb, am.yz, am.xz)));
            else
            nl = mk(__uint_as_float(band_andn(sb, sb, am.xyxz)), __uint_as_float(band_andn(sb, am.xyxz, am.xy)),
                    __uint_as_float(sb & am.xy));
          } else {
            const bool kxy = kind == SPT_RECT_XY, kxz = kind == SPT_RECT_XZ, kyz = !kxy && !kxz;
            nl = mk(kyz ? sg : 0.0f, kxz ? sg : 0.0f, kxy ? sg : 0.0f);
            if (TP::MAT) gn = mk(kyz ? 1.0f : 0.0f, kxz ? 1.0f : 0.0f, kxy ? 1.0f : 0.0f);
          }
        } else {
        if (!hit) {
          x = mk(0, 0, 0);
          if constexpr (TP::MAT) ++n_miss;
        } else {
          // plane distance as the reference derives it (:103); spheres: the root
          // (this and the normals below are restated by guide_vertex, spt_guide.hip: see the staging)
          float tr = hit_t<TP>(H, hpos, o, d, ia_hit, G);
          if (kind == SPT_RECT_XY) tr = hit_plane_t(H.w1 - o.z, d.z, ia_hit, tr);
          else if (kind == SPT_RECT_XZ) tr = hit_plane_t(H.w1 - o.y, d.y, ia_hit, tr);
          else if (kind == SPT_RECT_YZ) tr = hit_plane_t(H.w1 - o.x, d.x, ia_hit, tr);
          x = mk(o.x + d.x * tr, o.y + d.y * tr, o.z + d.z * tr);
        }
        // Hitable::normal, oriented against the ray (:123,:166,:209,:251); gn = the unoriented
        // (geometric) normal `n` of the SPEC/REFR code :482-491 (MAT only)
        if (kind == SPT_RECT_XY) {
          nl = d.z < 0.0f ? mk(0, 0, 1) : mk(0, 0, -1);
          if (TP::MAT) gn = mk(0, 0, 1);
        } else if (kind == SPT_RECT_XZ) {
          nl = d.y < 0.0f ? mk(0, 1, 0) : mk(0, -1, 0);
          if (TP::MAT) gn = mk(0, 1, 0);
        } else if (kind == SPT_RECT_YZ) {
          nl = d.x < 0.0f ? mk(1, 0, 0) : mk(-1, 0, 0);
          if (TP::MAT) gn = mk(1, 0, 0);
        } else {
          // Sphere::normal :248 as (x - p) * (1/r): x lies on the sphere to ~1e-7, so this is the
          // unit normal without the normalize's rsq (contract, oracle c_path; C5 -0.7 %)
          const f3 n = mk((x.x - H.w1) * H.w5, (x.y - H.w2) * H.w5, (x.z - H.w3) * H.w5);
          nl = dot3(n, d) < 0.0f ? n : mk(-n.x, -n.y, -n.z);
          if (TP::MAT) gn = n;
          atomicAdd(&s_nsph[threadIdx.x / 64], 1u);  // the lanes shading a sphere vertex
        }
        }
        f3 f = mk(H.cx, H.cy, H.cz);
        const f3 e = mk(H.ex, H.ey, H.ez);
        const int rr_t = H.rr_t;
        const int depth = dp1;  // this vertex's depth (1 = the first); dp1 moves on at the block's end
        u4 rl = r;  // RR / NEE-mix draws; at vertex 1 from stream 1 (only configs that need them)
        if (CF::NOS1 != 1 && depth == 1) {
          const SPT_CONST KParams* C = cptr_at<3>(Pg, left);
          if (C->rr_depth < 1 || (C->nee_prob > 0.0f && C->nee_prob < 1.0f))
            rl = philox_px(pk, s, 1u | 0x80000000u);
        }
        // Russian roulette :448-454 (+ optional hard depth cap), branch-free: f is scaled by the
        // host-rounded 1/p wherever RR applies (f * 1 elsewhere, exact); f is unused on a path that
        // ends here.
        const int max_depth = CF::MAXD0 == 1 ? 0 : P->max_depth;
        const bool capd = (max_depth > 0) & (depth >= max_depth);
        const bool rr = (depth > rr_depth_of<CF>(P)) | (rr_t < 0);   // p == 0
        const bool alive = (int)u16i(rl.x, rl.y) < rr_t;              // (p > 0) & (p >= 1 | u16 < p)
        // contract v6: a leaked path ends at its first miss (host leak_end_of, oracle
        // c_find_leak_end); the host launches the LEAK == 1 kernels only where that rule holds
        const bool leak = CF::LEAK == 1 || (CF::LEAK < 0 && P->leak_end != 0);
        const bool term = capd | (rr & !alive) | (!hit & leak);
        const float ip = keep(H.ip);  // == 1.0f / p, read unconditionally (no branch)
        const float fsc = rr ? ip : 1.0f;
        f = mk(f.x * fsc, f.y * fsc, f.z * fsc);
        L = mk(fmaf(T.x, e.x, L.x), fmaf(T.y, e.y, L.y), fmaf(T.z, e.z, L.z));
        // Every vertex lane takes T*f and moves its origin to x. A lane whose path ends here
        // restarts at the camera (or pops a REFR child), which resets both; doing it
        // unconditionally saves the register copies of a conditional update.
        T = mk(T.x * f.x, T.y * f.y, T.z * f.z);
        o = x;
        if constexpr (!kEarlyNee) vid = id;
        uint32_t nxt = kStCos;  // the state after this vertex unless the path ends here
        if (TP::MAT && !term && H.refl != SPT_DIFF) {
          // SPEC :481-482 and REFR :484-495 (smallpt's commented-out code; oracle c_path): no NEE.
          // (the directions are restated by guide_chain_step, spt_guide.hip: see the staging)
          // reflRay direction r.d - n*2*n.dot(r.d), renormalised in the unit-direction contract
          // (contract v8: a sphere's gn is unit only to ~3e-6 and the sphere test assumes |d| = 1).
          const f3 Tf = T;
          const float k2 = 2.0f * dot3(gn, d);
          f3 refl = mk(d.x - gn.x * k2, d.y - gn.y * k2, d.z - gn.z * k2);
          if (unit_dirs_of<TP>(Pg)) refl = normalize3(refl);
          bool use_refl = true;
          if (H.refl == SPT_REFR) {
            const bool into = dot3(gn, nl) > 0.0f;                 // :485
            const float nnt = into ? 1.0f / 1.5f : 1.5f / 1.0f;    // nc = 1, nt = 1.5 :486
            const float ddn = dot3(d, nl);
            const float cos2t = 1.0f - nnt * nnt * (1.0f - ddn * ddn);
            if (!(cos2t < 0.0f)) {                                 // else total internal reflection
              const float kk = (into ? 1.0f : -1.0f) * (ddn * nnt + sqrtf(cos2t));
              const f3 tdir = normalize3(mk(d.x * nnt - gn.x * kk, d.y * nnt - gn.y * kk,
                                            d.z * nnt - gn.z * kk));  // :489
              const float a = 1.5f - 1.0f, b = 1.5f + 1.0f, R0 = a * a / (b * b);
              const float c = 1.0f - (into ? -ddn : dot3(tdir, gn));
              const float Re = R0 + (1.0f - R0) * c * c * c * c * c, Tr = 1.0f - Re;
              const float Pp = 0.25f + 0.5f * Re, RP = Re / Pp, TP_ = Tr / (1.0f - Pp);  // :491
              if (depth > 2) {  // Russian roulette between the two :492-493
                if (u16(rl.z, rl.w) < Pp) {
                  T = mk(Tf.x * RP, Tf.y * RP, Tf.z * RP);
                } else {
                  T = mk(Tf.x * TP_, Tf.y * TP_, Tf.z * TP_);
                  d = tdir;
                  use_refl = false;
                }
              } else {  // both :494-495: reflection now, the refraction child later (same L)
                Node& N = s_stack[threadIdx.x * 2 + sp];
                N.o[0] = x.x; N.o[1] = x.y; N.o[2] = x.z;
                N.d[0] = tdir.x; N.d[1] = tdir.y; N.d[2] = tdir.z;
                N.T[0] = Tf.x * Tr; N.T[1] = Tf.y * Tr; N.T[2] = Tf.z * Tr;
                N.depth = depth;
                N.branch = branch | (1u << (depth - 1));
                ++sp;
                T = mk(Tf.x * Re, Tf.y * Re, Tf.z * Re);
              }
            }
          }
          if (use_refl) d = refl;
          nxt = kStSpec;
        } else {
          // DIFF :457-480. T is T*f now; the NEE weight (if the light is reached) multiplies it
          // when the shadow ray resolves, so T = (T*f)*w exactly as the contract rounds it.
          // Computed for every vertex lane (a lane whose path ends here discards it): no branch.
          const SPT_CONST KParams* D = cptr_at<4>(Pg, left);
          bool nee;
          if constexpr (CF::NEE == 1) {
            nee = true;
          } else if constexpr (CF::NEE == 0) {
            nee = false;
          } else {
            const float q = D->nee_prob;
            if (q >= 1.0f) nee = true;
            else if (q <= 0.0f) nee = false;
            else nee = u16(rl.z, rl.w) < q;
          }
          if (nee) {
            // light_sampling :363-369 and the shadow-ray direction :466.
            float xl, zl;
            const int lmode = CF::LMODE >= 0 ? CF::LMODE : D->light_mode;
            if (lmode == SPT_LIGHT_GLIBC_WRAP) {
              const uint32_t ldxi = CF::LREF == 1 ? kRefLdxi : D->ldxi;
              const uint32_t ldzi = CF::LREF == 1 ? kRefLdzi : D->ldzi;
              const float lx0 = CF::LREF == 1 ? kRefLx0 : D->lx0, lz0 = CF::LREF == 1 ? kRefLz0 : D->lz0;
              if constexpr (CF::LREF == 1) {
                // dx = dz = 36 = 4 * 9: the lattice x0 - 1 + m 2^-22, m = r >> 9 (oracle
                // c_wrap_sample) as fma(2^23 + m, 2^-22, x0 - 3) -- the float with bits
                // 0x4B000000 | m is 2^23 + m, so the sum is the same real, rounded once: one or and
                // one fma (rounds 1-4: shift, 24-bit multiply, conversion, fma)
                static_assert(kRefLdxi == 36u && kRefLdzi == 36u, "LREF light lattice");
                // (kFunnelFloats: the shift and the or as one funnel shift, funnel_float)
                const float mx = KT::kFunnelFloats ? funnel_float<0x96u>(r.x) : __uint_as_float(0x4B000000u | (r.x >> 9));
                const float mz = KT::kFunnelFloats ? funnel_float<0x96u>(r.y) : __uint_as_float(0x4B000000u | (r.y >> 9));
                xl = fmaf(mx, 0x1p-22f, lx0 - 3.0f);
                zl = fmaf(mz, 0x1p-22f, lz0 - 3.0f);
              } else {
                xl = D->lx_lattice ? fmaf((float)(r.x >> D->lx_shift), D->lx_scale, D->lx0m1)
                                   : fmaf((float)(int32_t)(((r.x >> 8) << 7) * ldxi), 0x1p-31f, lx0);
                zl = D->lz_lattice ? fmaf((float)(r.y >> D->lz_shift), D->lz_scale, D->lz0m1)
                                   : fmaf((float)(int32_t)(((r.y >> 8) << 7) * ldzi), 0x1p-31f, lz0);
              }
            } else {
              xl = fmaf(u01(r.x), D->ldx, D->lx0);
              zl = fmaf(u01(r.y), D->ldz, D->lz0);
            }
            const float ly = CF::LREF == 1 ? kRefLy : D->ly;
            // light_vec (:367); normalised only in the unit-direction contract (nee_weight)
            const f3 vl = mk(xl - x.x, ly - x.y, zl - x.z);
            const f3 dl = unit_dirs_of<TP>(Pg) ? normalize3(vl) : vl;
            if constexpr (!kNeeByIdentity) l_nee += term ? 0u : 1u;
            const SPT_CONST SceneGeo* G2 = TP::CONSTGEO ? nullptr : cptr(D->geo);
            // a miss keeps id (:466-467), so a vertex ON the light always traces its shadow ray
            bool la, early = false;
            if constexpr (kEarlyNee) {  // the light's own test (light_accepts), keeping t and a
              const Ray6 rl6{x.y, rcp_nr(dl.y), dl.x, x.x, dl.z, x.z};
              RectHit h;
              if constexpr (TP::UPLIGHT) h = rect_eval_test(cptr(D->geo)->test[0], rl6);  // the uploaded light
              else h = rect_eval(CornellRectPtr{kCornellLightPos}, rl6);
              la = h.inb & key_valid(h.tt, kCornellLightPos);
              if constexpr (TP::UPLIGHT) early = la & early_geo_proven<1>(x, D);
              else if constexpr (TP::UPBOX) early = la & early_geo_proven<0>(x, D);
              else early = la & early_nee_proven(x);
              // The weight of :471-472 now, for a proven lane and a traced one alike: nee_weight's
              // arithmetic with |dl . nl| = |dl_a| on the normal's axis a (the dot's zero terms are
              // exact) and t = the light's own t, the bits the trace returns for it. The resolve
              // then needs neither the light's t nor the weight (round 4: -5 VALU per iteration).
              const float adot = fabsf(axis_pick<kAxb>(am, dl.z, dl.y, dl.x));
              const float num = fabsf(dl.y) * adot;
              const float vv = dot3(dl, dl);
              w_nee = (num * kRefNeeC) * rcp_nr((h.tt * h.tt) * (vv * vv));
            } else if constexpr (kEarlySph || kEarlyGeo) {  // the uploaded light rect (XZ, host-checked)
              const RectHit h = rect_eval(G2->rect + D->light_pos,
                                          Ray6{x.y, rcp_nr(dl.y), dl.x, x.x, dl.z, x.z});
              la = h.inb & key_valid(h.tt, (uint32_t)D->light_pos);
              if constexpr (kEarlySph) early = la & early_room_proven(x, D->early_y0);
              else early = la & early_geo_proven<2>(x, D);
              t = early ? h.tt : t;
            } else {
              la = light_accepts<TP>(D, G2, rects_of<TP>(G2), x, dl);
            }
            d = dl;  // a rejected lane generates its cosine direction next iteration anyway
            bool onl;  // the vertex lies on the light
            if constexpr (KT::kStateMasks) onl = __builtin_amdgcn_inverse_ballot_w64(idlm);
            else onl = id == light_slot_of<TP, CF>(D);
            const bool cand = onl | la;
            nxt = early ? kStEarly : (cand ? kStShadow : kStCos);
          }
        }
        ls = term ? kStTerm : nxt;
        dp1 = depth + 1;  // (here: incremented where depth is read, it is copied at the block's end)
      }
      // 5') the HEAD NEE kernel resolves shadow rays here, after the shading block: the ones traced
      //    in this iteration and the ones early_nee_proven() has just resolved (t = the light's t,
      //    the same bits the trace returns). Same arithmetic as 5); the light is black, so a ray
      //    that reaches it shades the light vertex as L += (T*w)*e and ends the path (RR with
      //    p == 0, :448), which is all the common vertex block would do there.
      if constexpr (kEarly) {
        // The block's masks are taken at the top level, where they are counted: the proven lanes,
        // the resolving ones (the block's guard), and the light compare on the trace's final id.
        // (As lane masks, see 5.)
        const uint64_t eam = __ballot(ls == kStEarly);
        // a traced shadow ray that reached the light; never a proven lane (its path ray hit what
        // it shaded, not the black light, which would have ended the path)
        uint64_t thm;
        if constexpr (KT::kStateMasks) thm = idlm;
        else thm = __ballot(id == light_slot_of<TP, CF>(cptr_at<5>(Pg, left)));
        const uint64_t resm = tsm | eam;
        count_lanes<kLaneEvents>(n_early, eam);
        count_lanes<kLaneEvents>(n_shadow, resm);
        count_lanes<kLaneEvents>(n_hit, resm & thm);  // (+ the proven ones, n_early, at the end)
        if (__builtin_amdgcn_inverse_ballot_w64(resm)) {
          SPT_REGION(6);
          const bool ea = __builtin_amdgcn_inverse_ballot_w64(eam);
          const bool lh = __builtin_amdgcn_inverse_ballot_w64(eam | thm);
          if (lh) SPT_REGION(7);
          float wl;
          if constexpr (kEarlyNee) {
            wl = w_nee;  // (from the vertex, above)
          } else {
            // the light's t: the pre-test's for a proven lane, else the traced light hit's own
            // (k_L - o.y) / d.y as the trace ranked it (the light is an XZ rect)
            const float kl = s_prims[light_slot_of<TP, CF>(cptr_at<6>(Pg, left))].w1;
            const float tl = ea ? t : plane_t(kl - o.y, ia_hit);
            // (computed for every resolving lane: a branch around it cost exec-mask SALU)
            wl = keep(nee_weight(unit_dirs_of<TP>(Pg), d, nl, tl, kRefLarea, kRefNeeC));
          }
          // the black light ends a path that reaches it, so only the light vertex's L needs T*w
          // (a lane whose shadow ray is blocked keeps T: the cosine sample follows). A blocked
          // lane adds (T*0)*e = +0 instead of selecting: L + 0 is L bit for bit, T being finite
          // and >= 0 on a path that has not reached the light (one select, not three)
          const float wh = lh ? wl : 0.0f;
          const f3 Tw = mk(T.x * wh, T.y * wh, T.z * wh);
          const DevPrim& H = s_prims[light_slot_of<TP, CF>(cptr_at<7>(Pg, left))];
          L = mk(fmaf(Tw.x, H.ex, L.x), fmaf(Tw.y, H.ey, L.y), fmaf(Tw.z, H.ez, L.z));
          ls = lh ? kStTerm : kStCos;
        }
      }
      // 7) path end: accumulate this sample (:536-538) and start the next one.
      if (ls == kStTerm) {
        if (TP::MAT && sp > 0) {  // the pending refraction child of a REFR split
          --sp;
          const Node& N = s_stack[threadIdx.x * 2 + sp];
          o = mk(N.o[0], N.o[1], N.o[2]);
          d = mk(N.d[0], N.d[1], N.d[2]);
          T = mk(N.T[0], N.T[1], N.T[2]);
          dp1 = N.depth + 1;
          branch = N.branch;
          ls = kStSpec;
        } else {
          SPT_REGION(9);
          const float scale = CF::CAMAX == 1 ? ck.fs : (CF::CAMAX == 2 ? cg.fs : cptr(Pg)->fix_scale);
          acc0 += fix31(L.x, scale);
          acc1 += fix31(L.y, scale);
          acc2 += fix31(L.z, scale);
          ++s;
          L = mk(0, 0, 0);
          T = mk(1, 1, 1);
          dp1 = 1;
          {
            const SPT_CONST KParams* C = cptr_at<8>(Pg, left);
            o = CF::CAMAX == 1   ? mk(ck.o0, ck.o1, ck.o2)
                : CF::CAMAX == 2 ? mk(cg.o0, cg.o1, cg.o2)
                                 : mk(C->cam[0], C->cam[1], C->cam[2]);
          }
          if (TP::MAT) branch = 0;
          ls = kStCam;
          if (s >= s_end) {  // the unit's last sample: flush its pixel's fixed-point sums
            SPT_REGION(1);
            if (lp >> 31) {  // the unit's owner: its slot, written exactly once (zeros included)
              unsigned long long* a = cptr(Pg)->slots + 3ull * (lp & 0x7FFFFFFFu);
              a[0] = acc0;
              a[1] = acc1;
              a[2] = acc2;
            } else {  // a stolen range: add into its pixel's accumulator
              unsigned long long* a = cptr(Pg)->accum + 3ull * lp;
              if (acc0) atomicAdd(a + 0, acc0);
              if (acc1) atomicAdd(a + 1, acc1);
              if (acc2) atomicAdd(a + 2, acc2);
            }
            acc0 = acc1 = acc2 = 0;
            ls = kStIdle;
          }
        }
      }
    }
#ifdef SPT_REGION_STATS
#pragma unroll
    for (int k = 0; k < kRegions; ++k) {
      const uint64_t m = __ballot((reg_flags >> k) & 1u);
      reg_exec[k] += m != 0;
      reg_lanes[k] += (uint32_t)__popcll(m);
    }
    reg_flags = 0;
#endif
    if (--left == 0) break;  // no lane has work, or the runaway guard
  }
  capped = live;  // left with work in hand: the guard (the units are dropped, the host reports it)
  {
    unsigned long long* st = cptr(Pg)->stats;  // wave-reduced by the atomic optimizer
#ifdef SPT_WAVE_TIMES
    if (lane == 0) {  // [12] sum of durations, [13] sum of squares, [14] min start, [15] max end,
                      // [16] sum of iterations, [17] max iterations (stats words 12+ are free here)
      const unsigned long long t1 = __builtin_amdgcn_s_memrealtime(), dt = t1 - wave_t0;
      atomicAdd(st + 12, dt);
      atomicAdd(st + 13, dt * dt);
      atomicMin(st + 14, wave_t0);
      atomicMax(st + 15, t1);
      atomicAdd(st + 16, (unsigned long long)wave_iters);
      atomicMax(st + 17, (unsigned long long)wave_iters);
      atomicAdd(st + 18, wave_t0 >> 4);  // sums of start / end times (/16: no overflow)
      atomicAdd(st + 19, t1 >> 4);
      atomicAdd(st + 20, (unsigned long long)__smid());
      const uint32_t wid = blockIdx.x * (kBlock / 64) + threadIdx.x / 64;
      if (wid < 32768) {
        st[32 + 3 * wid] = wave_t0;
        st[33 + 3 * wid] = t1;
        st[34 + 3 * wid] = ((unsigned long long)__smid() << 32) | wave_iters;
      }
    }
#endif
#ifdef SPT_REGION_STATS
    if (lane == 0) {  // wave-uniform values: one lane adds them
      for (int k = 0; k < kRegions; ++k) {
        atomicAdd(st + kStatRegion + 2 * k, (unsigned long long)reg_exec[k]);
        atomicAdd(st + kStatRegion + 1 + 2 * k, (unsigned long long)reg_lanes[k]);
      }
    }
#endif
    // The event counts: wave-uniform, lane 0 adds them; in the kLaneEvents variants every lane adds
    // its own (the atomic optimizer reduces each over the wave).
    const unsigned long long np = TP::MAT ? n_path : n_gen;
    auto add_events = [&](bool mine) {
      if (!mine) return;
      // light hits: the traced ones and the proven ones (a proven shadow ray reaches the light)
      const unsigned long long nh = (unsigned long long)n_hit + (kEarly ? n_early : 0u);
      atomicAdd(st + 3, nh + (kLaneEvents ? 0ull : np));  // vertices = path rays + light hits
      atomicAdd(st + 5, nh);
      atomicAdd(st + 7, (unsigned long long)n_miss);
      if constexpr (!TP::MAT) atomicAdd(st + kStatShadowTraced, (unsigned long long)n_shadow);
      if constexpr (kEarly) atomicAdd(st + kStatShadowProven, (unsigned long long)n_early);
    };
    if constexpr (kLaneEvents) add_events(true);
    if (lane == 0) {  // wave-uniform counters: one lane adds them
      if (capped) atomicAdd(st + 0, 1ull);  // the host reports an error
      atomicAdd(st + 1, np);
      if constexpr (kLaneEvents) atomicAdd(st + 3, np);
      atomicAdd(st + 6, (unsigned long long)(TP::MAT ? n_cos : n_gen));
      add_events(!kLaneEvents);
      if constexpr (TP::MAT) atomicAdd(st + kStatShadowTraced, (unsigned long long)n_shadow);  // (wave-uniform)
      if constexpr (TP::SPH) atomicAdd(st + kStatSphereVertices, (unsigned long long)s_nsph[threadIdx.x / 64]);
    }
    if (!TP::MAT && blockIdx.x == 0 && threadIdx.x == 0) {  // one camera ray per sample: not cosine rays
      const SPT_CONST KParams* C = cptr(Pg);
      const unsigned long long samples = (unsigned long long)C->n_local_pix * (unsigned long long)C->s_count;
      atomicAdd(st + 6, 0ull - samples);  // (the word is whole again once every wave has added its n_gen)
    }
    if constexpr (!kNeeByIdentity) {  // the per-lane count (the atomic optimizer reduces it over the wave)
      atomicAdd(st + 2, (unsigned long long)l_nee);
      atomicAdd(st + 4, (unsigned long long)l_nee);
    }
  }
}
// 1.31 fixed point -> float, clamp :538 (values are >= 0 by construction). Thread t takes
// unit-order pixel t (coalesced slot reads, chunk j's slot at j * npix + t), adds the pixel's
// stolen-range sums and writes its spread pixel p = (t mod K) * (npix / K) + t / K. Integer sums:
// the order of the adds cannot matter.
__global__ void __launch_bounds__(kBlock)
finalize_slots_kernel(const unsigned long long* __restrict__ accum,
                      const unsigned long long* __restrict__ slots, float* __restrict__ rgb,
                      uint32_t npix, uint32_t n_chunks, uint32_t scr_k, uint32_t scr_q,
                      const unsigned long long* __restrict__ stats) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= npix) return;
  const uint32_t p = (t & ((1u << scr_k) - 1u)) * scr_q + (t >> scr_k);
  if (stats[0] != 0) {  // the launch hit its iteration cap: the slots of the units it dropped hold an
    rgb[3ull * p] = rgb[3ull * p + 1] = rgb[3ull * p + 2] = __builtin_nanf("");  // earlier launch's
    return;                                                                  // sums; no image at all
  }
  unsigned long long v0 = accum[3ull * p], v1 = accum[3ull * p + 1], v2 = accum[3ull * p + 2];
  for (uint32_t j = 0; j < n_chunks; ++j) {
    const unsigned long long* q = slots + 3ull * ((size_t)j * npix + t);
    v0 += q[0];
    v1 += q[1];
    v2 += q[2];
  }
  const float f0 = (float)v0 * 0x1p-31f, f1 = (float)v1 * 0x1p-31f, f2 = (float)v2 * 0x1p-31f;
  rgb[3ull * p] = f0 > 1.0f ? 1.0f : f0;
  rgb[3ull * p + 1] = f1 > 1.0f ? 1.0f : f1;
  rgb[3ull * p + 2] = f2 > 1.0f ? 1.0f : f2;
}

// ---- The launchers (spt_launch.h): everything else about a launch is the host files'.
using RenderFn = void (*)(const KParams*);
#define SPT_X_FN(id, name, TP, CF, level, young) render_kernel<TP, CF>,
static const RenderFn kRenderKernels[KV_COUNT] = {SPT_KERNEL_VARIANTS(SPT_X_FN)};
#undef SPT_X_FN
// The same variants over a pixel list (KParams::pix_list): a second expansion of the table, so the
// unlisted kernels above are untouched by the list (profiles/r14_adaptive_regs.txt).
#define SPT_X_FN(id, name, TP, CF, level, young) render_kernel<TP, CF, true>,
static const RenderFn kRenderKernelsListed[KV_COUNT] = {SPT_KERNEL_VARIANTS(SPT_X_FN)};
#undef SPT_X_FN

int render_kernel_occupancy(int kv) {
  int bpc = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, kRenderKernels[kv], kBlock, 0) != hipSuccess)
    return 0;
  return bpc;
}

void launch_render_kernel(int kv, int grid, const KParams* kp_dev, void* stream, bool listed) {
  hipLaunchKernelGGL((listed ? kRenderKernelsListed : kRenderKernels)[kv], dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, kp_dev);
}

void launch_finalize_slots(const unsigned long long* accum, const unsigned long long* slots,
                           float* rgb, uint32_t npix, uint32_t n_chunks, uint32_t scr_k,
                           uint32_t scr_q, const unsigned long long* stats, void* stream) {
  hipLaunchKernelGGL(finalize_slots_kernel, dim3((npix + kBlock - 1) / kBlock), dim3(kBlock), 0,
                     (hipStream_t)stream, accum, slots, rgb, npix, n_chunks, scr_k, scr_q, stats);
}

}  // namespace spt

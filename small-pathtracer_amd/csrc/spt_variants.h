// spt_variants.h — the render kernel's variants, stated once: the types a variant is compiled on
// (Topo, Cfg), what follows from them (KernelTraits), and the one list of the 26 variants
// (SPT_KERNEL_VARIANTS) that the enum, the public names, the function-pointer table
// (spt_kernel.hip) and the host's info table (kKernelInfo, read by spt_dispatch.cpp) are expanded
// from. Plain C++: no device code.
#pragma once
#include <stdint.h>

#include "../../include/spt.h"
#include "spt_cornell.h"

namespace spt {

// Scene topology the kernel is specialised for: rect counts per kind (-1 = runtime loop), whether
// spheres exist (runtime loop), the light's grouped position (-1 = runtime), and whether the rect
// bounds are the compile-time HEAD scene (CONSTGEO) or read from the uploaded scene (s_load).
// MAT: SPEC/REFR materials and the uniform-hemisphere flag may occur (generic kernel); the
// specialisations are all-DIFF, cosine-scatter scenes (keeps their cosine block branch-free).
// NT*: rect tests per kind (parallel pairs count once).
template <int NXY_, int NXZ_, int NYZ_, bool SPH_, int LPOS_, bool CONSTGEO_ = false,
          int NTXY_ = -1, int NTXZ_ = -1, int NTYZ_ = -1, bool MAT_ = SPH_, bool WIDE_ = false,
          int NBOX_ = -1, bool UPBOX_ = false, bool UPLIGHT_ = false>
struct Topo {
  static constexpr int NBOX = NBOX_;  // boxes of contract v6 (uploaded geometry; -1 = run time)
  // CONSTGEO with the two boxes uploaded (an edited rect[] whose room and light are HEAD's): the
  // room and light as literals, the boxes' slab tests from LDS, the early resolve's box clauses
  // from KParams (early_geo_proven)
  static constexpr bool UPBOX = UPBOX_;
  // UPBOX with the light uploaded as well (an edited light; the room literal): the light's test from
  // the uploaded scene through scalar loads, its plane's y bound of the early resolve from KParams
  static constexpr bool UPLIGHT = UPLIGHT_;
  static constexpr int NXY = NXY_, NXZ = NXZ_, NYZ = NYZ_, LPOS = LPOS_;
  static constexpr int NTXY = NTXY_, NTXZ = NTXZ_, NTYZ = NTYZ_;
  static constexpr bool SPH = SPH_, CONSTGEO = CONSTGEO_, MAT = MAT_;
  static constexpr bool WIDE = WIDE_;  // fp64 wide spheres may occur (their own kernel: VGPRs)
  // Ray-direction contract (oracle c_unit_dirs): 1 = unit directions (spheres, REFR), 0 = free-scale
  // (rect-only DIFF scenes: path directions normalised with rsq_nr1, the NEE vector not at all),
  // -1 = KParams::unit_dirs at run time (the generic kernels)
  static constexpr int DIRS = MAT_ ? -1 : (SPH_ ? 1 : 0);
};
// rect[] of :287-311 (light = XZ #3 -> pos 8); tests besides the room (contract v5): 2 XY box
// pairs; light + 2 box tops; 2 YZ box pairs
using TopoCornell = Topo<6, 5, 6, false, 8, false, 0, 1, 0, false, false, 2>;
using TopoCornellConst = Topo<kCornellNXY, kCornellNXZ, kCornellNYZ, false, kCornellLightPos, true>;
// the same with the boxes uploaded (a box moved or resized; room, light and topology HEAD's)
using TopoCornellUpBox = Topo<kCornellNXY, kCornellNXZ, kCornellNYZ, false, kCornellLightPos, true, -1, -1,
                              -1, false, false, 2, true>;
// ... and with the light uploaded too (the light moved or resized; the room HEAD's)
using TopoCornellUpLight = Topo<kCornellNXY, kCornellNXZ, kCornellNYZ, false, kCornellLightPos, true, -1, -1,
                                -1, false, false, 2, true, true>;
using TopoGeneric = Topo<-1, -1, -1, true, -1>;
// Any scene with spheres but only DIFF materials and cosine scattering (the C5 32-sphere scene):
// no SPEC/REFR stack and branch words, 8 waves/SIMD instead of the generic kernel's 6.
using TopoSphDiff = Topo<-1, -1, -1, true, -1, false, -1, -1, -1, false>;
// Any other rect-only, all-DIFF, cosine-scatter scene (uploaded geometry, run-time loops): the
// free-scale direction contract at compile time (Topo::DIRS 0), no sphere loop.
using TopoRectDiff = Topo<-1, -1, -1, false, -1>;
// Scenes with wide spheres (radius >= SPT_WIDE_SPHERE_RADIUS, tested in fp64: the classic smallpt
// box): the generic kernel plus the fp64 sphere loop, kept apart because the doubles cost VGPRs.
using TopoGenericWide = Topo<-1, -1, -1, true, -1, false, -1, -1, -1, true, true>;

// Estimator configuration the kernel is specialised for (compile-time where the host can prove
// it, -1 = read from KParams at run time). Only wave-uniform branches and parameter loads go away;
// per lane the arithmetic is the same contract.
//   NEE:   1 = nee_prob >= 1 (HEAD :464), 0 = nee_prob <= 0 (cosine only, :474-477)
//   LMODE: light sampling (SPT_LIGHT_GLIBC_WRAP / SPT_LIGHT_UNIFORM)
//   BLACK: 1 = the light's colour is 0, so a path reaching it ends there (RR with p == 0, :448)
//   MAXD0: 1 = no hard depth cap (max_depth == 0, the reference)
//   NOS1:  1 = no vertex-1 stream-1 draws (rr_depth >= 1 and nee_prob is 0 or 1)
//   CAMAX: 1 = axis-aligned camera (horizontal = (h,0,0), vertical = (0,v,0) up to the sign of
//          zero, origin components nonzero, as the reference's :521 camera): the zero products of
//          the camera's fma chain vanish exactly, so the ray is the same bits with 5 fewer VALU;
//          2 = any camera (Camera :262-275 with any lookat/vup, round 6), its per-pixel P_x, P_y,
//          P_z per work unit and the jitter's Cu, Cv in SGPRs: 6 fmas per camera ray (1: 2,
//          0/-1: 12 and scalar loads); the same bits as the general form (contract v5)
//   LREF:  1 = the reference's light sampling and RR constants (light x0/dx 32/36, z0/dz 63/36,
//          y 81.6, area 1296 :365-367,:471; light id 6 :467; rr_depth 5 :448): literals instead
//          of scalar loads in the loop
//   LEAK:  1 = contract v6's leak-end rule (a leaked path ends at its first miss; the host proves
//          it applies, leak_end_of), 0 = leaked paths go on from the miss vertex as the reference's
//          (SPT_FLAG_REFERENCE_LEAKS, or a scene the rule does not hold for), -1 = KParams::leak_end
// The host proves these from the constants themselves (spt_dispatch.cpp, estimator_ok).
template <int NEE_, int LMODE_, int BLACK_, int MAXD0_, int NOS1_, int CAMAX_, int LREF_ = 0,
          int LEAK_ = -1>
struct Cfg {
  static constexpr int NEE = NEE_, LMODE = LMODE_, BLACK = BLACK_, MAXD0 = MAXD0_, NOS1 = NOS1_;
  static constexpr int CAMAX = CAMAX_, LREF = LREF_, LEAK = LEAK_;
};
using CfgRuntime = Cfg<-1, -1, -1, -1, -1, -1>;
// C3/C4: the reference's HEAD estimator; C2: cosine-weighted only (leak-end rule / reference leaks)
using CfgHeadNee = Cfg<1, SPT_LIGHT_GLIBC_WRAP, 1, 1, 1, 1, 1, 1>;
using CfgHeadCos = Cfg<0, SPT_LIGHT_GLIBC_WRAP, 1, 1, 1, 1, 1, 1>;
using CfgHeadNeeRef = Cfg<1, SPT_LIGHT_GLIBC_WRAP, 1, 1, 1, 1, 1, 0>;
// the same estimators with any camera (a tilted lookat)
using CfgHeadNeeCam = Cfg<1, SPT_LIGHT_GLIBC_WRAP, 1, 1, 1, 2, 1, 1>;
using CfgHeadCosCam = Cfg<0, SPT_LIGHT_GLIBC_WRAP, 1, 1, 1, 2, 1, 1>;
using CfgHeadCosRef = Cfg<0, SPT_LIGHT_GLIBC_WRAP, 1, 1, 1, 1, 1, 0>;
// Sphere scenes with the reference's NEE estimator and black light (C5): early NEE resolve
using CfgSphNee = Cfg<1, SPT_LIGHT_GLIBC_WRAP, 1, -1, -1, -1, 1, 1>;
using CfgSphNeeRef = Cfg<1, SPT_LIGHT_GLIBC_WRAP, 1, -1, -1, -1, 1, 0>;
// The LREF constants (the host checks spt_params against them before it picks an LREF kernel).
constexpr int kRefLightId = 6, kRefRrDepth = 5;
constexpr float kRefLx0 = 32.0f, kRefLz0 = 63.0f, kRefLy = 81.6f, kRefLarea = 1296.0f;
constexpr uint32_t kRefLdxi = 36u, kRefLdzi = 36u;

// How a variant resolves NEE shadow rays without a trace, and where the host sets what it needs.
enum EarlyKind {
  kEarlyNone,      // every shadow ray the light's test accepts is traced
  kEarlyLiteral,   // early_nee_proven: HEAD's clauses as literals, always on
  kEarlySphere,    // early_room_proven: above KParams::early_y0 (+inf: off)
  kEarlyClauses,   // early_geo_proven: the uploaded-geometry clauses KParams::eb_*, er_* (er_span 0: off)
};

// What follows from the types a variant is compiled on. render_kernel branches on these; the host
// reads the same values through kKernelInfo.
template <class TP, class CF>
struct KernelTraits {
  // NEE events need no counter in the HEAD NEE kernels: with NEE always on and no SPEC/REFR, every
  // non-terminal vertex takes one (nee_events = vertices - samples, added by the host).
  static constexpr bool kNeeByIdentity = CF::NEE == 1 && !TP::MAT;
  // Early NEE resolve (early_nee_proven): the HEAD NEE kernel only. The shadow-ray resolve then
  // runs after the shading block, for the rays traced in this iteration and the proven ones.
  static constexpr bool kEarlyNee = TP::CONSTGEO && !TP::MAT && !TP::SPH && CF::NEE == 1 &&
                                    CF::BLACK == 1 && CF::LREF == 1 && CF::MAXD0 == 1;
  // The sphere NEE kernel (C5): the same early resolve with the sphere-scene predicate.
  static constexpr bool kEarlySph = !kEarlyNee && TP::SPH && !TP::MAT && !TP::WIDE && CF::NEE == 1 &&
                                    CF::BLACK == 1 && CF::LREF == 1;
  // The uploaded-geometry HEAD-topology NEE kernel (an edited rect[]): early_geo_proven.
  static constexpr bool kEarlyGeo = !kEarlyNee && !TP::SPH && !TP::MAT && TP::NBOX == 2 && CF::NEE == 1 &&
                                    CF::BLACK == 1 && CF::LREF == 1 && CF::MAXD0 == 1;
  static constexpr bool kEarly = kEarlyNee || kEarlySph || kEarlyGeo;
  // The loop's event counters (misses, shadow rays, light hits) are wave-uniform, in SGPRs. Three
  // NEE variants sit at the SGPR cap and paid four more with SGPR spills into VGPR lanes and a VGPR
  // (the run-time-geometry rect kernels cornell_nee and rectdiff_nee, and uplight_nee_cam): theirs
  // stay per lane, in VGPRs. So do the generic kernels' (SPEC/REFR materials), which are not at the
  // cap (78 VGPRs, 5-6 waves per SIMD) and ran 1.7 % slower with the scalar form. A measured choice
  // (profiles/r21_vgprs.txt, profiles/r21_event_counts_ab.txt), like the young cut.
  static constexpr bool kLaneEvents =
      TP::MAT || (!TP::SPH && CF::NEE == 1 && (!TP::CONSTGEO || (TP::UPLIGHT && CF::CAMAX == 2)));
  // The lane states' numbering (spt_kernel.hip, LaneStates): the generating states first, which makes
  // the generate guard one compare. The generic kernels (SPEC/REFR) keep the idle state at 0: with the
  // other numbering the wide-sphere kernel took 82 VGPRs for 80 and lost a wave of occupancy.
  static constexpr bool kGenStatesFirst = !TP::MAT;
  // The traced shadow lanes' mask is derived on the scalar unit from the trace guard's and the shade
  // guard's ballots (spt_kernel.hip, 5): between generate and shade a lane is idle, kStPath or
  // kStShadow, so the mask is the one and-not the other instead of a third compare. Only where both
  // ballots exist at the region's convergent top level and the state does not change between them:
  // the literal early-resolve kernels with wave-uniform event counters. There the light compare on the
  // trace's final id is taken once as well, for the shading's NEE candidates and the resolve's light
  // hits. The others keep their own compares (the sphere NEE kernel paid an SGPR spill and a VGPR).
  static constexpr bool kStateMasks = kEarlyNee && !kLaneEvents;
  // The camera / cosine select of the generated direction as bit selects on the mask ls - 1 (the
  // generate block of spt_kernel.hip): kernels without SPEC/REFR, whose generating lanes are kStCam
  // or kStCos only, and with the axis-aligned camera, whose wave-uniform z the compare form copies
  // into a VGPR in every iteration (elsewhere the two forms are the same number of instructions).
  static constexpr bool kCamMask = kGenStatesFirst && CF::CAMAX == 1;
  // Round 30, the literal kernels (TP::CONSTGEO: HEAD's and the room-literal edited-scene ones); the
  // run-time-geometry and generic kernels keep their instructions (tools/isa_same.py).
  // A random word's unit-interval float, (E << 23) | (r >> 9), as one funnel shift (spt_device.h,
  // funnel_float): the cosine sample's xi2 and the LREF light lattice's two words.
  static constexpr bool kFunnelFloats = TP::CONSTGEO;
  // The primitive slots carry the rectangle's kind in bits 4 and 5 (spt_cornell.h, cornell_slot), so
  // the hit's two plane-axis masks are two one-bit field extracts of the winning position where the
  // grouped numbering needed a subtract and a shift each (spt_kernel.hip, axis_masks). The room-literal
  // NEE kernels (upbox_nee, uplight_nee and their any-camera forms) keep the grouped numbering: with
  // the slots each of them paid one more SGPR spill (profiles/r30_vgprs.txt).
  static constexpr bool kAxisBits = TP::CONSTGEO && !(TP::UPBOX && CF::NEE == 1);
  // A miss reads the table entry its key's low bits name, slot 63 staged with zero emission, instead
  // of selecting prim 0's position behind the hit compare (spt_trace.h, intersect_scene): the literal
  // leak-end kernels, where a miss ends the path in the same shading block, and of those the ones in
  // which no shadow ray can miss and keep its vertex's id -- the early-resolve NEE kernels, which
  // trace a shadow ray only when the light's own test accepts it, and the cosine-only ones.
  static constexpr bool kMissEntry = TP::CONSTGEO && CF::LEAK == 1 && (kEarlyNee || CF::NEE == 0);
  // For the host. The UPBOX / UPLIGHT kernels are CONSTGEO (kEarlyNee) and take their box clauses
  // from KParams (early_geo_proven inside early_nee_proven's place): clauses, not literals.
  static constexpr EarlyKind early = kEarlyNee ? (TP::UPBOX ? kEarlyClauses : kEarlyLiteral)
                                     : kEarlySph ? kEarlySphere
                                     : kEarlyGeo ? kEarlyClauses
                                                 : kEarlyNone;
};

// The scene classes the host sorts a scene into; a Topo runs the scenes of one class (topo_class).
// Each of the HEAD classes is a subset of the one before it.
enum SceneClass {
  kSceneWide,          // fp64 wide spheres: only TopoGenericWide has their loop
  kSceneGeneric,       // anything without wide spheres
  kSceneSphDiff,       // all-DIFF, cosine scatter, with (narrow) spheres
  kSceneRectDiff,      // all-DIFF, cosine scatter, rectangles only
  kSceneHeadTopo,      // ... with HEAD's topology (counts, light position, room, two boxes)
  kSceneHeadRoom,      // ... whose room is HEAD's bit for bit
  kSceneHeadRoomLight, // ... and whose light is HEAD's too
  kSceneHeadLiteral,   // the HEAD scene's geometry bit for bit
  kSceneClassCount
};
template <class TP>
constexpr SceneClass topo_class() {
  return TP::WIDE                    ? kSceneWide
         : TP::MAT                   ? kSceneGeneric
         : TP::SPH                   ? kSceneSphDiff
         : TP::UPLIGHT               ? kSceneHeadRoom
         : TP::UPBOX                 ? kSceneHeadRoomLight
         : TP::CONSTGEO              ? kSceneHeadLiteral
         : TP::NBOX == 2             ? kSceneHeadTopo
                                     : kSceneRectDiff;
}

// Specialisation levels, the caps of SPT_FLAG_KERNEL_LEVEL: a variant runs when its level is within
// the cap (generic 0, cornell 1, const 2, auto 3).
constexpr int kLevelGeneric = 0, kLevelCornell = 1, kLevelConst = 2, kLevelAuto = 3;

// THE list of variants, in the order of their public ids (spt_kernel_name; tests/test_dispatch.py
// pins ids and names): X(enum id, public name, Topo, Cfg, level, young cut).
// Young cut: the launch sizing applies SPT_YOUNG_CUT (spt_kparams.h) to this variant. A measured
// choice, not a consequence of the types (profiles/r05_young_cut_ab.json: the literal HEAD NEE
// kernels and the room-literal edited-scene NEE kernels gained, the others lost).
#define SPT_KERNEL_VARIANTS(X)                                                             \
  X(GENERIC, "generic", TopoGeneric, CfgRuntime, kLevelGeneric, false)                     \
  X(CORNELL, "cornell", TopoCornell, CfgRuntime, kLevelCornell, false)                     \
  X(CONST, "const", TopoCornellConst, CfgRuntime, kLevelConst, false)                      \
  X(CONST_NEE, "const_nee", TopoCornellConst, CfgHeadNee, kLevelAuto, true)                \
  X(CONST_COS, "const_cos", TopoCornellConst, CfgHeadCos, kLevelAuto, false)               \
  X(SPHDIFF, "sphdiff", TopoSphDiff, CfgRuntime, kLevelCornell, false)                     \
  X(WIDE, "wide", TopoGenericWide, CfgRuntime, kLevelGeneric, false)                       \
  X(SPHDIFF_NEE, "sphdiff_nee", TopoSphDiff, CfgSphNee, kLevelAuto, false)                 \
  X(RECTDIFF, "rectdiff", TopoRectDiff, CfgRuntime, kLevelCornell, false)                  \
  X(CONST_NEE_REF, "const_nee_ref", TopoCornellConst, CfgHeadNeeRef, kLevelAuto, true)     \
  X(CONST_COS_REF, "const_cos_ref", TopoCornellConst, CfgHeadCosRef, kLevelAuto, false)    \
  X(SPHDIFF_NEE_REF, "sphdiff_nee_ref", TopoSphDiff, CfgSphNeeRef, kLevelAuto, false)      \
  X(CORNELL_NEE, "cornell_nee", TopoCornell, CfgHeadNee, kLevelConst, false)               \
  X(CORNELL_COS, "cornell_cos", TopoCornell, CfgHeadCos, kLevelConst, false)               \
  X(RECTDIFF_NEE, "rectdiff_nee", TopoRectDiff, CfgHeadNee, kLevelConst, false)            \
  X(RECTDIFF_COS, "rectdiff_cos", TopoRectDiff, CfgHeadCos, kLevelConst, false)            \
  X(UPBOX_NEE, "upbox_nee", TopoCornellUpBox, CfgHeadNee, kLevelAuto, true)                \
  X(UPBOX_COS, "upbox_cos", TopoCornellUpBox, CfgHeadCos, kLevelAuto, false)               \
  X(CONST_NEE_CAM, "const_nee_cam", TopoCornellConst, CfgHeadNeeCam, kLevelAuto, true)     \
  X(CONST_COS_CAM, "const_cos_cam", TopoCornellConst, CfgHeadCosCam, kLevelAuto, false)    \
  X(UPBOX_NEE_CAM, "upbox_nee_cam", TopoCornellUpBox, CfgHeadNeeCam, kLevelAuto, true)     \
  X(UPBOX_COS_CAM, "upbox_cos_cam", TopoCornellUpBox, CfgHeadCosCam, kLevelAuto, false)    \
  X(UPLIGHT_NEE, "uplight_nee", TopoCornellUpLight, CfgHeadNee, kLevelAuto, true)          \
  X(UPLIGHT_COS, "uplight_cos", TopoCornellUpLight, CfgHeadCos, kLevelAuto, false)         \
  X(UPLIGHT_NEE_CAM, "uplight_nee_cam", TopoCornellUpLight, CfgHeadNeeCam, kLevelAuto, true) \
  X(UPLIGHT_COS_CAM, "uplight_cos_cam", TopoCornellUpLight, CfgHeadCosCam, kLevelAuto, false)

#define SPT_X_ENUM(id, name, TP, CF, level, young) KV_##id,
enum KernelVariant { SPT_KERNEL_VARIANTS(SPT_X_ENUM) KV_COUNT };
#undef SPT_X_ENUM

// One variant as the host sees it: its name, the scenes and params it runs (the Cfg constants, -1 =
// run time), and what the launch and the statistics must know about it.
struct KernelInfo {
  const char* name;
  SceneClass scene;
  int level;
  int nee, lmode, black, maxd0, nos1, camax, lref, leak;  // Cfg
  bool nee_by_identity;
  EarlyKind early;
  bool young_cut;
};
template <class TP, class CF>
constexpr KernelInfo kernel_info(const char* name, int level, bool young) {
  return KernelInfo{name,      topo_class<TP>(), level,    CF::NEE,  CF::LMODE, CF::BLACK,
                    CF::MAXD0, CF::NOS1,         CF::CAMAX, CF::LREF, CF::LEAK,
                    KernelTraits<TP, CF>::kNeeByIdentity, KernelTraits<TP, CF>::early, young};
}
#define SPT_X_INFO(id, name, TP, CF, level, young) kernel_info<TP, CF>(name, level, young),
constexpr KernelInfo kKernelInfo[KV_COUNT] = {SPT_KERNEL_VARIANTS(SPT_X_INFO)};
#undef SPT_X_INFO

}  // namespace spt

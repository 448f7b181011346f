// spt_launch.h — the seams of the render path (internal; the public statement is include/spt.h):
//   spt_dispatch.cpp  pure host code, no HIP: validation, scene grouping, the kernel choice, the
//                     launch sizing, the last-error text
//   spt_kernel.hip    the render kernels, and their three launchers below: hipLaunchKernelGGL on a
//                     template instantiation is the one thing a plain C++ file cannot do
//   spt_guide.hip     the guide kernel and its two launchers (both kernels trace through spt_trace.h)
//   spt_guide_light.hip  the light-guide kernel and its two launchers (it traces through spt_trace.h too)
//   spt_context.cpp  contexts, uploads, launches and statistics (HIP runtime calls)
#pragma once
#include <stdint.h>

#include "spt_kparams.h"
#include "spt_status.h"
#include "spt_variants.h"

namespace spt {

// ---- spt_dispatch.cpp (and spt_status.h's fail)
spt_status validate(const spt_prim* prims, int32_t n, const spt_camera* cam, const spt_params* p);
void to_dev(const spt_prim* s, int n, DevPrim* out);
// Grouped geometry; *light_pos = position of prim `light` in rect[] / sph[] (-1 if absent).
void build_geo(const spt_prim* s, int n, SceneGeo* g, int light, int* light_pos);
// The kernel variant of a render (KV_*). Also sets what the variant runs under in *K: the fp32
// camera, light_black, leak_end, early_y0, the early_geo_setup clauses and ul_ybits.
int select_variant(const spt_prim* prims, int n_prims, const spt_camera* cam, const spt_params* p,
                   const SceneGeo& g, int light_pos, KParams* K);

// The sizes of one launch that are not KParams fields.
struct LaunchPlan {
  bool small_launch;  // fewer than SPT_SMALL_ITERS lane-iterations per resident lane
  int bpc, grid;      // resident blocks per CU of this launch, blocks
  uint32_t n_chunks;  // units per pixel
};
// Launch sizing, plain arithmetic: from the device's CU count, the variant kv and its resident
// blocks per CU, the params, the sample window's length and the shard's pixels to the unit size,
// the grid, the queue policy (guided grabs, stealing, young cut), the pixel spreading, the magic
// divisors, the camera terms (from K->cam: select_variant first) and the light lattice. Fills *K
// and *plan; fails when the launch would have 2^31 units or more.
spt_status plan_launch(int n_cu, int variant_bpc, int kv, const spt_params* p, int32_t s_count,
                       int n_local_pix, KParams* K, LaunchPlan* plan);

// ---- spt_kernel.hip (stream: a hipStream_t; errors are left to the caller's hipGetLastError)
int render_kernel_occupancy(int kv);  // resident blocks per CU of variant kv; <= 0: query failed
// listed: the variant over KParams::pix_list (kp_dev->pix_list must be set)
void launch_render_kernel(int kv, int grid, const KParams* kp_dev, void* stream, bool listed = false);
void launch_finalize_slots(const unsigned long long* accum, const unsigned long long* slots,
                           float* rgb, uint32_t npix, uint32_t n_chunks, uint32_t scr_k,
                           uint32_t scr_q, const unsigned long long* stats, void* stream);

// ---- spt_guide.hip (stream and errors as above)
// The guide kernel (SPT_HAS_GUIDE): guide_kernel<TopoGenericWide> for a scene with wide spheres, else
// guide_kernel<TopoGeneric>. grid * kBlock lanes >= n_local_pix << guide_kshift. chain: the
// instantiation that follows the specular chain (SPT_HAS_GUIDE_CHAIN), which has its own occupancy.
int guide_kernel_occupancy(bool wide, bool chain);  // resident blocks per CU; <= 0: query failed
void launch_guide_kernel(bool wide, bool chain, int grid, const KParams* kp_dev, void* stream);

// ---- spt_guide_light.hip (stream and errors as above)
// The light-guide kernel (SPT_HAS_GUIDE_LIGHT): the same four instantiations, chosen the same way.
// grid * kBlock lanes >= n_local_pix << light_kshift.
int light_guide_kernel_occupancy(bool wide, bool chain);  // resident blocks per CU; <= 0: query failed
void launch_light_guide_kernel(bool wide, bool chain, int grid, const KParams* kp_dev, void* stream);

// ---- spt_dispatch.cpp: lanes per pixel of a guide launch (a power of two, 1..64): the smallest K
// with n_local_pix * K >= the device's resident lanes (n_cu * bpc * kBlock), at most the window's
// sample count rounded up to a power of two.
int guide_lanes_per_pixel(int n_cu, int bpc, int n_local_pix, int32_t s_count);

}  // namespace spt

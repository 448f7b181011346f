// spt_guide_light.hip — the light guide (include/spt.h, SPT_HAS_GUIDE_LIGHT), device and host:
// light_guide_kernel, which fills a light guide's integer records with the render's own trace
// (spt_trace.h), and its two launchers (spt_launch.h; the context launches it, spt_context.cpp
// spt_light_guide_window); then the object that holds the records on the device, the resolve and shade
// kernels and the spt_light_guide_* / spt_light_shade_async calls. The resolve's and the shade's
// arithmetic is spt_guide_light.h's, shared with the CPU statements (spt_guide_light_host.cpp).
#include <hip/hip_runtime.h>

#include <cmath>

#include "spt_guide_device.h"
#include "spt_guide_light.h"
#include "spt_launch.h"
#include "spt_trace.h"

namespace spt {

// ---- The light-guide kernel: the guide's own ray of every sample of the window, followed to the
// guide's vertex (spt_guide_device.h: the first hit, or with CHAIN the vertex where the chain guide takes
// its record), and from a DIFF vertex that is not the light one shadow ray towards a point of the light
// rectangle. Per tested sample the pixel's record int64[4] counts the test, a lit one counts again and
// adds the render's PDF_inverse * BRDF in the render's 1.31 fixed point (fix31).
// The launch has guide_kernel's shape (spt_guide.hip): K = 2^light_kshift lanes of one wave share local
// pixel lp = global lane >> kshift, lane l of the group takes samples s_base + l, + K, ..., the three
// partial sums are reduced over the group with the xor butterfly of cross-lane moves (no LDS memory)
// and the group's first lane does the read-add-write. No queue and no atomics: within a launch a pixel
// belongs to one group and launches on one light guide are ordered by the caller's stream.

// PDF_inverse * BRDF of :471-472: nee_weight of spt_kernel.hip restated operation for operation (it
// stays there: the render kernels' listings are not to move), and div_nr with it.
__device__ __forceinline__ float light_nee_weight(bool unit, f3 d, f3 nl, float t, float larea, float nee_c) {
  if (unit) {
    const float pdf = fabsf((larea * d.y) * rcp_nr(t * t));         // :471
    const float brdf = fabsf(dot3(d, nl) * 0.318309886183790672f);  // :472
    return pdf * brdf;
  }
  const float num = fabsf(d.y) * fabsf(dot3(d, nl));
  const float vv = dot3(d, d);
  return (num * nee_c) * rcp_nr((t * t) * (vv * vv));
}

template <class TP, bool CHAIN>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_num_sgpr(SPT_NUM_SGPR)))
light_guide_kernel(const KParams* __restrict__ Pg) {
  static_assert(!TP::CONSTGEO && TP::MAT && TP::SPH, "the light-guide kernel runs the run-time topologies");
  constexpr int kSegs = CHAIN ? SPT_GUIDE_MAX_CHAIN : 1;
  __shared__ DevPrim s_prims[kMaxPrims];
  __shared__ int s_pos2idx[kMaxPrims];  // grouped position -> primitive index
  __shared__ GeoTest s_test[TP::WIDE ? 1 : kMaxPrims];
  {  // the block's staging: guide_kernel's (render_kernel's for the run-time topologies), pasted
    const SPT_CONST KParams* P = cptr(Pg);
    const SPT_CONST SceneGeo* G = cptr(P->geo);
    const int nrect = G->n_xy + G->n_xz + G->n_yz;
    for (int i = threadIdx.x; i < P->n_prims; i += kBlock) {
      s_prims[i] = P->prims[i];
      s_pos2idx[i] = i < nrect ? G->rect[i].idx : G->sph[i - nrect].idx;
      if (!TP::WIDE && i < G->n_txy + G->n_txz + G->n_tyz + 3 * G->has_room + 3 * G->n_box) {
        const SPT_CONST GeoTest& q = G->test[i];
        s_test[i] = GeoTest{q.k0, q.k1, q.ma, q.ha, q.mb, q.hb, q.pos0, q.pos1};
      }
    }
  }
  __syncthreads();

  const SPT_CONST KParams* P = cptr(Pg);
  const uint32_t ksh = P->light_kshift, K = 1u << ksh;
  const uint32_t gl = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  const uint32_t lp = gl >> ksh, l = gl & (K - 1u);
  const bool live = lp < (uint32_t)P->n_local_pix;  // (a group is live or not as a whole)
  long long n_tested = 0, n_lit = 0, w_sum = 0;
  if (live) {
    PxKey pk;
    float fx, fy;
    pixel_terms<false>(P, lp, pk, fx, fy);
    const f3 cam = mk(P->cam[0], P->cam[1], P->cam[2]);
    const float px = fmaf(P->cam_au[0], fx, fmaf(P->cam_av[0], fy, P->cam_l[0]));
    const float py = fmaf(P->cam_au[1], fx, fmaf(P->cam_av[1], fy, P->cam_l[1]));
    const float pz = fmaf(P->cam_au[2], fx, fmaf(P->cam_av[2], fy, P->cam_l[2]));
    const bool unit = unit_dirs_of<TP>(Pg);
    const float scale = P->fix_scale;
    const uint32_t s_lim = P->s_lim;
    for (uint32_t s = P->s_base + l; s < s_lim; s += K) {
      const SPT_CONST KParams* C = cptr(Pg);  // re-issued scalar loads, not long-lived SGPRs
      const u4 r = philox_px(pk, s, 1u);
      const float Fu = jitter_f(r.x, r.y), Fv = jitter_f(r.z, r.w);
      const f3 v = mk(fmaf(Fv, C->cam_cv[0], fmaf(Fu, C->cam_cu[0], px)),
                      fmaf(Fv, C->cam_cv[1], fmaf(Fu, C->cam_cu[1], py)),
                      fmaf(Fv, C->cam_cv[2], fmaf(Fu, C->cam_cu[2], pz)));
      f3 o = cam, d = normalize_dir(v, unit);
      f3 A = mk(1.0f, 1.0f, 1.0f);  // (the chain step's throughput and length: not recorded here)
      float D = 0.0f;
      for (int seg = 0; seg < kSegs; ++seg) {
        const SPT_CONST KParams* Q = cptr(Pg);  // re-issued per trace
        const SPT_CONST SceneGeo* G = cptr(Q->geo);
        int id = 0, hpos;
        float ia_hit = 0.0f;
        f3 inv;
        if (!intersect_scene<TP>(G, rects_of<TP>(G), tests_of<TP>(G, s_test), G->sph, s_pos2idx, o, d, id,
                                 ia_hit, hpos, inv))
          break;  // a miss on any segment adds nothing
        const DevPrim& H = s_prims[id];
        const float t = hit_t<TP>(H, hpos, o, d, ia_hit, G);  // the winner's exact t
        const GuideVertex V = guide_vertex<true>(H, o, d, ia_hit, t);
        if (H.refl == SPT_DIFF) {
          // the guide's vertex. The render does its NEE at a DIFF vertex only, and a vertex on the
          // light itself is the emitter seen, not a lit surface: neither is tested
          if (id == Q->light_id) break;
          n_tested += 1;
          // the light point: light_sampling's SPT_LIGHT_UNIFORM arithmetic (render_kernel, "light_sampling
          // :363-369") from the Philox word nothing else draws (vertex word 0)
          const u4 rl = philox_px(pk, s, 0u);
          const float xl = fmaf(u01(rl.x), Q->ldx, Q->lx0);
          const float zl = fmaf(u01(rl.y), Q->ldz, Q->lz0);
          // light_vec (:367); normalised only in the unit-direction contract (render_kernel :466)
          const f3 vl = mk(xl - V.x.x, Q->ly - V.x.y, zl - V.x.z);
          const f3 dl = unit ? normalize3(vl) : vl;
          const SPT_CONST SceneGeo* G2 = cptr(cptr(Pg)->geo);
          int id2 = 0, hpos2;
          float ia2 = 0.0f;
          f3 inv2;
          const bool h2 = intersect_scene<TP>(G2, rects_of<TP>(G2), tests_of<TP>(G2, s_test), G2->sph,
                                              s_pos2idx, V.x, dl, id2, ia2, hpos2, inv2);
          const SPT_CONST KParams* L = cptr(Pg);
          if (h2 && id2 == L->light_id) {  // the reference's test :467
            const float t2 = hit_t<TP>(s_prims[id2], hpos2, V.x, dl, ia2, G2);
            const float wt = light_nee_weight(unit, dl, V.nl, t2, L->larea, L->nee_c);
            n_lit += 1;
            w_sum += (long long)fix31(wt, scale);
          }
          break;
        }
        if (seg == kSegs - 1) break;  // a first-hit mirror, an exhausted chain: not tested
        guide_chain_step(H, unit, V.x, V.gn, V.nl, t, A, D, o, d);
      }
    }
  }
  // the group's sums: every lane of the wave takes part (a dead group's lanes hold zeros)
  for (uint32_t m = 1; m < K; m <<= 1) {
    n_tested += shfl_xor64(n_tested, (int)m);
    n_lit += shfl_xor64(n_lit, (int)m);
    w_sum += shfl_xor64(w_sum, (int)m);
  }
  if (live && l == 0) {
    long long* rec = cptr(Pg)->light_rec + 4ull * lp;
    rec[0] += n_tested;
    rec[1] += n_lit;
    rec[2] += w_sum;
  }
}

// ---- The launchers (spt_launch.h)
using LightGuideFn = void (*)(const KParams*);
static LightGuideFn light_guide_fn(bool wide, bool chain) {
  if (chain) return wide ? light_guide_kernel<TopoGenericWide, true> : light_guide_kernel<TopoGeneric, true>;
  return wide ? light_guide_kernel<TopoGenericWide, false> : light_guide_kernel<TopoGeneric, false>;
}

int light_guide_kernel_occupancy(bool wide, bool chain) {
  int bpc = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, light_guide_fn(wide, chain), kBlock, 0) != hipSuccess)
    return 0;
  return bpc;
}

void launch_light_guide_kernel(bool wide, bool chain, int grid, const KParams* kp_dev, void* stream) {
  hipLaunchKernelGGL(light_guide_fn(wide, chain), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, kp_dev);
}

}  // namespace spt

// ---- The light-guide object, the resolve, the shade and the spt_light_* calls

using spt::fail;

namespace {

using spt::kBlock;  // (one block size in this file: the render path's, spt_kparams.h)
constexpr int32_t kMaxSpp = 1 << 24;  // a guide's cap: slot 2 adds at most 2^31 per sample

// One thread per pixel: its 32-byte record as two 16-byte loads, the planes that were asked for.
__global__ void __launch_bounds__(kBlock)
light_resolve_kernel(const long long* __restrict__ rec, uint32_t npix, int64_t n, float r, int full,
                     float* __restrict__ visibility, float* __restrict__ direct, float* __restrict__ tested) {
  const uint32_t px = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (px >= npix) return;
  const longlong2* q = reinterpret_cast<const longlong2*>(rec + 4ull * px);
  const longlong2 q0 = q[0], q1 = q[1];
  const long long S[4] = {q0.x, q0.y, q1.x, q1.y};
  float v, d, ts;
  spt_light_math::resolve_record(S, n, r, full, &v, &d, &ts);
  if (visibility) visibility[px] = v;
  if (direct) direct[px] = d;
  if (tested) tested[px] = ts;
}

// One thread per pixel; out may be albedo (each thread reads its three floats before it writes them).
__global__ void __launch_bounds__(kBlock)
light_shade_kernel(const float* albedo, const float* __restrict__ visibility, uint64_t npix, float shade_floor,
                   float* out) {
  const uint64_t px = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (px >= npix) return;
  const float m = spt_light_math::shade_factor(shade_floor, visibility[px]);
  const float a0 = albedo[3 * px], a1 = albedo[3 * px + 1], a2 = albedo[3 * px + 2];
  out[3 * px] = a0 * m;
  out[3 * px + 1] = a1 * m;
  out[3 * px + 2] = a2 * m;
}

}  // namespace

extern "C" spt_status spt_light_guide_create(int32_t device, const spt_params* p, uint32_t flags,
                                             spt_light_guide** out) {
  if (!p || !out) return fail(SPT_ERR_INVALID_ARG, "null argument");
  if (flags & ~SPT_GUIDE_THROUGH_SPECULAR) return fail(SPT_ERR_INVALID_ARG, "unknown light guide flags");
  if (p->width > 0 && p->height > 0 && p->spp > kMaxSpp)
    return fail(SPT_ERR_INVALID_ARG, "a light guide takes at most 2^24 samples per pixel");
  spt::WindowShape shape;
  SPT_TRY(spt::shape_from_params(p, 0x7FFFFFFFull, &shape));
  SPT_TRY(spt::open_device(device));
  spt_light_guide* g = new spt_light_guide();
  static_cast<spt::WindowShape&>(*g) = shape;
  g->device = device;
  g->flags = flags;
  g->npix = (size_t)g->rows * (size_t)g->width;
  if (g->npix) {
    const size_t bytes = g->npix * spt_light_math::kSlots * sizeof(long long);
    hipError_t e = hipMalloc(&g->rec, bytes);
    if (e == hipSuccess) e = hipMemset(g->rec, 0, bytes);
    if (e != hipSuccess) {
      if (g->rec) (void)hipFree(g->rec);
      delete g;
      return fail(SPT_ERR_OOM, std::string("light guide alloc: ") + hipGetErrorString(e));
    }
  }
  *out = g;
  return SPT_OK;
}

extern "C" spt_status spt_light_guide_destroy(spt_light_guide* g) {
  if (!g) return SPT_OK;
  if (g->rec) {
    (void)hipSetDevice(g->device);
    (void)hipFree(g->rec);
  }
  delete g;
  return SPT_OK;
}

extern "C" spt_status spt_light_guide_clear(spt_light_guide* g, void* stream) {
  if (!g) return fail(SPT_ERR_INVALID_ARG, "null light guide");
  if (g->npix) {
    SPT_HIP(hipSetDevice(g->device));
    SPT_HIP(hipMemsetAsync(g->rec, 0, g->npix * spt_light_math::kSlots * sizeof(long long),
                           (hipStream_t)stream));
  }
  g->samples_done = 0;
  return SPT_OK;
}

extern "C" spt_status spt_light_guide_info_get(const spt_light_guide* g, spt_guide_info* out) {
  if (!g || !out) return fail(SPT_ERR_INVALID_ARG, "null argument");
  out->width = g->width;
  out->rows = g->rows;
  out->spp_total = g->spp_total;
  out->samples_done = g->samples_done;
  out->lanes_per_pixel = g->lanes_per_pixel;
  out->flags = g->flags;
  return SPT_OK;
}

// The launch with the lanes per pixel forced (force_k > 0), as spt_guide.hip's guide_render.
static spt_status light_guide_render(spt_context* ctx, spt_light_guide* g, const spt_prim* prims,
                                     int32_t n_prims, const spt_camera* cam, const spt_params* p,
                                     int32_t sample_base, int32_t sample_count, int force_k, void* stream) {
  if (!ctx || !g || !p) return fail(SPT_ERR_INVALID_ARG, "null context/light guide/params");
  SPT_TRY(spt::shape_accepts(*g, p, sample_base, sample_count, "light guide"));
  if (spt_context_device(ctx) != g->device)
    return fail(SPT_ERR_INVALID_ARG, "the light guide and the context are on different devices");
  if (g->npix) {
    int32_t k = 0;
    SPT_TRY(spt_light_guide_window(ctx, prims, n_prims, cam, p, sample_base, sample_count, g->rec, &k,
                                   force_k, g->flags, stream));
    g->lanes_per_pixel = k;
  }
  g->samples_done += sample_count;  // (a shard without rows only counts)
  return SPT_OK;
}

extern "C" spt_status spt_light_guide_render_async(spt_context* ctx, spt_light_guide* g,
                                                   const spt_prim* prims, int32_t n_prims,
                                                   const spt_camera* cam, const spt_params* p,
                                                   int32_t sample_base, int32_t sample_count, void* stream) {
  return light_guide_render(ctx, g, prims, n_prims, cam, p, sample_base, sample_count, 0, stream);
}

#ifdef SPT_GUIDE_BENCH  // tools/guide_bench.py's library only: never in the shipped libspt.so
extern "C" spt_status spt_light_guide_bench_render_k(spt_context* ctx, spt_light_guide* g,
                                                     const spt_prim* prims, int32_t n_prims,
                                                     const spt_camera* cam, const spt_params* p,
                                                     int32_t sample_base, int32_t sample_count, int32_t k,
                                                     void* stream) {
  if (k < 1 || k > 64 || (k & (k - 1))) return fail(SPT_ERR_INVALID_ARG, "k: a power of two, 1..64");
  return light_guide_render(ctx, g, prims, n_prims, cam, p, sample_base, sample_count, k, stream);
}
#endif

extern "C" spt_status spt_light_guide_resolve(const spt_light_guide* g, float* visibility_dev,
                                              float* direct_dev, float* tested_dev, void* stream) {
  if (!g) return fail(SPT_ERR_INVALID_ARG, "null light guide");
  if (!g->npix || (!visibility_dev && !direct_dev && !tested_dev)) return SPT_OK;
  SPT_HIP(hipSetDevice(g->device));
  int full = 0;
  const float r = spt_film_math::resolve_factor(g->spp_total, g->samples_done, &full);
  hipLaunchKernelGGL(light_resolve_kernel, dim3((unsigned)((g->npix + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     (hipStream_t)stream, (const long long*)g->rec, (uint32_t)g->npix, g->samples_done, r,
                     full, visibility_dev, direct_dev, tested_dev);
  SPT_HIP(hipGetLastError());
  return SPT_OK;
}

extern "C" spt_status spt_light_guide_download(const spt_light_guide* g, int64_t* host_records, void* stream) {
  if (!g || (g->npix && !host_records)) return fail(SPT_ERR_INVALID_ARG, "null argument");
  if (!g->npix) return SPT_OK;
  return spt::copy_and_wait(g->device, host_records, g->rec,
                            g->npix * spt_light_math::kSlots * sizeof(long long), hipMemcpyDeviceToHost,
                            stream);
}

// On the current device: the planes name it (the denoiser's entry points take theirs the same way).
extern "C" spt_status spt_light_shade_async(const float* albedo_dev, const float* visibility_dev,
                                            int64_t n_pixels, float shade_floor, float* out_dev,
                                            void* stream) {
  if (n_pixels < 0 || n_pixels > 0x7FFFFFFFll) return fail(SPT_ERR_INVALID_ARG, "spt_light_shade: bad n_pixels");
  if (!spt_light_math::shade_floor_ok(shade_floor))
    return fail(SPT_ERR_INVALID_ARG, "spt_light_shade: shade_floor must be in (0, 1]");
  if (n_pixels == 0) return SPT_OK;
  if (!albedo_dev || !visibility_dev || !out_dev) return fail(SPT_ERR_INVALID_ARG, "spt_light_shade: null plane");
  hipLaunchKernelGGL(light_shade_kernel, dim3((unsigned)((n_pixels + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     (hipStream_t)stream, albedo_dev, visibility_dev, (uint64_t)n_pixels, shade_floor, out_dev);
  SPT_HIP(hipGetLastError());
  return SPT_OK;
}

// spt_guide.hip — the guide planes (include/spt.h, SPT_HAS_GUIDE), device and host: guide_kernel, which
// fills a guide's integer records with the render's own trace (spt_trace.h), and its two launchers
// (spt_launch.h; the context launches it, spt_context.cpp spt_guide_window); then the object that holds
// the records on the device, the resolve kernel and the spt_guide_* calls. The resolve's arithmetic is
// spt_guide.h's, shared with the CPU statement (spt_guide_host.cpp).
#include <hip/hip_runtime.h>

#include "spt_guide.h"
#include "spt_guide_device.h"
#include "spt_launch.h"
#include "spt_trace.h"

namespace spt {

// ---- The guide kernel: the render's own first ray of every sample of the window, stopped at its
// first vertex. Per hit sample the pixel's record int64[8] takes the hit primitive's colour in the
// render's 1.31 fixed point (fix31), the oriented normal as sgn * fix31(|n|), the ray parameter in
// 48.16 and a hit count; a miss adds nothing.
// Every (pixel, sample) costs the same -- one Philox call, one trace -- so there is no queue and no
// stealing: K = 2^guide_kshift lanes of one wave share local pixel lp = global lane >> kshift, lane l
// of the group takes samples s_base + l, + K, ..., the eight partial sums are reduced over the group
// with an xor butterfly of cross-lane moves (no LDS memory), and the group's first lane does the
// read-add-write of the record. Within a launch a pixel belongs to one group and launches on one guide
// are ordered by the caller's stream, so no atomics. The integers make the sums independent of K,
// the window split and the shard.
// The camera ray is the general form of contract v5 with P_c per pixel (render_kernel's CAMAX 2
// arithmetic: the same bits as the inline general form, oracle c_path).
//
// The vertex frame, the chain step and the 64-bit cross-lane move are spt_guide_device.h's, shared
// with the light-guide kernel (spt_guide_light.hip).
//
// One lane's partial sums of its pixel's record, and the eight adds of one hit sample (include/spt.h,
// the record's layout): colour c and |nl| through the render's fix31 with the launch's scale, as
// render_kernel's path end accumulates a sample's radiance; the depth in 48.16, capped at 2^20.
struct GuideSums { long long a0 = 0, a1 = 0, a2 = 0, n0 = 0, n1 = 0, n2 = 0, dsum = 0, hits = 0; };
__device__ __forceinline__ void guide_record_add(GuideSums& S, f3 c, f3 nl, float depth, float scale) {
  S.a0 += (long long)fix31(c.x, scale);
  S.a1 += (long long)fix31(c.y, scale);
  S.a2 += (long long)fix31(c.z, scale);
  const long long m0 = (long long)fix31(fabsf(nl.x), scale), m1 = (long long)fix31(fabsf(nl.y), scale);
  const long long m2 = (long long)fix31(fabsf(nl.z), scale);
  S.n0 += nl.x < 0.0f ? -m0 : m0;
  S.n1 += nl.y < 0.0f ? -m1 : m1;
  S.n2 += nl.z < 0.0f ? -m2 : m2;
  S.dsum += (long long)(unsigned long long)(fminf(depth, 0x1p20f) * 65536.0f);
  S.hits += 1;
}

// One body for both kinds of record. A sample's ray is followed for at most kSegs segments and its
// record taken at the first DIFF hit or at the last segment, whatever is hit there; a miss on any
// segment adds nothing. CHAIN (spt_guide_create_ex with SPT_GUIDE_THROUGH_SPECULAR): kSegs is
// SPT_GUIDE_MAX_CHAIN, the ray goes on through SPEC and REFR primitives, and the lanes of a group
// differ in their trace counts (the reduction does not change). Without it kSegs is 1: the first-hit
// record is the chain record of one segment, colour 1 * c (exact) and depth t.
template <class TP, bool CHAIN>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_num_sgpr(SPT_NUM_SGPR)))
guide_kernel(const KParams* __restrict__ Pg) {
  static_assert(!TP::CONSTGEO && TP::MAT && TP::SPH, "the guide kernel runs the run-time topologies");
  constexpr int kSegs = CHAIN ? SPT_GUIDE_MAX_CHAIN : 1;
  __shared__ DevPrim s_prims[kMaxPrims];
  __shared__ int s_pos2idx[kMaxPrims];  // grouped position -> primitive index
  __shared__ GeoTest s_test[TP::WIDE ? 1 : kMaxPrims];
  {  // the block's staging: render_kernel's for the run-time topologies, pasted (see above)
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
  const uint32_t ksh = P->guide_kshift, K = 1u << ksh;
  const uint32_t gl = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  const uint32_t lp = gl >> ksh, l = gl & (K - 1u);
  const bool live = lp < (uint32_t)P->n_local_pix;  // (a group is live or not as a whole)
  GuideSums S;
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
      f3 A = mk(1.0f, 1.0f, 1.0f);  // the chain's throughput and length so far
      float D = 0.0f;
      for (int seg = 0; seg < kSegs; ++seg) {
        // re-issued per trace, as C is per sample; the first-hit pass's one trace reads it through C,
        // with the sample's camera loads (one wait fewer per sample: the two-branch kernel's form)
        const SPT_CONST SceneGeo* G = cptr((CHAIN ? cptr(Pg) : C)->geo);
        int id = 0, hpos;
        float ia_hit = 0.0f;
        f3 inv;
        if (!intersect_scene<TP>(G, rects_of<TP>(G), tests_of<TP>(G, s_test), G->sph, s_pos2idx, o, d, id,
                                 ia_hit, hpos, inv))
          break;
        const DevPrim& H = s_prims[id];
        const float t = hit_t<TP>(H, hpos, o, d, ia_hit, G);  // the winner's exact t
        const GuideVertex V = guide_vertex<CHAIN>(H, o, d, ia_hit, t);
        if (H.refl == SPT_DIFF || seg == kSegs - 1) {
          guide_record_add(S, mk(A.x * H.cx, A.y * H.cy, A.z * H.cz), V.nl, CHAIN ? D + t : t, scale);
          break;
        }
        guide_chain_step(H, unit, V.x, V.gn, V.nl, t, A, D, o, d);
      }
    }
  }
  // the group's sums: every lane of the wave takes part (a dead group's lanes hold zeros)
  for (uint32_t m = 1; m < K; m <<= 1) {
    S.a0 += shfl_xor64(S.a0, (int)m);
    S.a1 += shfl_xor64(S.a1, (int)m);
    S.a2 += shfl_xor64(S.a2, (int)m);
    S.n0 += shfl_xor64(S.n0, (int)m);
    S.n1 += shfl_xor64(S.n1, (int)m);
    S.n2 += shfl_xor64(S.n2, (int)m);
    S.dsum += shfl_xor64(S.dsum, (int)m);
    S.hits += shfl_xor64(S.hits, (int)m);
  }
  if (live && l == 0) {
    long long* rec = cptr(Pg)->guide_rec + 8ull * lp;
    rec[0] += S.a0;
    rec[1] += S.a1;
    rec[2] += S.a2;
    rec[3] += S.n0;
    rec[4] += S.n1;
    rec[5] += S.n2;
    rec[6] += S.dsum;
    rec[7] += S.hits;
  }
}

// ---- The launchers (spt_launch.h)
using GuideFn = void (*)(const KParams*);
static GuideFn guide_fn(bool wide, bool chain) {
  if (chain) return wide ? guide_kernel<TopoGenericWide, true> : guide_kernel<TopoGeneric, true>;
  return wide ? guide_kernel<TopoGenericWide, false> : guide_kernel<TopoGeneric, false>;
}

int guide_kernel_occupancy(bool wide, bool chain) {
  int bpc = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, guide_fn(wide, chain), kBlock, 0) != hipSuccess)
    return 0;
  return bpc;
}

void launch_guide_kernel(bool wide, bool chain, int grid, const KParams* kp_dev, void* stream) {
  hipLaunchKernelGGL(guide_fn(wide, chain), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, kp_dev);
}

}  // namespace spt

// ---- The guide object, the resolve and the spt_guide_* calls

using spt::fail;

namespace {

using spt::kBlock;  // (one block size in this file: the render path's, spt_kparams.h)
constexpr int32_t kMaxSpp = 1 << 24;  // slot 6 adds < 2^36 per sample: 2^24 samples stay below 2^63

// One thread per pixel: its 64-byte record as four 16-byte loads, the planes that were asked for.
__global__ void __launch_bounds__(kBlock)
guide_resolve_kernel(const long long* __restrict__ rec, uint32_t npix, int64_t n, float r, int full,
                     float* __restrict__ albedo, float* __restrict__ normal, float* __restrict__ depth,
                     float* __restrict__ coverage) {
  const uint32_t px = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (px >= npix) return;
  const longlong2* q = reinterpret_cast<const longlong2*>(rec + 8ull * px);
  const longlong2 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
  const long long S[8] = {q0.x, q0.y, q1.x, q1.y, q2.x, q2.y, q3.x, q3.y};
  float a[3], nn[3], d, c;
  spt_guide_math::resolve_record(S, n, r, full, a, nn, &d, &c);
  if (albedo) {
    albedo[3ull * px] = a[0];
    albedo[3ull * px + 1] = a[1];
    albedo[3ull * px + 2] = a[2];
  }
  if (normal) {
    normal[3ull * px] = nn[0];
    normal[3ull * px + 1] = nn[1];
    normal[3ull * px + 2] = nn[2];
  }
  if (depth) depth[px] = d;
  if (coverage) coverage[px] = c;
}

}  // namespace

extern "C" spt_status spt_guide_create_ex(int32_t device, const spt_params* p, uint32_t flags,
                                          spt_guide** out) {
  if (!p || !out) return fail(SPT_ERR_INVALID_ARG, "null argument");
  if (flags & ~SPT_GUIDE_THROUGH_SPECULAR) return fail(SPT_ERR_INVALID_ARG, "unknown guide flags");
  // the guide's own cap sits between the shape's first check and its second: a size that is not
  // positive is reported first, as ever
  if (p->width > 0 && p->height > 0 && p->spp > kMaxSpp)
    return fail(SPT_ERR_INVALID_ARG, "a guide takes at most 2^24 samples per pixel");
  spt::WindowShape shape;
  SPT_TRY(spt::shape_from_params(p, 0x7FFFFFFFull, &shape));
  SPT_TRY(spt::open_device(device));
  spt_guide* g = new spt_guide();
  static_cast<spt::WindowShape&>(*g) = shape;
  g->device = device;
  g->flags = flags;
  g->npix = (size_t)g->rows * (size_t)g->width;
  if (g->npix) {
    hipError_t e = hipMalloc(&g->rec, g->npix * 8 * sizeof(long long));
    if (e == hipSuccess) e = hipMemset(g->rec, 0, g->npix * 8 * sizeof(long long));
    if (e != hipSuccess) {
      if (g->rec) (void)hipFree(g->rec);
      delete g;
      return fail(SPT_ERR_OOM, std::string("guide alloc: ") + hipGetErrorString(e));
    }
  }
  *out = g;
  return SPT_OK;
}

extern "C" spt_status spt_guide_create(int32_t device, const spt_params* p, spt_guide** out) {
  return spt_guide_create_ex(device, p, 0u, out);
}

extern "C" spt_status spt_guide_destroy(spt_guide* g) {
  if (!g) return SPT_OK;
  if (g->rec) {
    (void)hipSetDevice(g->device);
    (void)hipFree(g->rec);
  }
  delete g;
  return SPT_OK;
}

extern "C" spt_status spt_guide_clear(spt_guide* g, void* stream) {
  if (!g) return fail(SPT_ERR_INVALID_ARG, "null guide");
  if (g->npix) {
    SPT_HIP(hipSetDevice(g->device));
    SPT_HIP(hipMemsetAsync(g->rec, 0, g->npix * 8 * sizeof(long long), (hipStream_t)stream));
  }
  g->samples_done = 0;
  return SPT_OK;
}

extern "C" spt_status spt_guide_info_get(const spt_guide* g, spt_guide_info* out) {
  if (!g || !out) return fail(SPT_ERR_INVALID_ARG, "null argument");
  out->width = g->width;
  out->rows = g->rows;
  out->spp_total = g->spp_total;
  out->samples_done = g->samples_done;
  out->lanes_per_pixel = g->lanes_per_pixel;
  out->flags = g->flags;
  return SPT_OK;
}

// The launch with the lanes per pixel forced (force_k > 0): what tools/guide_bench.py's K sweep calls
// in a library built with -DSPT_GUIDE_BENCH; the ABI's call passes 0.
static spt_status guide_render(spt_context* ctx, spt_guide* g, const spt_prim* prims, int32_t n_prims,
                               const spt_camera* cam, const spt_params* p, int32_t sample_base,
                               int32_t sample_count, int force_k, void* stream) {
  if (!ctx || !g || !p) return fail(SPT_ERR_INVALID_ARG, "null context/guide/params");
  SPT_TRY(spt::shape_accepts(*g, p, sample_base, sample_count, "guide"));
  if (spt_context_device(ctx) != g->device)
    return fail(SPT_ERR_INVALID_ARG, "the guide and the context are on different devices");
  if (g->npix) {
    int32_t k = 0;
    SPT_TRY(spt_guide_window(ctx, prims, n_prims, cam, p, sample_base, sample_count, g->rec, &k, force_k,
                             g->flags, stream));
    g->lanes_per_pixel = k;
  }
  g->samples_done += sample_count;  // (a shard without rows only counts)
  return SPT_OK;
}

extern "C" spt_status spt_guide_render_async(spt_context* ctx, spt_guide* g, const spt_prim* prims,
                                             int32_t n_prims, const spt_camera* cam,
                                             const spt_params* p, int32_t sample_base,
                                             int32_t sample_count, void* stream) {
  return guide_render(ctx, g, prims, n_prims, cam, p, sample_base, sample_count, 0, stream);
}

#ifdef SPT_GUIDE_BENCH  // tools/guide_bench.py's library only: never in the shipped libspt.so
extern "C" spt_status spt_guide_bench_render_k(spt_context* ctx, spt_guide* g, const spt_prim* prims,
                                               int32_t n_prims, const spt_camera* cam,
                                               const spt_params* p, int32_t sample_base,
                                               int32_t sample_count, int32_t k, void* stream) {
  if (k < 1 || k > 64 || (k & (k - 1))) return fail(SPT_ERR_INVALID_ARG, "k: a power of two, 1..64");
  return guide_render(ctx, g, prims, n_prims, cam, p, sample_base, sample_count, k, stream);
}
#endif

extern "C" spt_status spt_guide_resolve(const spt_guide* g, float* albedo_dev, float* normal_dev,
                                        float* depth_dev, float* coverage_dev, void* stream) {
  if (!g) return fail(SPT_ERR_INVALID_ARG, "null guide");
  if (!g->npix || (!albedo_dev && !normal_dev && !depth_dev && !coverage_dev)) return SPT_OK;
  SPT_HIP(hipSetDevice(g->device));
  int full = 0;
  const float r = spt_film_math::resolve_factor(g->spp_total, g->samples_done, &full);
  hipLaunchKernelGGL(guide_resolve_kernel, dim3((unsigned)((g->npix + kBlock - 1) / kBlock)),
                     dim3(kBlock), 0, (hipStream_t)stream, (const long long*)g->rec, (uint32_t)g->npix,
                     g->samples_done, r, full, albedo_dev, normal_dev, depth_dev, coverage_dev);
  SPT_HIP(hipGetLastError());
  return SPT_OK;
}

extern "C" spt_status spt_guide_download(const spt_guide* g, int64_t* host_records, void* stream) {
  if (!g || (g->npix && !host_records)) return fail(SPT_ERR_INVALID_ARG, "null argument");
  if (!g->npix) return SPT_OK;
  return spt::copy_and_wait(g->device, host_records, g->rec, g->npix * 8 * sizeof(long long),
                            hipMemcpyDeviceToHost, stream);
}

// spt_guide.hip — the guide planes (include/spt.h, SPT_HAS_GUIDE): the object that holds a guide's
// integer records on the device, the resolve kernel and the spt_guide_* calls. The kernel that fills
// the records is guide_kernel (spt_kernel.hip), launched through the context (spt_context.cpp,
// spt_guide_window); the resolve's arithmetic is spt_guide.h's, shared with the CPU statement
// (spt_guide_host.cpp).
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/spt.h"
#include "spt_guide.h"

struct spt_guide {
  int device = 0;
  int32_t width = 0, rows = 0, spp_total = 0;
  int64_t samples_done = 0;
  // the params the guide was created for (a pass must bring the same ones)
  int32_t height = 0, tile_rows = 0, shard_index = 0, shard_count = 1;
  long long* rec = nullptr;  // [rows * width][8], device
  size_t npix = 0;
  int32_t lanes_per_pixel = 0;  // K of the last launch
  uint32_t flags = 0;           // SPT_GUIDE_*: the kind of record every pass adds (set at creation)
};

int spt_shard_row_count(const spt_params* p);  // spt_host.cpp
void spt_set_last_error(const std::string& msg);

namespace {

constexpr int kBlock = 256;
constexpr int32_t kMaxSpp = 1 << 24;  // slot 6 adds < 2^36 per sample: 2^24 samples stay below 2^63

spt_status fail(spt_status s, const std::string& msg) {
  spt_set_last_error(msg);
  return s;
}
#define GUIDE_HIP(call)                                                                 \
  do {                                                                                  \
    hipError_t e_ = (call);                                                             \
    if (e_ != hipSuccess)                                                               \
      return fail(e_ == hipErrorOutOfMemory ? SPT_ERR_OOM : SPT_ERR_HIP,                \
                  std::string(#call) + ": " + hipGetErrorString(e_));                   \
  } while (0)

int tile_rows_of(const spt_params* p) { return p->tile_rows > 0 ? p->tile_rows : 8; }

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
  if (p->width <= 0 || p->height <= 0 || p->spp <= 0)
    return fail(SPT_ERR_INVALID_ARG, "width/height/spp must be positive");
  if (p->spp > kMaxSpp) return fail(SPT_ERR_INVALID_ARG, "a guide takes at most 2^24 samples per pixel");
  if ((uint64_t)p->width * (uint64_t)p->height > 0x7FFFFFFFull)
    return fail(SPT_ERR_INVALID_ARG, "image too large for 32-bit pixel counters");
  if (p->shard_count < 1 || p->shard_index < 0 || p->shard_index >= p->shard_count || p->tile_rows < 0)
    return fail(SPT_ERR_INVALID_ARG, "bad shard_index/shard_count/tile_rows");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
    return fail(SPT_ERR_NO_DEVICE, "no HIP device");
  if (device < 0 || device >= count) return fail(SPT_ERR_INVALID_ARG, "bad device ordinal");
  GUIDE_HIP(hipSetDevice(device));
  spt_guide* g = new spt_guide();
  g->device = device;
  g->flags = flags;
  g->width = p->width;
  g->height = p->height;
  g->spp_total = p->spp;
  g->tile_rows = tile_rows_of(p);
  g->shard_index = p->shard_index;
  g->shard_count = p->shard_count;
  g->rows = spt_shard_row_count(p);
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
    GUIDE_HIP(hipSetDevice(g->device));
    GUIDE_HIP(hipMemsetAsync(g->rec, 0, g->npix * 8 * sizeof(long long), (hipStream_t)stream));
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
  if (p->width != g->width || p->height != g->height || p->spp != g->spp_total)
    return fail(SPT_ERR_INVALID_ARG, "width/height/spp differ from the guide's");
  if (p->tile_rows < 0 || tile_rows_of(p) != g->tile_rows || p->shard_index != g->shard_index ||
      p->shard_count != g->shard_count)
    return fail(SPT_ERR_INVALID_ARG, "the shard fields differ from the guide's");
  if (sample_base < 0 || sample_count < 1 || (int64_t)sample_base + sample_count > g->spp_total)
    return fail(SPT_ERR_INVALID_ARG, "sample window outside [0, spp)");
  if (g->samples_done + sample_count > g->spp_total)
    return fail(SPT_ERR_INVALID_ARG, "the guide would hold more than spp samples");
  if (spt_context_device(ctx) != g->device)
    return fail(SPT_ERR_INVALID_ARG, "the guide and the context are on different devices");
  if (g->npix) {
    int32_t k = 0;
    const spt_status st = spt_guide_window(ctx, prims, n_prims, cam, p, sample_base, sample_count,
                                           g->rec, &k, force_k, g->flags, stream);
    if (st != SPT_OK) return st;
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
  GUIDE_HIP(hipSetDevice(g->device));
  int full = 0;
  const float r = spt_film_math::resolve_factor(g->spp_total, g->samples_done, &full);
  hipLaunchKernelGGL(guide_resolve_kernel, dim3((unsigned)((g->npix + kBlock - 1) / kBlock)),
                     dim3(kBlock), 0, (hipStream_t)stream, (const long long*)g->rec, (uint32_t)g->npix,
                     g->samples_done, r, full, albedo_dev, normal_dev, depth_dev, coverage_dev);
  GUIDE_HIP(hipGetLastError());
  return SPT_OK;
}

extern "C" spt_status spt_guide_download(const spt_guide* g, int64_t* host_records, void* stream) {
  if (!g || (g->npix && !host_records)) return fail(SPT_ERR_INVALID_ARG, "null argument");
  if (!g->npix) return SPT_OK;
  GUIDE_HIP(hipSetDevice(g->device));
  GUIDE_HIP(hipMemcpyAsync(host_records, g->rec, g->npix * 8 * sizeof(long long), hipMemcpyDeviceToHost,
                           (hipStream_t)stream));
  GUIDE_HIP(hipStreamSynchronize((hipStream_t)stream));
  return SPT_OK;
}

// spt_film.hip — the resumable integer film (include/spt.h "progressive rendering").
//
// A render launch over a sample window [base, base + count) of an spp_total-sample image converts
// every sample with the image's one scale 2^31 / spp_total and sums in uint64 (spt_kernel.hip), so the
// windows' integers add up to the one-shot render's, whatever the split, the order, the context or
// the GPU. The film keeps those sums between launches: uint64[rows * w][3] in image pixel order.
//
//   accumulate  film += the pass's per-pixel sums (unit slots + stolen-range accumulator), and
//               optionally the resolved floats in the same pass (a progressive viewer reads the
//               film once)
//   resolve     film -> float: min((float)sum * 2^-31 [* r], 1), r = spp_total / samples_done
//               rounded once on the host (a preview; no factor for a full film)
//   merge       dst += src
//
// All three stream: one pass over the sums at 16 bytes per access (two sums, or four floats),
// 256 threads per block, no reuse -- HBM-bound. -ffp-contract=off (the Makefile) keeps the preview two
// separate multiplies, as spt_film_resolve_host and a numpy restatement compute it.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "spt_film.h"

int spt_shard_row_count(const spt_params* p);  // spt_host.cpp

namespace {

using u64 = unsigned long long;
constexpr int kBlock = 256;
constexpr uint32_t kQuadLanes = 192;  // 3 * kBlock sums per block / 4 per lane

__host__ __device__ __forceinline__ float film_resolve1(u64 v, float r, int full) {
  float f = (float)v * 0x1p-31f;
  if (!full) f = f * r;
  return f > 1.0f ? 1.0f : f;
}

// Every 16-byte load of a thread has landed before any of its registers is used. Measured on
// gfx950: the first form of the resolve kernel (tail loop and unaligned-store branch in the same
// kernel; the compiler started converting under a partial wait, vmcnt(1), and reused the address
// registers meanwhile) returned wrong floats for the second sum of ~0.5 % of its quads at 1024x768,
// whole waves, another set every launch, from correct sums. The same kernel with this full wait gave
// none in any launch, and so did the straight-line form below without it. The cause is not
// established (the ISA reads correct), so the kernels here are straight-line AND wait; they are
// HBM-bound, the wait costs nothing measurable. tests/test_gpu_film.py checks them at that size.
__device__ __forceinline__ void loads_landed(ulonglong2& a, ulonglong2& b) {
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(a.x), "+v"(a.y), "+v"(b.x), "+v"(b.y)::"memory");
}

// One sum of the accumulate's phase 2 (a run's unaligned head or tail).
__device__ __forceinline__ void acc_one(u64* __restrict__ film, const u64* __restrict__ accum,
                                        float* __restrict__ rgb, size_t e, u64 add, bool capped,
                                        float r, int full) {
  float f = __builtin_nanf("");
  if (!capped) {
    const u64 v = film[e] + add + accum[e];
    film[e] = v;
    f = film_resolve1(v, r, full);
  }
  if (rgb) rgb[e] = f;
}

// film += the launch's sums; rgb (optional) = the film resolved after the add.
//
// Phase 1, unit order: thread t sums the slots of unit-order pixel t (chunk j's slot at j * npix + t:
// coalesced, the order of finalize_slots_kernel) and parks the three sums in LDS at the place of its
// image pixel p = (t mod K) * scr_q + t / K, K = 2^scr_k. A block's 256 unit-order pixels are K runs
// of R = 256 / K consecutive image pixels (run a starts at pixel a * scr_q + blockIdx * R).
// Phase 2, image order: a run is up to 3 R consecutive sums of the film, of the stolen-range
// accumulator (pixel order too) and of rgb. Lanes 0..191 take four sums each from the run's first
// 32-byte boundary on (two 16-byte loads of the film and of the accumulator, two 16-byte stores, one
// float4 store); lanes 192..192+K-1 take their run's unaligned ends one sum at a time.
//
// Every thread reads the launch's runaway-guard word first: when the launch dropped units its slots
// hold an earlier launch's sums, so nothing is added and a given rgb is all NaN (never a partial
// image); the host takes the pass's samples back (spt_context_stats).
__global__ void __launch_bounds__(kBlock)
film_accumulate_kernel(const u64* __restrict__ accum, const u64* __restrict__ slots,
                       u64* __restrict__ film, float* __restrict__ rgb, uint32_t npix,
                       uint32_t n_chunks, uint32_t scr_k, uint32_t scr_q,
                       const u64* __restrict__ stats, float r, int full, int rgb_vec) {
  __shared__ u64 s_sum[3 * kBlock];
  const bool capped = stats[0] != 0;
  const uint32_t R = (uint32_t)kBlock >> scr_k;
  const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (!capped && t < npix) {
    u64 v0 = 0, v1 = 0, v2 = 0;
    for (uint32_t j = 0; j < n_chunks; ++j) {
      const u64* q = slots + 3ull * ((size_t)j * npix + t);
      v0 += q[0];
      v1 += q[1];
      v2 += q[2];
    }
    // blockIdx * 256 is a multiple of K: t mod K and t / K - blockIdx * R from threadIdx alone
    const uint32_t a = threadIdx.x & ((1u << scr_k) - 1u), bl = threadIdx.x >> scr_k;
    u64* d = s_sum + 3u * (a * R + bl);
    d[0] = v0;
    d[1] = v1;
    d[2] = v2;
  }
  __syncthreads();
  const uint32_t b0 = blockIdx.x * R;               // < scr_q: the grid is ceil(npix / 256)
  const uint32_t n = 3u * min(R, scr_q - b0);       // sums per run in this block
  const uint32_t i = threadIdx.x;
  if (i < kQuadLanes) {
    const uint32_t Q = kQuadLanes >> scr_k;         // quads per full run
    const uint32_t a = (i << scr_k) / kQuadLanes, j = i - a * Q;
    const size_t e0 = 3ull * ((size_t)a * scr_q + b0);
    const uint32_t h = min((0u - (uint32_t)e0) & 3u, n);  // sums before the 32-byte boundary
    if (j >= (n - h) / 4u) return;
    const uint32_t idx = h + 4u * j;
    const size_t e = e0 + idx;                      // a multiple of 4
    float4 f = make_float4(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""),
                           __builtin_nanf(""));
    if (!capped) {
      const u64* s = s_sum + 3u * a * R + idx;
      ulonglong2 f0 = *(const ulonglong2*)(film + e), f1 = *(const ulonglong2*)(film + e + 2);
      ulonglong2 a0 = *(const ulonglong2*)(accum + e), a1 = *(const ulonglong2*)(accum + e + 2);
      loads_landed(f0, f1);
      loads_landed(a0, a1);
      ulonglong2 v0, v1;
      v0.x = f0.x + a0.x + s[0];
      v0.y = f0.y + a0.y + s[1];
      v1.x = f1.x + a1.x + s[2];
      v1.y = f1.y + a1.y + s[3];
      *(ulonglong2*)(film + e) = v0;
      *(ulonglong2*)(film + e + 2) = v1;
      f = make_float4(film_resolve1(v0.x, r, full), film_resolve1(v0.y, r, full),
                      film_resolve1(v1.x, r, full), film_resolve1(v1.y, r, full));
    }
    if (rgb) {
      if (rgb_vec) {
        *(float4*)(rgb + e) = f;
      } else {  // a caller's buffer off the 16-byte grid
        rgb[e] = f.x;
        rgb[e + 1] = f.y;
        rgb[e + 2] = f.z;
        rgb[e + 3] = f.w;
      }
    }
  } else if (i < kQuadLanes + (1u << scr_k)) {
    const uint32_t a = i - kQuadLanes;
    const size_t e0 = 3ull * ((size_t)a * scr_q + b0);
    const uint32_t h = min((0u - (uint32_t)e0) & 3u, n);
    const uint32_t body_end = h + ((n - h) & ~3u);
    const u64* s = s_sum + 3u * a * R;
    for (uint32_t idx = 0; idx < h; ++idx)
      acc_one(film, accum, rgb, e0 + idx, capped ? 0ull : s[idx], capped, r, full);
    for (uint32_t idx = body_end; idx < n; ++idx)
      acc_one(film, accum, rgb, e0 + idx, capped ? 0ull : s[idx], capped, r, full);
  }
}

// film -> float over the whole quads of [0, n): four sums per thread, two 16-byte loads and one
// float4 store (rgb 16-byte aligned), straight-line. What is left -- the last n mod 4 sums, or
// everything when the caller's rgb is off the 16-byte grid -- goes through film_resolve_tail_kernel.
__global__ void __launch_bounds__(kBlock)
film_resolve_kernel(const u64* film, float* rgb, size_t n, float r, int full) {
  const size_t e = 4ull * ((size_t)blockIdx.x * kBlock + threadIdx.x);
  if (e + 4 <= n) {
    ulonglong2 v0 = *(const ulonglong2*)(film + e), v1 = *(const ulonglong2*)(film + e + 2);
    loads_landed(v0, v1);
    float4 f;
    f.x = film_resolve1(v0.x, r, full);
    f.y = film_resolve1(v0.y, r, full);
    f.z = film_resolve1(v1.x, r, full);
    f.w = film_resolve1(v1.y, r, full);
    *(float4*)(rgb + e) = f;
  }
}

// One sum per thread over [begin, n).
__global__ void __launch_bounds__(kBlock)
film_resolve_tail_kernel(const u64* film, float* rgb, size_t begin, size_t n, float r, int full) {
  const size_t e = begin + (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (e < n) rgb[e] = film_resolve1(film[e], r, full);
}

// dst += src over the whole quads of [0, n): four sums per thread, 16-byte loads and stores.
__global__ void __launch_bounds__(kBlock)
film_merge_kernel(u64* dst, const u64* src, size_t n) {
  const size_t e = 4ull * ((size_t)blockIdx.x * kBlock + threadIdx.x);
  if (e + 4 <= n) {
    ulonglong2 d0 = *(const ulonglong2*)(dst + e), d1 = *(const ulonglong2*)(dst + e + 2);
    ulonglong2 s0 = *(const ulonglong2*)(src + e), s1 = *(const ulonglong2*)(src + e + 2);
    loads_landed(d0, d1);
    loads_landed(s0, s1);
    d0.x += s0.x;
    d0.y += s0.y;
    d1.x += s1.x;
    d1.y += s1.y;
    *(ulonglong2*)(dst + e) = d0;
    *(ulonglong2*)(dst + e + 2) = d1;
  }
}

// ... and the last n mod 4 sums.
__global__ void __launch_bounds__(kBlock)
film_merge_tail_kernel(u64* dst, const u64* src, size_t begin, size_t n) {
  const size_t e = begin + (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (e < n) dst[e] += src[e];
}

spt_status fail(spt_status s, const std::string& msg) {
  spt_set_last_error(msg);
  return s;
}
#define FILM_HIP(call)                                                                  \
  do {                                                                                  \
    hipError_t e_ = (call);                                                             \
    if (e_ != hipSuccess)                                                               \
      return fail(e_ == hipErrorOutOfMemory ? SPT_ERR_OOM : SPT_ERR_HIP,                \
                  std::string(#call) + ": " + hipGetErrorString(e_));                   \
  } while (0)

int tile_rows_of(const spt_params* p) { return p->tile_rows > 0 ? p->tile_rows : 8; }

// The preview factor spp_total / samples_done, rounded once; *full = no factor at all.
float resolve_factor(int32_t spp_total, int64_t done, int* full) {
  *full = done == (int64_t)spp_total;
  return done > 0 ? (float)((double)spp_total / (double)done) : 0.0f;
}

unsigned quad_blocks(size_t n) { return (unsigned)(((n + 3) / 4 + kBlock - 1) / kBlock); }
unsigned tail_blocks(size_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }
bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" spt_status spt_film_create(int32_t device, const spt_params* p, spt_film** out) {
  if (!p || !out) return fail(SPT_ERR_INVALID_ARG, "null argument");
  if (p->width <= 0 || p->height <= 0 || p->spp <= 0)
    return fail(SPT_ERR_INVALID_ARG, "width/height/spp must be positive");
  if ((uint64_t)p->width * (uint64_t)p->height > 0xFFFFFFFFull)
    return fail(SPT_ERR_INVALID_ARG, "image too large for 32-bit pixel counters");
  if (p->shard_count < 1 || p->shard_index < 0 || p->shard_index >= p->shard_count || p->tile_rows < 0)
    return fail(SPT_ERR_INVALID_ARG, "bad shard_index/shard_count/tile_rows");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
    return fail(SPT_ERR_NO_DEVICE, "no HIP device");
  if (device < 0 || device >= count) return fail(SPT_ERR_INVALID_ARG, "bad device ordinal");
  FILM_HIP(hipSetDevice(device));
  spt_film* f = new spt_film();
  f->device = device;
  f->width = p->width;
  f->height = p->height;
  f->spp_total = p->spp;
  f->tile_rows = tile_rows_of(p);
  f->shard_index = p->shard_index;
  f->shard_count = p->shard_count;
  f->rows = spt_shard_row_count(p);
  f->n = 3ull * (size_t)f->rows * (size_t)f->width;
  if (f->n) {
    hipError_t e = hipMalloc(&f->sums, f->n * sizeof(u64));
    if (e == hipSuccess) e = hipMemset(f->sums, 0, f->n * sizeof(u64));
    if (e != hipSuccess) {
      if (f->sums) (void)hipFree(f->sums);
      delete f;
      return fail(SPT_ERR_OOM, std::string("film alloc: ") + hipGetErrorString(e));
    }
  }
  *out = f;
  return SPT_OK;
}

extern "C" spt_status spt_film_destroy(spt_film* f) {
  if (!f) return SPT_OK;
  if (f->last_ctx) spt_context_forget_film(f->last_ctx, f);
  if (f->sums) {
    (void)hipSetDevice(f->device);
    (void)hipFree(f->sums);
  }
  delete f;
  return SPT_OK;
}

extern "C" spt_status spt_film_info_get(const spt_film* f, spt_film_info* out) {
  if (!f || !out) return fail(SPT_ERR_INVALID_ARG, "null argument");
  out->width = f->width;
  out->rows = f->rows;
  out->spp_total = f->spp_total;
  out->samples_done = f->samples_done;
  return SPT_OK;
}

extern "C" spt_status spt_film_clear(spt_film* f, void* stream) {
  if (!f) return fail(SPT_ERR_INVALID_ARG, "null film");
  if (f->n) {
    FILM_HIP(hipSetDevice(f->device));
    FILM_HIP(hipMemsetAsync(f->sums, 0, f->n * sizeof(u64), (hipStream_t)stream));
  }
  f->samples_done = 0;
  return SPT_OK;
}

spt_status spt_film_accumulate(spt_film* f, spt_context* c, const unsigned long long* accum,
                               const unsigned long long* slots, float* rgb_dev, uint32_t npix,
                               uint32_t n_chunks, uint32_t scr_k, uint32_t scr_q,
                               const unsigned long long* stats, int32_t s_count, void* stream) {
  if (f->n != 3ull * npix) return fail(SPT_ERR_INVALID_ARG, "the film does not have the launch's pixels");
  int full = 0;
  const float r = resolve_factor(f->spp_total, f->samples_done + s_count, &full);
  hipLaunchKernelGGL(film_accumulate_kernel, dim3((npix + kBlock - 1) / kBlock), dim3(kBlock), 0,
                     (hipStream_t)stream, accum, slots, f->sums, rgb_dev, npix, n_chunks, scr_k, scr_q,
                     stats, r, full, (int)aligned16(rgb_dev));
  FILM_HIP(hipGetLastError());
  f->samples_done += s_count;
  if (f->last_ctx && f->last_ctx != c) spt_context_forget_film(f->last_ctx, f);
  f->last_ctx = c;
  return SPT_OK;
}

void spt_film_rollback(spt_film* f, const spt_context* c, int32_t s_count) {
  if (f->last_ctx == c && f->samples_done >= s_count) f->samples_done -= s_count;
}

void spt_film_forget_context(spt_film* f, const spt_context* c) {
  if (f->last_ctx == c) f->last_ctx = nullptr;
}

extern "C" spt_status spt_film_render_async(spt_context* ctx, spt_film* f, const spt_prim* prims,
                                            int32_t n_prims, const spt_camera* cam,
                                            const spt_params* p, int32_t sample_base,
                                            int32_t sample_count, float* rgb_dev, void* stream) {
  if (!ctx || !f || !p) return fail(SPT_ERR_INVALID_ARG, "null context/film/params");
  if (p->width != f->width || p->height != f->height || p->spp != f->spp_total)
    return fail(SPT_ERR_INVALID_ARG, "width/height/spp differ from the film's");
  if (p->tile_rows < 0 || tile_rows_of(p) != f->tile_rows || p->shard_index != f->shard_index ||
      p->shard_count != f->shard_count)
    return fail(SPT_ERR_INVALID_ARG, "the shard fields differ from the film's");
  if (sample_base < 0 || sample_count < 1 || (int64_t)sample_base + sample_count > f->spp_total)
    return fail(SPT_ERR_INVALID_ARG, "sample window outside [0, spp)");
  if (f->samples_done + sample_count > f->spp_total)
    return fail(SPT_ERR_INVALID_ARG, "the film would hold more than spp samples");
  const spt_status st = spt_render_window(ctx, prims, n_prims, cam, p, sample_base, sample_count,
                                          rgb_dev, f, stream);
  if (st != SPT_OK) return st;
  if (f->rows == 0) f->samples_done += sample_count;  // a shard without rows: nothing to add, still counted
  return SPT_OK;
}

extern "C" spt_status spt_film_resolve(const spt_film* f, float* rgb_dev, void* stream) {
  if (!f) return fail(SPT_ERR_INVALID_ARG, "null film");
  if (f->n == 0) return SPT_OK;
  if (!rgb_dev) return fail(SPT_ERR_INVALID_ARG, "null output");
  FILM_HIP(hipSetDevice(f->device));
  int full = 0;
  const float r = resolve_factor(f->spp_total, f->samples_done, &full);
  const size_t body = aligned16(rgb_dev) ? f->n & ~(size_t)3 : 0;  // sums the 16-byte kernel takes
  if (body) {
    hipLaunchKernelGGL(film_resolve_kernel, dim3(quad_blocks(body)), dim3(kBlock), 0,
                       (hipStream_t)stream, (const u64*)f->sums, rgb_dev, body, r, full);
    FILM_HIP(hipGetLastError());
  }
  if (body < f->n) {
    hipLaunchKernelGGL(film_resolve_tail_kernel, dim3(tail_blocks(f->n - body)), dim3(kBlock), 0,
                       (hipStream_t)stream, (const u64*)f->sums, rgb_dev, body, f->n, r, full);
    FILM_HIP(hipGetLastError());
  }
  return SPT_OK;
}

extern "C" spt_status spt_film_merge(spt_film* dst, const spt_film* src, void* stream) {
  if (!dst || !src || dst == src) return fail(SPT_ERR_INVALID_ARG, "merge needs two films");
  if (dst->width != src->width || dst->rows != src->rows || dst->spp_total != src->spp_total)
    return fail(SPT_ERR_INVALID_ARG, "films of unequal width/rows/spp");
  if (dst->device != src->device)
    return fail(SPT_ERR_INVALID_ARG, "films on different devices: download one and upload it beside the other");
  if (dst->samples_done + src->samples_done > dst->spp_total)
    return fail(SPT_ERR_INVALID_ARG, "the merged film would hold more than spp samples");
  if (dst->n) {
    FILM_HIP(hipSetDevice(dst->device));
    const size_t body = dst->n & ~(size_t)3;
    if (body) {
      hipLaunchKernelGGL(film_merge_kernel, dim3(quad_blocks(body)), dim3(kBlock), 0,
                         (hipStream_t)stream, dst->sums, (const u64*)src->sums, body);
      FILM_HIP(hipGetLastError());
    }
    if (body < dst->n) {
      hipLaunchKernelGGL(film_merge_tail_kernel, dim3(tail_blocks(dst->n - body)), dim3(kBlock), 0,
                         (hipStream_t)stream, dst->sums, (const u64*)src->sums, body, dst->n);
      FILM_HIP(hipGetLastError());
    }
  }
  dst->samples_done += src->samples_done;
  return SPT_OK;
}

extern "C" spt_status spt_film_download(const spt_film* f, uint64_t* host_sums, void* stream) {
  if (!f) return fail(SPT_ERR_INVALID_ARG, "null film");
  if (f->n == 0) return SPT_OK;
  if (!host_sums) return fail(SPT_ERR_INVALID_ARG, "null output");
  FILM_HIP(hipSetDevice(f->device));
  FILM_HIP(hipMemcpyAsync(host_sums, f->sums, f->n * sizeof(u64), hipMemcpyDeviceToHost,
                          (hipStream_t)stream));
  FILM_HIP(hipStreamSynchronize((hipStream_t)stream));
  return SPT_OK;
}

extern "C" spt_status spt_film_upload(spt_film* f, const uint64_t* host_sums, int64_t samples_done,
                                      void* stream) {
  if (!f) return fail(SPT_ERR_INVALID_ARG, "null film");
  if (samples_done < 0 || samples_done > f->spp_total)
    return fail(SPT_ERR_INVALID_ARG, "samples_done outside [0, spp]");
  if (f->n) {
    if (!host_sums) return fail(SPT_ERR_INVALID_ARG, "null input");
    FILM_HIP(hipSetDevice(f->device));
    FILM_HIP(hipMemcpyAsync(f->sums, host_sums, f->n * sizeof(u64), hipMemcpyHostToDevice,
                            (hipStream_t)stream));
    FILM_HIP(hipStreamSynchronize((hipStream_t)stream));
  }
  f->samples_done = samples_done;
  return SPT_OK;
}

extern "C" spt_status spt_film_resolve_host(const uint64_t* sums, const spt_film_info* info,
                                            float* rgb_out) {
  if (!info) return fail(SPT_ERR_INVALID_ARG, "null info");
  if (info->width <= 0 || info->rows < 0 || info->spp_total <= 0 || info->samples_done < 0 ||
      info->samples_done > info->spp_total)
    return fail(SPT_ERR_INVALID_ARG, "bad film info");
  const size_t n = 3ull * (size_t)info->rows * (size_t)info->width;
  if (n == 0) return SPT_OK;
  if (!sums || !rgb_out) return fail(SPT_ERR_INVALID_ARG, "null sums/output");
  int full = 0;
  const float r = resolve_factor(info->spp_total, info->samples_done, &full);
  for (size_t k = 0; k < n; ++k) rgb_out[k] = film_resolve1((u64)sums[k], r, full);
  return SPT_OK;
}

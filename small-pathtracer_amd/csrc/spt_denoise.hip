// spt_denoise.hip — the edge-stopping a-trous filter on the device (include/spt.h, SPT_HAS_DENOISE):
// the denoiser object that owns the scratch, the pack, variance and a-trous kernels and the
// spt_denoise_* / spt_film_denoise calls. The arithmetic is spt_denoise.h's, shared with the CPU
// statement (spt_denoise_host.cpp): the kernels only decide which lane takes which pixel.
#include <hip/hip_runtime.h>

#include <initializer_list>

#include "spt_denoise.h"
#include "spt_film.h"
#include "spt_guide.h"

using namespace spt_denoise_math;
using spt::fail;

struct spt_denoiser {
  int device = 0;
  int32_t width = 0, height = 0;
  size_t npix = 0;
  void* base = nullptr;  // the one allocation the planes below are carved from
  f4 *cv[2] = {nullptr, nullptr}, *nz = nullptr, *av = nullptr;
  float2* grad = nullptr;
  // the film path's planes (spt_film_denoise): rgb, se, albedo, normal (3 floats each), depth (1)
  float *rgb = nullptr, *se = nullptr, *albedo = nullptr, *normal = nullptr, *depth = nullptr;
};

namespace {

constexpr int kTileX = 64, kTileY = 4, kBlock = kTileX * kTileY;  // a wave covers 64 consecutive x

// The block's tile -> this lane's pixel. Blocks are a 1-D grid over the tiles, rows of tiles first.
__device__ __forceinline__ bool pixel_of(int32_t w, int32_t h, int32_t* x, int32_t* y) {
  const uint32_t tiles_x = ((uint32_t)w + kTileX - 1) / kTileX;
  const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  *x = (int32_t)(tx * kTileX + (threadIdx.x & (kTileX - 1)));
  *y = (int32_t)(ty * kTileY + threadIdx.x / kTileX);
  return *x < w && *y < h;
}

struct DevPlanes {
  const f4 *cv_, *nz_, *av_;
  int32_t w;
  __device__ __forceinline__ f4 cv(int32_t x, int32_t y) const { return cv_[(size_t)y * w + x]; }
  __device__ __forceinline__ f4 nz(int32_t x, int32_t y) const { return nz_[(size_t)y * w + x]; }
  __device__ __forceinline__ f4 av(int32_t x, int32_t y) const { return av_[(size_t)y * w + x]; }
  __device__ __forceinline__ float v(int32_t x, int32_t y) const { return cv_[(size_t)y * w + x].w; }
};

// Pack: five planes in, the packed planes and the depth gradient out.
__global__ void __launch_bounds__(kBlock)
denoise_pack_kernel(const float* __restrict__ rgb, const float* __restrict__ se,
                    const float* __restrict__ albedo, const float* __restrict__ normal,
                    const float* __restrict__ depth, int32_t w, int32_t h, Args A, f4* __restrict__ cv,
                    f4* __restrict__ nz, f4* __restrict__ av, float2* __restrict__ grad) {
  int32_t x, y;
  if (!pixel_of(w, h, &x, &y)) return;
  const size_t i = (size_t)y * w + x;
  const float c[3] = {rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]};
  const float e[3] = {se[3 * i], se[3 * i + 1], se[3 * i + 2]};
  const float a[3] = {albedo[3 * i], albedo[3 * i + 1], albedo[3 * i + 2]};
  const float z = depth[i];
  cv[i] = prepare(c, e, a, A);
  nz[i] = f4{normal[3 * i], normal[3 * i + 1], normal[3 * i + 2], z};
  av[i] = f4{a[0], a[1], a[2], 0.0f};
  const float zl = x > 0 ? depth[i - 1] : 0.0f, zr = x < w - 1 ? depth[i + 1] : 0.0f;
  const float zu = y > 0 ? depth[i - w] : 0.0f, zd = y < h - 1 ? depth[i + w] : 0.0f;
  grad[i] = make_float2(gradient(x, w, zl, z, zr), gradient(y, h, zu, z, zd));
}

// vt of the current v into av.w, before the iteration that reads it at both ends of every tap.
__global__ void __launch_bounds__(kBlock)
denoise_variance_kernel(const f4* __restrict__ cv, f4* __restrict__ av, int32_t w, int32_t h) {
  int32_t x, y;
  if (!pixel_of(w, h, &x, &y)) return;
  const DevPlanes P{cv, nullptr, nullptr, w};
  av[(size_t)y * w + x].w = variance_filter(P, x, y, w, h);
}

// One iteration: a pixel per lane, three 16-byte loads per tap (a wave's lanes read one contiguous
// row segment), the bounds test per tap. LAST: the finish instead of the other ping-pong plane.
template <bool LAST>
__global__ void __launch_bounds__(kBlock)
denoise_atrous_kernel(const f4* __restrict__ cv, const f4* __restrict__ nz, const f4* __restrict__ av,
                      const float2* __restrict__ grad, int32_t w, int32_t h, int32_t step, Args A,
                      f4* __restrict__ cv_out, float* __restrict__ out, float* __restrict__ se_out) {
  int32_t x, y;
  if (!pixel_of(w, h, &x, &y)) return;
  const size_t i = (size_t)y * w + x;
  const DevPlanes P{cv, nz, av, w};
  const float2 g = grad[i];
  const f4 r = iterate(P, x, y, w, h, step, g.x, g.y, A);
  if constexpr (LAST)
    finish(r, av[i], A, out + 3 * i, se_out ? se_out + 3 * i : nullptr);
  else
    cv_out[i] = r;
}

// The LDS-tiled form of one iteration, for the steps whose halo (2 * STEP pixels) is smaller than the
// tile: a block stages its 32 x 8 tile plus halo of the three packed planes in LDS (places outside the
// image are left unwritten: the per-tap bounds test is the image's, so they are never read), then every
// lane runs the same iterate() on the staged copy. Same operations in the same order: same bits.
constexpr int kLdsX = 32, kLdsY = 8;

template <int STEP>
struct LdsPlanes {
  static constexpr int kW = kLdsX + 4 * STEP;
  const f4 *cv_, *nz_, *av_;
  int32_t x0, y0;  // the image position of the staged region's first element
  __device__ __forceinline__ f4 cv(int32_t x, int32_t y) const { return cv_[(y - y0) * kW + (x - x0)]; }
  __device__ __forceinline__ f4 nz(int32_t x, int32_t y) const { return nz_[(y - y0) * kW + (x - x0)]; }
  __device__ __forceinline__ f4 av(int32_t x, int32_t y) const { return av_[(y - y0) * kW + (x - x0)]; }
};

template <int STEP, bool LAST>
__global__ void __launch_bounds__(kBlock)
denoise_atrous_lds_kernel(const f4* __restrict__ cv, const f4* __restrict__ nz, const f4* __restrict__ av,
                          const float2* __restrict__ grad, int32_t w, int32_t h, Args A,
                          f4* __restrict__ cv_out, float* __restrict__ out, float* __restrict__ se_out) {
  constexpr int kHalo = 2 * STEP, kW = kLdsX + 2 * kHalo, kH = kLdsY + 2 * kHalo, kN = kW * kH;
  __shared__ f4 s_cv[kN], s_nz[kN], s_av[kN];
  const uint32_t tiles_x = ((uint32_t)w + kLdsX - 1) / kLdsX;
  const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int32_t x0 = (int32_t)(tx * kLdsX) - kHalo, y0 = (int32_t)(ty * kLdsY) - kHalo;
  for (int e = (int)threadIdx.x; e < kN; e += kBlock) {
    const int ly = e / kW, lx = e - ly * kW;
    const int32_t gx = x0 + lx, gy = y0 + ly;
    if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
      const size_t g = (size_t)gy * w + gx;
      s_cv[e] = cv[g];
      s_nz[e] = nz[g];
      s_av[e] = av[g];
    }
  }
  __syncthreads();
  const int32_t x = (int32_t)(tx * kLdsX + (threadIdx.x & (kLdsX - 1)));
  const int32_t y = (int32_t)(ty * kLdsY + threadIdx.x / kLdsX);
  if (x >= w || y >= h) return;
  const size_t i = (size_t)y * w + x;
  const LdsPlanes<STEP> P{s_cv, s_nz, s_av, x0, y0};
  const float2 g = grad[i];
  const f4 r = iterate(P, x, y, w, h, STEP, g.x, g.y, A);
  if constexpr (LAST)
    finish(r, s_av[(y - y0) * kW + (x - x0)], A, out + 3 * i, se_out ? se_out + 3 * i : nullptr);
  else
    cv_out[i] = r;
}

size_t tiles_of(int32_t w, int32_t h, int tile_x, int tile_y) {
  return (((size_t)w + tile_x - 1) / tile_x) * (((size_t)h + tile_y - 1) / tile_y);
}
// A launch holds fewer than 2^32 threads: both tilings must fit (spt_denoiser_create refuses otherwise).
constexpr size_t kMaxTiles = 0xFFFFFFFFull / kBlock;

// Which form an iteration takes: 0 = by step (the tiled form for steps 1 and 2), 1 = plain loads
// always, 2 = the tiled form where it exists. Only the bench library can change it.
int g_form = 0;

// One a-trous iteration of step `step` from `cur` into cv_out (or, last, into out / se_out).
void launch_atrous(const spt_denoiser* dn, const f4* cur, int32_t step, bool last, const Args& A,
                   f4* cv_out, float* out, float* se_out, int form, hipStream_t stream) {
  const int32_t w = dn->width, h = dn->height;
  const f4 *nz = dn->nz, *av = dn->av;
  const float2* grad = dn->grad;
  const dim3 block(kBlock);
  if (form != 1 && step <= 2) {
    const dim3 grid((unsigned)tiles_of(w, h, kLdsX, kLdsY));
#define DN_LDS(S, L) hipLaunchKernelGGL((denoise_atrous_lds_kernel<S, L>), grid, block, 0, stream, cur, nz, av, grad, w, h, A, cv_out, out, se_out)
    if (step == 1 && last) DN_LDS(1, true);
    else if (step == 1) DN_LDS(1, false);
    else if (last) DN_LDS(2, true);
    else DN_LDS(2, false);
#undef DN_LDS
    return;
  }
  const dim3 grid((unsigned)tiles_of(w, h, kTileX, kTileY));
  if (last)
    hipLaunchKernelGGL(denoise_atrous_kernel<true>, grid, block, 0, stream, cur, nz, av, grad, w, h, step, A,
                       cv_out, out, se_out);
  else
    hipLaunchKernelGGL(denoise_atrous_kernel<false>, grid, block, 0, stream, cur, nz, av, grad, w, h, step, A,
                       cv_out, out, se_out);
}

// The filter of five device planes, already validated.
spt_status run(spt_denoiser* dn, const float* rgb, const float* se, const float* albedo,
               const float* normal, const float* depth, const spt_denoise_params* p, float* out,
               float* se_out, hipStream_t stream) {
  const size_t bytes = dn->npix * 3 * sizeof(float);
  if (p->iterations == 0) {
    SPT_HIP(hipMemcpyAsync(out, rgb, bytes, hipMemcpyDeviceToDevice, stream));
    if (se_out) SPT_HIP(hipMemcpyAsync(se_out, se, bytes, hipMemcpyDeviceToDevice, stream));
    return SPT_OK;
  }
  const Args A = make_args(p);
  const dim3 grid((unsigned)tiles_of(dn->width, dn->height, kTileX, kTileY)), block(kBlock);
  const int32_t w = dn->width, h = dn->height;
  hipLaunchKernelGGL(denoise_pack_kernel, grid, block, 0, stream, rgb, se, albedo, normal, depth, w, h,
                     A, dn->cv[0], dn->nz, dn->av, dn->grad);
  for (int32_t it = 0; it < p->iterations; ++it) {
    const f4* cur = dn->cv[it & 1];
    hipLaunchKernelGGL(denoise_variance_kernel, grid, block, 0, stream, cur, dn->av, w, h);
    const bool last = it == p->iterations - 1;
    launch_atrous(dn, cur, (int32_t)1 << it, last, A, last ? nullptr : dn->cv[(it + 1) & 1],
                  last ? out : nullptr, last ? se_out : nullptr, g_form, stream);
  }
  SPT_HIP(hipGetLastError());
  return SPT_OK;
}

spt_status check_call(const spt_denoiser* dn, const spt_denoise_params* p, const float* out,
                      const float* se_out, std::initializer_list<const float*> inputs) {
  if (!dn) return fail(SPT_ERR_INVALID_ARG, "null denoiser");
  if (const char* e = params_error(p)) return fail(SPT_ERR_INVALID_ARG, std::string("denoise: ") + e);
  if (!out) return fail(SPT_ERR_INVALID_ARG, "denoise: null output plane");
  if (se_out == out) return fail(SPT_ERR_INVALID_ARG, "denoise: out and se_out are one plane");
  for (const float* in : inputs) {
    if (!in) return fail(SPT_ERR_INVALID_ARG, "denoise: null plane");
    if (in == out || (se_out && in == se_out))
      return fail(SPT_ERR_INVALID_ARG, "denoise: an output plane is an input plane");
  }
  return SPT_OK;
}

}  // namespace

extern "C" spt_status spt_denoiser_create(int32_t device, int32_t width, int32_t height,
                                          spt_denoiser** out) {
  if (!out) return fail(SPT_ERR_INVALID_ARG, "null argument");
  if (width <= 0 || height <= 0 || (int64_t)width * (int64_t)height > kMaxPixels)
    return fail(SPT_ERR_INVALID_ARG, "denoiser: width/height must be positive and hold at most 2^31 - 1 pixels");
  if (tiles_of(width, height, kTileX, kTileY) > kMaxTiles || tiles_of(width, height, kLdsX, kLdsY) > kMaxTiles)
    return fail(SPT_ERR_INVALID_ARG, "denoiser: the image is too narrow or too flat for one launch (spt.h)");
  SPT_TRY(spt::open_device(device));
  spt_denoiser* dn = new spt_denoiser();
  dn->device = device;
  dn->width = width;
  dn->height = height;
  dn->npix = (size_t)width * (size_t)height;
  // 4 f4 planes, the gradient, 13 floats of film planes: 124 bytes per pixel, 16-byte planes first
  const size_t n = dn->npix, n4 = (n + 3) & ~(size_t)3;  // float planes padded to 16 bytes
  const size_t bytes = n * (4 * sizeof(f4) + sizeof(float2)) + (n & 1) * sizeof(float2) +
                       (4 * 3 * n4 + n4) * sizeof(float);
  const hipError_t e = hipMalloc(&dn->base, bytes);
  if (e != hipSuccess) {
    delete dn;
    return fail(SPT_ERR_OOM, std::string("denoiser alloc: ") + hipGetErrorString(e));
  }
  char* b = (char*)dn->base;
  dn->cv[0] = (f4*)b;
  dn->cv[1] = dn->cv[0] + n;
  dn->nz = dn->cv[1] + n;
  dn->av = dn->nz + n;
  dn->grad = (float2*)(dn->av + n);
  dn->rgb = (float*)(dn->grad + n + (n & 1));
  dn->se = dn->rgb + 3 * n4;
  dn->albedo = dn->se + 3 * n4;
  dn->normal = dn->albedo + 3 * n4;
  dn->depth = dn->normal + 3 * n4;
  *out = dn;
  return SPT_OK;
}

extern "C" spt_status spt_denoiser_destroy(spt_denoiser* dn) {
  if (!dn) return SPT_OK;
  if (dn->base) {
    (void)hipSetDevice(dn->device);
    (void)hipFree(dn->base);
  }
  delete dn;
  return SPT_OK;
}

extern "C" spt_status spt_denoise_async(spt_denoiser* dn, const float* rgb_dev, const float* se_dev,
                                        const float* albedo_dev, const float* normal_dev,
                                        const float* depth_dev, const spt_denoise_params* params,
                                        float* out_dev, float* se_out_dev, void* stream) {
  SPT_TRY(check_call(dn, params, out_dev, se_out_dev, {rgb_dev, se_dev, albedo_dev, normal_dev, depth_dev}));
  SPT_HIP(hipSetDevice(dn->device));
  return run(dn, rgb_dev, se_dev, albedo_dev, normal_dev, depth_dev, params, out_dev, se_out_dev,
             (hipStream_t)stream);
}

extern "C" spt_status spt_film_denoise(const spt_film* film, const spt_guide* guide, spt_denoiser* dn,
                                       const spt_denoise_params* params, float* out_dev,
                                       float* se_out_dev, void* stream) {
  if (!film || !guide) return fail(SPT_ERR_INVALID_ARG, "film_denoise: null film or guide");
  SPT_TRY(check_call(dn, params, out_dev, se_out_dev, {}));
  if (!film->batch) return fail(SPT_ERR_INVALID_ARG, "film_denoise: not a noise film");
  if (film->batches_done < 2)
    return fail(SPT_ERR_INVALID_ARG, "film_denoise: the error needs at least two batches");
  if (guide->samples_done == 0) return fail(SPT_ERR_INVALID_ARG, "film_denoise: the guide holds no sample");
  if (film->shard_count > 1)
    return fail(SPT_ERR_INVALID_ARG,
                "film_denoise: a shard's rows are not image neighbours; gather the planes and call spt_denoise_async");
  if (film->width != dn->width || film->rows != dn->height || !spt::shape_equal(*film, *guide))
    return fail(SPT_ERR_INVALID_ARG, "film_denoise: the film's or the guide's size differs from the denoiser's");
  if (film->device != dn->device)
    return fail(SPT_ERR_INVALID_ARG, "film_denoise: the film and the denoiser are on different devices");
  SPT_TRY(spt_film_resolve(film, dn->rgb, stream));
  SPT_TRY(spt_film_noise_map(film, dn->se, stream));
  SPT_TRY(spt_guide_resolve(guide, dn->albedo, dn->normal, dn->depth, nullptr, stream));
  SPT_HIP(hipSetDevice(dn->device));
  return run(dn, dn->rgb, dn->se, dn->albedo, dn->normal, dn->depth, params, out_dev, se_out_dev,
             (hipStream_t)stream);
}

#ifdef SPT_DENOISE_BENCH  // tools/denoise_bench.py's library only: never in the shipped libspt.so
// 0 = by step, 1 = plain loads always, 2 = the tiled form where it exists.
extern "C" spt_status spt_denoise_bench_form(int32_t form) {
  if (form < 0 || form > 2) return fail(SPT_ERR_INVALID_ARG, "form: 0, 1 or 2");
  g_form = form;
  return SPT_OK;
}
// One launch of one kernel on the denoiser's scratch, for a timing of that kernel alone. which: 0 the
// pack of the five planes, 1 the variance pass over cv[0], 2 an a-trous pass cv[0] -> cv[1], 3 the
// a-trous pass with the finish fused in, cv[0] -> out / se_out. form as above (plain or tiled).
extern "C" spt_status spt_denoise_bench_kernel(spt_denoiser* dn, int32_t which, int32_t step, int32_t form,
                                               const float* rgb, const float* se, const float* albedo,
                                               const float* normal, const float* depth,
                                               const spt_denoise_params* params, float* out, float* se_out,
                                               void* stream_v) {
  if (!dn || params_error(params) || which < 0 || which > 3 || step < 1 || step > 32 || (step & (step - 1)) ||
      form < 1 || form > 2 || (form == 2 && step > 2))
    return fail(SPT_ERR_INVALID_ARG, "bench_kernel: bad argument");
  hipStream_t stream = (hipStream_t)stream_v;
  const Args A = make_args(params);
  const dim3 grid((unsigned)tiles_of(dn->width, dn->height, kTileX, kTileY)), block(kBlock);
  SPT_HIP(hipSetDevice(dn->device));
  if (which == 0)
    hipLaunchKernelGGL(denoise_pack_kernel, grid, block, 0, stream, rgb, se, albedo, normal, depth, dn->width,
                       dn->height, A, dn->cv[0], dn->nz, dn->av, dn->grad);
  else if (which == 1)
    hipLaunchKernelGGL(denoise_variance_kernel, grid, block, 0, stream, (const f4*)dn->cv[0], dn->av,
                       dn->width, dn->height);
  else
    launch_atrous(dn, dn->cv[0], step, which == 3, A, which == 3 ? nullptr : dn->cv[1],
                  which == 3 ? out : nullptr, which == 3 ? se_out : nullptr, form, stream);
  SPT_HIP(hipGetLastError());
  return SPT_OK;
}
#endif

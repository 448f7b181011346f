// spt_denoise.hip — the edge-stopping a-trous filter on the device (include/spt.h, SPT_HAS_DENOISE):
// the denoiser object that owns the scratch, the pack, variance and a-trous kernels and the
// spt_denoise_* / spt_film_denoise calls, and the two-half filter (SPT_HAS_DENOISE_PAIR): its pack,
// variance, a-trous and summary kernels, its scratch, and the spt_denoise_pair_* / spt_film_pair_denoise
// calls, and the filter bank (SPT_HAS_DENOISE_BANK): the halves-storing pair finish, the error, smoothing,
// blend and summary kernels, its scratch, and the spt_denoise_bank_* / spt_film_pair_denoise_bank calls.
// The arithmetic is spt_denoise.h's, shared with the CPU statement (spt_denoise_host.cpp): the
// kernels only decide which lane takes which pixel.
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
  // the pair scratch (SPT_HAS_DENOISE_PAIR), allocated by the first pair call: half B's ping-pong
  // planes and vt, the second film's rgb and se, the summary's partials and total
  void* pair_base = nullptr;
  f4* cb[2] = {nullptr, nullptr};
  float *vtb = nullptr, *rgb_b = nullptr, *se_b = nullptr;
  double* parts = nullptr;
  uint32_t n_parts = 0;
  // the bank scratch (SPT_HAS_DENOISE_BANK), allocated by the first bank call: the halves' results o^A and
  // o^B of the candidate in flight, the four out_k planes, the ping-pong planes of the four error
  // estimates, the bank summary's partials and total
  void* bank_base = nullptr;
  f4* bm[2] = {nullptr, nullptr};
  float *oa = nullptr, *ob = nullptr, *outk = nullptr;
  size_t outk_stride = 0;  // floats between two candidates' out planes
  double* bank_parts = nullptr;
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

// ---- the two-half filter (SPT_HAS_DENOISE_PAIR): iterate_pair() on the 64 x 4 tiling ----

struct DevPairPlanes {
  const f4 *ca_, *cb_, *nz_, *av_;
  const float* vtb_;
  int32_t w;
  __device__ __forceinline__ f4 ca(int32_t x, int32_t y) const { return ca_[(size_t)y * w + x]; }
  __device__ __forceinline__ f4 cb(int32_t x, int32_t y) const { return cb_[(size_t)y * w + x]; }
  __device__ __forceinline__ f4 nz(int32_t x, int32_t y) const { return nz_[(size_t)y * w + x]; }
  __device__ __forceinline__ f4 av(int32_t x, int32_t y) const { return av_[(size_t)y * w + x]; }
  __device__ __forceinline__ float vtb(int32_t x, int32_t y) const { return vtb_[(size_t)y * w + x]; }
};

// Pack of the pair: seven planes in; both halves' (c, v), the packed guides and the gradient out.
__global__ void __launch_bounds__(kBlock)
denoise_pair_pack_kernel(const float* __restrict__ rgb_a, const float* __restrict__ se_a,
                         const float* __restrict__ rgb_b, const float* __restrict__ se_b,
                         const float* __restrict__ albedo, const float* __restrict__ normal,
                         const float* __restrict__ depth, int32_t w, int32_t h, Args A, f4* __restrict__ ca,
                         f4* __restrict__ cb, f4* __restrict__ nz, f4* __restrict__ av,
                         float2* __restrict__ grad) {
  int32_t x, y;
  if (!pixel_of(w, h, &x, &y)) return;
  const size_t i = (size_t)y * w + x;
  const float a[3] = {albedo[3 * i], albedo[3 * i + 1], albedo[3 * i + 2]};
  const float c0[3] = {rgb_a[3 * i], rgb_a[3 * i + 1], rgb_a[3 * i + 2]};
  const float e0[3] = {se_a[3 * i], se_a[3 * i + 1], se_a[3 * i + 2]};
  const float c1[3] = {rgb_b[3 * i], rgb_b[3 * i + 1], rgb_b[3 * i + 2]};
  const float e1[3] = {se_b[3 * i], se_b[3 * i + 1], se_b[3 * i + 2]};
  const float z = depth[i];
  ca[i] = prepare(c0, e0, a, A);
  cb[i] = prepare(c1, e1, a, A);
  nz[i] = f4{normal[3 * i], normal[3 * i + 1], normal[3 * i + 2], z};
  av[i] = f4{a[0], a[1], a[2], 0.0f};
  const float zl = x > 0 ? depth[i - 1] : 0.0f, zr = x < w - 1 ? depth[i + 1] : 0.0f;
  const float zu = y > 0 ? depth[i - w] : 0.0f, zd = y < h - 1 ? depth[i + w] : 0.0f;
  grad[i] = make_float2(gradient(x, w, zl, z, zr), gradient(y, h, zu, z, zd));
}

// vt of both halves' current v: half A's into av.w, half B's into its own plane.
__global__ void __launch_bounds__(kBlock)
denoise_pair_variance_kernel(const f4* __restrict__ ca, const f4* __restrict__ cb, f4* __restrict__ av,
                             float* __restrict__ vtb, int32_t w, int32_t h) {
  int32_t x, y;
  if (!pixel_of(w, h, &x, &y)) return;
  const DevPlanes PA{ca, nullptr, nullptr, w}, PB{cb, nullptr, nullptr, w};
  av[(size_t)y * w + x].w = variance_filter(PA, x, y, w, h);
  vtb[(size_t)y * w + x] = variance_filter(PB, x, y, w, h);
}

// One iteration of both halves: a pixel per lane, five loads per tap (four of 16 bytes, vt^B's 4), the
// bounds test per tap. LAST: the pair's finish instead of the other ping-pong planes.
template <bool LAST>
__global__ void __launch_bounds__(kBlock)
denoise_atrous_pair_kernel(const f4* __restrict__ ca, const f4* __restrict__ cb, const f4* __restrict__ nz,
                           const f4* __restrict__ av, const float* __restrict__ vtb,
                           const float2* __restrict__ grad, int32_t w, int32_t h, int32_t step, Args A,
                           int32_t own, f4* __restrict__ ca_out, f4* __restrict__ cb_out,
                           float* __restrict__ out, float* __restrict__ se_out, float* __restrict__ diff) {
  int32_t x, y;
  if (!pixel_of(w, h, &x, &y)) return;
  const size_t i = (size_t)y * w + x;
  const DevPairPlanes P{ca, cb, nz, av, vtb, w};
  const float2 g = grad[i];
  f4 ra, rb;
  iterate_pair(P, x, y, w, h, step, g.x, g.y, A, own != 0, &ra, &rb);
  if constexpr (LAST) {
    finish_pair(ra, rb, av[i], A, out + 3 * i, se_out ? se_out + 3 * i : nullptr, diff ? diff + 3 * i : nullptr);
  } else {
    ca_out[i] = ra;
    cb_out[i] = rb;
  }
}

// The LDS-tiled form of one pair iteration, for steps 1 and 2 (as denoise_atrous_lds_kernel): the 32 x 8
// tile plus halo of the four packed planes and vt^B staged in LDS (29 KB at step 1, 43.5 KB at step 2),
// then the same iterate_pair() on the staged copy. Same operations in the same order: same bits.
template <int STEP>
struct LdsPairPlanes {
  static constexpr int kW = kLdsX + 4 * STEP;
  const f4 *ca_, *cb_, *nz_, *av_;
  const float* vtb_;
  int32_t x0, y0;  // the image position of the staged region's first element
  __device__ __forceinline__ f4 ca(int32_t x, int32_t y) const { return ca_[(y - y0) * kW + (x - x0)]; }
  __device__ __forceinline__ f4 cb(int32_t x, int32_t y) const { return cb_[(y - y0) * kW + (x - x0)]; }
  __device__ __forceinline__ f4 nz(int32_t x, int32_t y) const { return nz_[(y - y0) * kW + (x - x0)]; }
  __device__ __forceinline__ f4 av(int32_t x, int32_t y) const { return av_[(y - y0) * kW + (x - x0)]; }
  __device__ __forceinline__ float vtb(int32_t x, int32_t y) const { return vtb_[(y - y0) * kW + (x - x0)]; }
};

template <int STEP, bool LAST>
__global__ void __launch_bounds__(kBlock)
denoise_atrous_pair_lds_kernel(const f4* __restrict__ ca, const f4* __restrict__ cb, const f4* __restrict__ nz,
                               const f4* __restrict__ av, const float* __restrict__ vtb,
                               const float2* __restrict__ grad, int32_t w, int32_t h, Args A, int32_t own,
                               f4* __restrict__ ca_out, f4* __restrict__ cb_out, float* __restrict__ out,
                               float* __restrict__ se_out, float* __restrict__ diff) {
  constexpr int kHalo = 2 * STEP, kW = kLdsX + 2 * kHalo, kH = kLdsY + 2 * kHalo, kN = kW * kH;
  __shared__ f4 s_ca[kN], s_cb[kN], s_nz[kN], s_av[kN];
  __shared__ float s_vtb[kN];
  const uint32_t tiles_x = ((uint32_t)w + kLdsX - 1) / kLdsX;
  const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int32_t x0 = (int32_t)(tx * kLdsX) - kHalo, y0 = (int32_t)(ty * kLdsY) - kHalo;
  for (int e = (int)threadIdx.x; e < kN; e += kBlock) {
    const int ly = e / kW, lx = e - ly * kW;
    const int32_t gx = x0 + lx, gy = y0 + ly;
    if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
      const size_t g = (size_t)gy * w + gx;
      s_ca[e] = ca[g];
      s_cb[e] = cb[g];
      s_nz[e] = nz[g];
      s_av[e] = av[g];
      s_vtb[e] = vtb[g];
    }
  }
  __syncthreads();
  const int32_t x = (int32_t)(tx * kLdsX + (threadIdx.x & (kLdsX - 1)));
  const int32_t y = (int32_t)(ty * kLdsY + threadIdx.x / kLdsX);
  if (x >= w || y >= h) return;
  const size_t i = (size_t)y * w + x;
  const LdsPairPlanes<STEP> P{s_ca, s_cb, s_nz, s_av, s_vtb, x0, y0};
  const float2 g = grad[i];
  f4 ra, rb;
  iterate_pair(P, x, y, w, h, STEP, g.x, g.y, A, own != 0, &ra, &rb);
  if constexpr (LAST) {
    finish_pair(ra, rb, s_av[(y - y0) * kW + (x - x0)], A, out + 3 * i, se_out ? se_out + 3 * i : nullptr,
                diff ? diff + 3 * i : nullptr);
  } else {
    ca_out[i] = ra;
    cb_out[i] = rb;
  }
}

// iterations == 0: the halves as given, one pixel per thread.
__global__ void __launch_bounds__(kBlock)
denoise_pair_zero_kernel(const float* __restrict__ rgb_a, const float* __restrict__ se_a,
                         const float* __restrict__ rgb_b, const float* __restrict__ se_b, size_t npix,
                         float* __restrict__ out, float* __restrict__ se_out, float* __restrict__ diff) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= npix) return;
  finish_pair_zero(rgb_a + 3 * i, se_a + 3 * i, rgb_b + 3 * i, se_b + 3 * i, out + 3 * i,
                   se_out ? se_out + 3 * i : nullptr, diff ? diff + 3 * i : nullptr);
}

// The summary of a diff plane, in the film noise summary's shape. p[0] = the block's 256 partials
// combined pairwise, in an order fixed by the thread index alone.
__device__ __forceinline__ void pair_block_reduce(PairPartial* p) {
  for (uint32_t w = kBlock / 2; w > 0; w >>= 1) {
    __syncthreads();
    if (threadIdx.x < w) {
      PairPartial& a = p[threadIdx.x];
      const PairPartial& b = p[threadIdx.x + w];
      a.s[0] += b.s[0];
      a.s[1] += b.s[1];
      a.s[2] += b.s[2];
      a.diff_max = fmaxf(a.diff_max, b.diff_max);
    }
  }
  __syncthreads();
}

// Stage 1: one pixel per thread, one partial per block, as four planes of nb = gridDim.x doubles.
__global__ void __launch_bounds__(kBlock)
denoise_pair_partials_kernel(const float* __restrict__ diff, size_t npix, double* __restrict__ out) {
  __shared__ PairPartial s_p[kBlock];
  const size_t px = (size_t)blockIdx.x * kBlock + threadIdx.x;
  PairPartial v{};
  if (px < npix) pair_partial_add(v, diff + 3 * px);
  s_p[threadIdx.x] = v;
  pair_block_reduce(s_p);
  if (threadIdx.x == 0) {
    const size_t nb = gridDim.x;
    out[blockIdx.x] = s_p[0].s[0];
    out[nb + blockIdx.x] = s_p[0].s[1];
    out[2 * nb + blockIdx.x] = s_p[0].s[2];
    out[3 * nb + blockIdx.x] = (double)s_p[0].diff_max;
  }
}

// Stage 2, one block: thread t adds the partials t, t + 256, ... in that order; *total = the image's.
__global__ void __launch_bounds__(kBlock)
denoise_pair_total_kernel(const double* __restrict__ parts, uint32_t n, PairPartial* __restrict__ total) {
  __shared__ PairPartial s_p[kBlock];
  PairPartial v{};
  for (uint32_t i = threadIdx.x; i < n; i += kBlock) {
    v.s[0] += parts[i];
    v.s[1] += parts[(size_t)n + i];
    v.s[2] += parts[2 * (size_t)n + i];
    v.diff_max = fmaxf(v.diff_max, (float)parts[3 * (size_t)n + i]);
  }
  s_p[threadIdx.x] = v;
  pair_block_reduce(s_p);
  if (threadIdx.x == 0) *total = s_p[0];
}

// ---- the filter bank (SPT_HAS_DENOISE_BANK) ----

// The last iteration of a candidate's pair run with the halves kept: denoise_atrous_pair_kernel<true>'s
// pixel and taps, finish_halves instead of finish_pair (plain loads at every step: the tiled form would
// give the same bits).
__global__ void __launch_bounds__(kBlock)
denoise_atrous_pair_halves_kernel(const f4* __restrict__ ca, const f4* __restrict__ cb, const f4* __restrict__ nz,
                                  const f4* __restrict__ av, const float* __restrict__ vtb,
                                  const float2* __restrict__ grad, int32_t w, int32_t h, int32_t step, Args A,
                                  int32_t own, float* __restrict__ oa, float* __restrict__ ob) {
  int32_t x, y;
  if (!pixel_of(w, h, &x, &y)) return;
  const size_t i = (size_t)y * w + x;
  const DevPairPlanes P{ca, cb, nz, av, vtb, w};
  const float2 g = grad[i];
  f4 ra, rb;
  iterate_pair(P, x, y, w, h, step, g.x, g.y, A, own != 0, &ra, &rb);
  finish_halves(ra, rb, av[i], A, oa + 3 * i, ob + 3 * i);
}

// Candidate k's out plane and its error estimate, one pixel per thread: component k of the pixel's 16-byte
// element of estimates (candidate 0 writes the whole element, the others' components 0).
__global__ void __launch_bounds__(kBlock)
denoise_bank_error_kernel(const float* __restrict__ oa, const float* __restrict__ ob,
                          const float* __restrict__ rgb_a, const float* __restrict__ se_a,
                          const float* __restrict__ rgb_b, const float* __restrict__ se_b, size_t npix,
                          int32_t k, f4* __restrict__ m, float* __restrict__ out_k) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= npix) return;
  const float a[3] = {oa[3 * i], oa[3 * i + 1], oa[3 * i + 2]}, b[3] = {ob[3 * i], ob[3 * i + 1], ob[3 * i + 2]};
  float o[3];
  const float e = bank_error_of(a, b, rgb_a + 3 * i, se_a + 3 * i, rgb_b + 3 * i, se_b + 3 * i, o);
  out_k[3 * i] = o[0];
  out_k[3 * i + 1] = o[1];
  out_k[3 * i + 2] = o[2];
  if (k == 0)
    m[i] = f4{e, 0.0f, 0.0f, 0.0f};
  else
    ((float*)(m + i))[k] = e;
}

struct DevBankPlanes {
  const f4 *m_, *nz_, *av_;
  int32_t w;
  __device__ __forceinline__ f4 m(int32_t x, int32_t y) const { return m_[(size_t)y * w + x]; }
  __device__ __forceinline__ f4 nz(int32_t x, int32_t y) const { return nz_[(size_t)y * w + x]; }
  __device__ __forceinline__ f4 av(int32_t x, int32_t y) const { return av_[(size_t)y * w + x]; }
};

// One smoothing pass of the estimates: a pixel per lane, three 16-byte loads per tap (the estimates,
// (n, z), (albedo, .)), the bounds test per tap.
__global__ void __launch_bounds__(kBlock)
denoise_bank_smooth_kernel(const f4* __restrict__ m, const f4* __restrict__ nz, const f4* __restrict__ av,
                           const float2* __restrict__ grad, int32_t w, int32_t h, int32_t step, Args A,
                           int32_t n, f4* __restrict__ m_out) {
  int32_t x, y;
  if (!pixel_of(w, h, &x, &y)) return;
  const size_t i = (size_t)y * w + x;
  const DevBankPlanes P{m, nz, av, w};
  const float2 g = grad[i];
  m_out[i] = bank_pass<false>(P, x, y, w, h, step, g.x, g.y, A, n);
}

// Choice and blend in one pass: the argmin of every neighbour's loaded estimates on the fly, the shares,
// the blended image, the blended estimate and the pixel's own choice.
__global__ void __launch_bounds__(kBlock)
denoise_bank_blend_kernel(const f4* __restrict__ m, const f4* __restrict__ nz, const f4* __restrict__ av,
                          const float2* __restrict__ grad, int32_t w, int32_t h, Args A, int32_t n,
                          const float* __restrict__ outk, size_t stride, float* __restrict__ out,
                          float* __restrict__ mse, uint8_t* __restrict__ choice) {
  int32_t x, y;
  if (!pixel_of(w, h, &x, &y)) return;
  const size_t i = (size_t)y * w + x;
  const DevBankPlanes P{m, nz, av, w};
  const float2 g = grad[i];
  const f4 s = bank_pass<true>(P, x, y, w, h, 1, g.x, g.y, A, n);
  const f4 mp = m[i];
  float o[3];
  const float e = bank_blend(s, mp, n, outk, stride, 3 * i, o);
  out[3 * i] = o[0];
  out[3 * i + 1] = o[1];
  out[3 * i + 2] = o[2];
  if (mse) mse[i] = e;
  if (choice) choice[i] = (uint8_t)bank_choice(mp, n);
}

// The bank summary, in the pair summary's shape: p[0] = the block's 256 partials combined pairwise.
__device__ __forceinline__ void bank_block_reduce(BankPartial* p) {
  for (uint32_t w = kBlock / 2; w > 0; w >>= 1) {
    __syncthreads();
    if (threadIdx.x < w) bank_partial_merge(p[threadIdx.x], p[threadIdx.x + w]);
  }
  __syncthreads();
}

// Stage 1: one pixel per thread, one partial per block, as seven planes of nb = gridDim.x doubles.
__global__ void __launch_bounds__(kBlock)
denoise_bank_partials_kernel(const float* __restrict__ mse, const uint8_t* __restrict__ choice, size_t npix,
                             double* __restrict__ out) {
  __shared__ BankPartial s_p[kBlock];
  const size_t px = (size_t)blockIdx.x * kBlock + threadIdx.x;
  BankPartial v = bank_partial_zero();
  if (px < npix) bank_partial_add(v, mse[px], choice[px]);
  s_p[threadIdx.x] = v;
  bank_block_reduce(s_p);
  if (threadIdx.x == 0) {
    const size_t nb = gridDim.x;
    out[blockIdx.x] = s_p[0].sum;
    for (int k = 0; k < 4; ++k) out[(size_t)(1 + k) * nb + blockIdx.x] = s_p[0].count[k];
    out[5 * nb + blockIdx.x] = (double)s_p[0].mn;
    out[6 * nb + blockIdx.x] = (double)s_p[0].mx;
  }
}

// Stage 2, one block: thread t merges the partials t, t + 256, ... in that order; *total = the image's.
__global__ void __launch_bounds__(kBlock)
denoise_bank_total_kernel(const double* __restrict__ parts, uint32_t n, BankPartial* __restrict__ total) {
  __shared__ BankPartial s_p[kBlock];
  BankPartial v = bank_partial_zero();
  for (uint32_t i = threadIdx.x; i < n; i += kBlock) {
    BankPartial b;
    b.sum = parts[i];
    for (int k = 0; k < 4; ++k) b.count[k] = parts[(size_t)(1 + k) * n + i];
    b.mn = (float)parts[5 * (size_t)n + i];
    b.mx = (float)parts[6 * (size_t)n + i];
    bank_partial_merge(v, b);
  }
  s_p[threadIdx.x] = v;
  bank_block_reduce(s_p);
  if (threadIdx.x == 0) *total = s_p[0];
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

// The pair scratch, allocated once per denoiser at its first pair call (spt.h: 60 bytes per pixel and
// the summary's partials).
spt_status pair_scratch(spt_denoiser* dn) {
  if (dn->pair_base) return SPT_OK;
  const size_t n = dn->npix, n4 = (n + 3) & ~(size_t)3;
  const size_t blocks = (n + kBlock - 1) / kBlock;
  const size_t bytes = n * 2 * sizeof(f4) + (3 * n4 + 3 * n4 + n4) * sizeof(float) +
                       4 * blocks * sizeof(double) + sizeof(PairPartial);
  SPT_HIP(hipSetDevice(dn->device));
  void* base = nullptr;
  const hipError_t e = hipMalloc(&base, bytes);
  if (e != hipSuccess) return fail(SPT_ERR_OOM, std::string("denoiser pair scratch alloc: ") + hipGetErrorString(e));
  dn->pair_base = base;
  dn->cb[0] = (f4*)base;
  dn->cb[1] = dn->cb[0] + n;
  dn->rgb_b = (float*)(dn->cb[1] + n);
  dn->se_b = dn->rgb_b + 3 * n4;
  dn->vtb = dn->se_b + 3 * n4;
  dn->parts = (double*)(dn->vtb + n4);  // 16-byte aligned: every plane before it is a multiple of 16 bytes
  dn->n_parts = (uint32_t)blocks;
  return SPT_OK;
}

// Which form a pair iteration takes, as g_form: 0 = by step (the tiled form for steps 1 and 2), 1 = plain
// loads always, 2 = the tiled form where it exists. Only the bench library can change it.
int g_pair_form = 0;

// One pair iteration of step `step` from (ca, cb) into (ca_out, cb_out) (or, last, into out / se_out / diff).
void launch_atrous_pair(const spt_denoiser* dn, const f4* ca, const f4* cb, int32_t step, bool last, const Args& A,
                        int32_t own, f4* ca_out, f4* cb_out, float* out, float* se_out, float* diff, int form,
                        hipStream_t stream) {
  const int32_t w = dn->width, h = dn->height;
  const f4 *nz = dn->nz, *av = dn->av;
  const float* vtb = dn->vtb;
  const float2* grad = dn->grad;
  const dim3 block(kBlock);
  if (form != 1 && step <= 2) {
    const dim3 grid((unsigned)tiles_of(w, h, kLdsX, kLdsY));
#define DN_PAIR_LDS(S, L) hipLaunchKernelGGL((denoise_atrous_pair_lds_kernel<S, L>), grid, block, 0, stream, ca, cb, nz, av, vtb, grad, w, h, A, own, ca_out, cb_out, out, se_out, diff)
    if (step == 1 && last) DN_PAIR_LDS(1, true);
    else if (step == 1) DN_PAIR_LDS(1, false);
    else if (last) DN_PAIR_LDS(2, true);
    else DN_PAIR_LDS(2, false);
#undef DN_PAIR_LDS
    return;
  }
  const dim3 grid((unsigned)tiles_of(w, h, kTileX, kTileY));
  if (last)
    hipLaunchKernelGGL(denoise_atrous_pair_kernel<true>, grid, block, 0, stream, ca, cb, nz, av, vtb, grad, w, h,
                       step, A, own, ca_out, cb_out, out, se_out, diff);
  else
    hipLaunchKernelGGL(denoise_atrous_pair_kernel<false>, grid, block, 0, stream, ca, cb, nz, av, vtb, grad, w, h,
                       step, A, own, ca_out, cb_out, out, se_out, diff);
}

// The pair filter of seven device planes, already validated, the pair scratch in place.
spt_status run_pair(spt_denoiser* dn, const float* rgb_a, const float* se_a, const float* rgb_b,
                    const float* se_b, const float* albedo, const float* normal, const float* depth,
                    const spt_denoise_params* p, uint32_t pair_flags, float* out, float* se_out, float* diff,
                    hipStream_t stream) {
  const dim3 block(kBlock);
  if (p->iterations == 0) {
    hipLaunchKernelGGL(denoise_pair_zero_kernel, dim3(dn->n_parts), block, 0, stream, rgb_a, se_a, rgb_b, se_b,
                       dn->npix, out, se_out, diff);
    SPT_HIP(hipGetLastError());
    return SPT_OK;
  }
  const Args A = make_args(p);
  const int32_t own = (pair_flags & SPT_DENOISE_PAIR_OWN_WEIGHTS) ? 1 : 0;
  const dim3 grid((unsigned)tiles_of(dn->width, dn->height, kTileX, kTileY));
  const int32_t w = dn->width, h = dn->height;
  hipLaunchKernelGGL(denoise_pair_pack_kernel, grid, block, 0, stream, rgb_a, se_a, rgb_b, se_b, albedo, normal,
                     depth, w, h, A, dn->cv[0], dn->cb[0], dn->nz, dn->av, dn->grad);
  for (int32_t it = 0; it < p->iterations; ++it) {
    const f4 *ca = dn->cv[it & 1], *cb = dn->cb[it & 1];
    hipLaunchKernelGGL(denoise_pair_variance_kernel, grid, block, 0, stream, ca, cb, dn->av, dn->vtb, w, h);
    const bool last = it == p->iterations - 1;
    launch_atrous_pair(dn, ca, cb, (int32_t)1 << it, last, A, own, last ? nullptr : dn->cv[(it + 1) & 1],
                       last ? nullptr : dn->cb[(it + 1) & 1], last ? out : nullptr, last ? se_out : nullptr,
                       last ? diff : nullptr, g_pair_form, stream);
  }
  SPT_HIP(hipGetLastError());
  return SPT_OK;
}

spt_status check_pair_call(const spt_denoiser* dn, const spt_denoise_params* p, uint32_t pair_flags,
                           const float* out, const float* se_out, const float* diff,
                           std::initializer_list<const float*> inputs) {
  if (!dn) return fail(SPT_ERR_INVALID_ARG, "null denoiser");
  if (const char* e = params_error(p)) return fail(SPT_ERR_INVALID_ARG, std::string("denoise_pair: ") + e);
  if (const char* e = pair_flags_error(pair_flags)) return fail(SPT_ERR_INVALID_ARG, std::string("denoise_pair: ") + e);
  if (!out) return fail(SPT_ERR_INVALID_ARG, "denoise_pair: null output plane");
  if (se_out == out || diff == out || (se_out && se_out == diff))
    return fail(SPT_ERR_INVALID_ARG, "denoise_pair: two output planes are one plane");
  for (const float* in : inputs) {
    if (!in) return fail(SPT_ERR_INVALID_ARG, "denoise_pair: null plane");
    if (in == out || in == se_out || in == diff)
      return fail(SPT_ERR_INVALID_ARG, "denoise_pair: an output plane is an input plane");
  }
  return SPT_OK;
}

// What spt_film_denoise asks of a film, for one film of a pair.
spt_status check_pair_film(const spt_film* film, const spt_guide* guide, const spt_denoiser* dn) {
  if (!film->batch) return fail(SPT_ERR_INVALID_ARG, "film_pair_denoise: not a noise film");
  if (film->batches_done < 2)
    return fail(SPT_ERR_INVALID_ARG, "film_pair_denoise: the error needs at least two batches in each film");
  if (film->shard_count > 1)
    return fail(SPT_ERR_INVALID_ARG,
                "film_pair_denoise: a shard's rows are not image neighbours; gather the planes and call spt_denoise_pair_async");
  if (film->width != dn->width || film->rows != dn->height || !spt::shape_equal(*film, *guide))
    return fail(SPT_ERR_INVALID_ARG, "film_pair_denoise: a film's or the guide's size differs from the denoiser's");
  if (film->device != dn->device)
    return fail(SPT_ERR_INVALID_ARG, "film_pair_denoise: a film and the denoiser are on different devices");
  return SPT_OK;
}

// The bank scratch, allocated once per denoiser at its first bank call (spt.h: 104 bytes per pixel and the
// summary's partials).
spt_status bank_scratch(spt_denoiser* dn) {
  if (dn->bank_base) return SPT_OK;
  const size_t n = dn->npix, n4 = (n + 3) & ~(size_t)3;
  const size_t blocks = (n + kBlock - 1) / kBlock;
  const size_t bytes = n * 2 * sizeof(f4) + (2 + kMaxCands) * 3 * n4 * sizeof(float) +
                       7 * blocks * sizeof(double) + sizeof(BankPartial);
  SPT_HIP(hipSetDevice(dn->device));
  void* base = nullptr;
  const hipError_t e = hipMalloc(&base, bytes);
  if (e != hipSuccess) return fail(SPT_ERR_OOM, std::string("denoiser bank scratch alloc: ") + hipGetErrorString(e));
  dn->bank_base = base;
  dn->bm[0] = (f4*)base;
  dn->bm[1] = dn->bm[0] + n;
  dn->oa = (float*)(dn->bm[1] + n);
  dn->ob = dn->oa + 3 * n4;
  dn->outk = dn->ob + 3 * n4;
  dn->outk_stride = 3 * n4;
  dn->bank_parts = (double*)(dn->outk + kMaxCands * 3 * n4);  // 16-byte aligned, as the pair scratch's
  return SPT_OK;
}

// The bank of seven device planes, already validated, the pair and the bank scratch in place.
spt_status run_bank(spt_denoiser* dn, const float* rgb_a, const float* se_a, const float* rgb_b,
                    const float* se_b, const float* albedo, const float* normal, const float* depth,
                    const spt_denoise_params* cands, int32_t n_cands, const spt_bank_params* bank, float* out,
                    float* mse, uint8_t* choice, hipStream_t stream) {
  const dim3 block(kBlock), grid((unsigned)tiles_of(dn->width, dn->height, kTileX, kTileY)), flat(dn->n_parts);
  const int32_t w = dn->width, h = dn->height;
  const int32_t own = (bank->pair_flags & SPT_DENOISE_PAIR_OWN_WEIGHTS) ? 1 : 0;
  for (int32_t k = 0; k < n_cands; ++k) {
    const spt_denoise_params* p = cands + k;
    const float *oa = rgb_a, *ob = rgb_b;  // iterations == 0: the halves as given
    if (p->iterations > 0) {
      const Args A = make_args(p);
      hipLaunchKernelGGL(denoise_pair_pack_kernel, grid, block, 0, stream, rgb_a, se_a, rgb_b, se_b, albedo,
                         normal, depth, w, h, A, dn->cv[0], dn->cb[0], dn->nz, dn->av, dn->grad);
      for (int32_t it = 0; it < p->iterations; ++it) {
        const f4 *ca = dn->cv[it & 1], *cb = dn->cb[it & 1];
        hipLaunchKernelGGL(denoise_pair_variance_kernel, grid, block, 0, stream, ca, cb, dn->av, dn->vtb, w, h);
        if (it < p->iterations - 1)
          launch_atrous_pair(dn, ca, cb, (int32_t)1 << it, false, A, own, dn->cv[(it + 1) & 1],
                             dn->cb[(it + 1) & 1], nullptr, nullptr, nullptr, g_pair_form, stream);
        else
          hipLaunchKernelGGL(denoise_atrous_pair_halves_kernel, grid, block, 0, stream, ca, cb,
                             (const f4*)dn->nz, (const f4*)dn->av, (const float*)dn->vtb,
                             (const float2*)dn->grad, w, h, (int32_t)1 << it, A, own, dn->oa, dn->ob);
      }
      oa = dn->oa;
      ob = dn->ob;
    }
    hipLaunchKernelGGL(denoise_bank_error_kernel, flat, block, 0, stream, oa, ob, rgb_a, se_a, rgb_b, se_b,
                       dn->npix, k, dn->bm[0], dn->outk + (size_t)k * dn->outk_stride);
  }
  const Args A0 = make_args(cands);
  if (cands[n_cands - 1].iterations == 0)  // no candidate's pack left the guides in the scratch
    hipLaunchKernelGGL(denoise_pair_pack_kernel, grid, block, 0, stream, rgb_a, se_a, rgb_b, se_b, albedo, normal,
                       depth, w, h, A0, dn->cv[0], dn->cb[0], dn->nz, dn->av, dn->grad);
  const f4* cur = dn->bm[0];
  for (int32_t it = 0; it < bank->error_iterations; ++it) {
    f4* nxt = dn->bm[(it + 1) & 1];
    hipLaunchKernelGGL(denoise_bank_smooth_kernel, grid, block, 0, stream, cur, (const f4*)dn->nz,
                       (const f4*)dn->av, (const float2*)dn->grad, w, h, (int32_t)1 << it, A0, n_cands, nxt);
    cur = nxt;
  }
  hipLaunchKernelGGL(denoise_bank_blend_kernel, grid, block, 0, stream, cur, (const f4*)dn->nz, (const f4*)dn->av,
                     (const float2*)dn->grad, w, h, A0, n_cands, (const float*)dn->outk, dn->outk_stride, out, mse,
                     choice);
  SPT_HIP(hipGetLastError());
  return SPT_OK;
}

spt_status check_bank_call(const spt_denoiser* dn, const spt_denoise_params* cands, int32_t n_cands,
                           const spt_bank_params* bank, const float* out, const float* mse, const uint8_t* choice,
                           std::initializer_list<const float*> inputs) {
  if (!dn) return fail(SPT_ERR_INVALID_ARG, "null denoiser");
  if (const char* e = bank_error(cands, n_cands, bank)) return fail(SPT_ERR_INVALID_ARG, std::string("denoise_bank: ") + e);
  if (!out) return fail(SPT_ERR_INVALID_ARG, "denoise_bank: null output plane");
  const void *o = out, *m = mse, *c = choice;
  if (m == o || c == o || (m && m == c))
    return fail(SPT_ERR_INVALID_ARG, "denoise_bank: two output planes are one plane");
  for (const float* in : inputs) {
    if (!in) return fail(SPT_ERR_INVALID_ARG, "denoise_bank: null plane");
    if (in == o || in == m || in == c)
      return fail(SPT_ERR_INVALID_ARG, "denoise_bank: an output plane is an input plane");
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
    if (dn->pair_base) (void)hipFree(dn->pair_base);
    if (dn->bank_base) (void)hipFree(dn->bank_base);
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

extern "C" spt_status spt_denoise_pair_async(spt_denoiser* dn, const float* rgb_a_dev, const float* se_a_dev,
                                             const float* rgb_b_dev, const float* se_b_dev,
                                             const float* albedo_dev, const float* normal_dev,
                                             const float* depth_dev, const spt_denoise_params* params,
                                             uint32_t pair_flags, float* out_dev, float* se_out_dev,
                                             float* diff_dev, void* stream) {
  SPT_TRY(check_pair_call(dn, params, pair_flags, out_dev, se_out_dev, diff_dev,
                          {rgb_a_dev, se_a_dev, rgb_b_dev, se_b_dev, albedo_dev, normal_dev, depth_dev}));
  SPT_TRY(pair_scratch(dn));
  SPT_HIP(hipSetDevice(dn->device));
  return run_pair(dn, rgb_a_dev, se_a_dev, rgb_b_dev, se_b_dev, albedo_dev, normal_dev, depth_dev, params,
                  pair_flags, out_dev, se_out_dev, diff_dev, (hipStream_t)stream);
}

extern "C" spt_status spt_film_pair_denoise(const spt_film* film_a, const spt_film* film_b,
                                            const spt_guide* guide, spt_denoiser* dn,
                                            const spt_denoise_params* params, uint32_t pair_flags,
                                            float* out_dev, float* se_out_dev, float* diff_dev, void* stream) {
  if (!film_a || !film_b || !guide) return fail(SPT_ERR_INVALID_ARG, "film_pair_denoise: null film or guide");
  SPT_TRY(check_pair_call(dn, params, pair_flags, out_dev, se_out_dev, diff_dev, {}));
  if (film_a == film_b) return fail(SPT_ERR_INVALID_ARG, "film_pair_denoise: the two halves are one film");
  if (guide->samples_done == 0) return fail(SPT_ERR_INVALID_ARG, "film_pair_denoise: the guide holds no sample");
  SPT_TRY(check_pair_film(film_a, guide, dn));
  SPT_TRY(check_pair_film(film_b, guide, dn));
  if (film_a->spp_total != film_b->spp_total)
    return fail(SPT_ERR_INVALID_ARG, "film_pair_denoise: the films' spp_total differ");
  SPT_TRY(pair_scratch(dn));
  SPT_TRY(spt_film_resolve(film_a, dn->rgb, stream));
  SPT_TRY(spt_film_noise_map(film_a, dn->se, stream));
  SPT_TRY(spt_film_resolve(film_b, dn->rgb_b, stream));
  SPT_TRY(spt_film_noise_map(film_b, dn->se_b, stream));
  SPT_TRY(spt_guide_resolve(guide, dn->albedo, dn->normal, dn->depth, nullptr, stream));
  SPT_HIP(hipSetDevice(dn->device));
  return run_pair(dn, dn->rgb, dn->se, dn->rgb_b, dn->se_b, dn->albedo, dn->normal, dn->depth, params,
                  pair_flags, out_dev, se_out_dev, diff_dev, (hipStream_t)stream);
}

extern "C" spt_status spt_denoise_pair_summary(spt_denoiser* dn, const float* diff_dev, spt_pair_summary* out,
                                               void* stream_v) {
  if (!dn || !diff_dev || !out) return fail(SPT_ERR_INVALID_ARG, "denoise_pair_summary: null argument");
  SPT_TRY(pair_scratch(dn));
  hipStream_t stream = (hipStream_t)stream_v;
  SPT_HIP(hipSetDevice(dn->device));
  PairPartial* total_dev = (PairPartial*)(dn->parts + 4 * (size_t)dn->n_parts);
  hipLaunchKernelGGL(denoise_pair_partials_kernel, dim3(dn->n_parts), dim3(kBlock), 0, stream, diff_dev,
                     dn->npix, dn->parts);
  SPT_HIP(hipGetLastError());
  hipLaunchKernelGGL(denoise_pair_total_kernel, dim3(1), dim3(kBlock), 0, stream, (const double*)dn->parts,
                     dn->n_parts, total_dev);
  SPT_HIP(hipGetLastError());
  PairPartial total{};
  SPT_HIP(hipMemcpyAsync(&total, total_dev, sizeof total, hipMemcpyDeviceToHost, stream));
  SPT_HIP(hipStreamSynchronize(stream));
  pair_summary_finish(total, dn->npix, out);
  return SPT_OK;
}

extern "C" spt_status spt_denoise_bank_async(spt_denoiser* dn, const float* rgb_a_dev, const float* se_a_dev,
                                             const float* rgb_b_dev, const float* se_b_dev,
                                             const float* albedo_dev, const float* normal_dev,
                                             const float* depth_dev, const spt_denoise_params* cands,
                                             int32_t n_cands, const spt_bank_params* bank, float* out_dev,
                                             float* mse_dev, uint8_t* choice_dev, void* stream) {
  SPT_TRY(check_bank_call(dn, cands, n_cands, bank, out_dev, mse_dev, choice_dev,
                          {rgb_a_dev, se_a_dev, rgb_b_dev, se_b_dev, albedo_dev, normal_dev, depth_dev}));
  SPT_TRY(pair_scratch(dn));
  SPT_TRY(bank_scratch(dn));
  SPT_HIP(hipSetDevice(dn->device));
  return run_bank(dn, rgb_a_dev, se_a_dev, rgb_b_dev, se_b_dev, albedo_dev, normal_dev, depth_dev, cands, n_cands,
                  bank, out_dev, mse_dev, choice_dev, (hipStream_t)stream);
}

extern "C" spt_status spt_film_pair_denoise_bank(const spt_film* film_a, const spt_film* film_b,
                                                 const spt_guide* guide, spt_denoiser* dn,
                                                 const spt_denoise_params* cands, int32_t n_cands,
                                                 const spt_bank_params* bank, float* out_dev, float* mse_dev,
                                                 uint8_t* choice_dev, void* stream) {
  if (!film_a || !film_b || !guide) return fail(SPT_ERR_INVALID_ARG, "film_pair_denoise_bank: null film or guide");
  SPT_TRY(check_bank_call(dn, cands, n_cands, bank, out_dev, mse_dev, choice_dev, {}));
  if (film_a == film_b) return fail(SPT_ERR_INVALID_ARG, "film_pair_denoise_bank: the two halves are one film");
  if (guide->samples_done == 0) return fail(SPT_ERR_INVALID_ARG, "film_pair_denoise_bank: the guide holds no sample");
  SPT_TRY(check_pair_film(film_a, guide, dn));
  SPT_TRY(check_pair_film(film_b, guide, dn));
  if (film_a->spp_total != film_b->spp_total)
    return fail(SPT_ERR_INVALID_ARG, "film_pair_denoise_bank: the films' spp_total differ");
  SPT_TRY(pair_scratch(dn));
  SPT_TRY(bank_scratch(dn));
  SPT_TRY(spt_film_resolve(film_a, dn->rgb, stream));
  SPT_TRY(spt_film_noise_map(film_a, dn->se, stream));
  SPT_TRY(spt_film_resolve(film_b, dn->rgb_b, stream));
  SPT_TRY(spt_film_noise_map(film_b, dn->se_b, stream));
  SPT_TRY(spt_guide_resolve(guide, dn->albedo, dn->normal, dn->depth, nullptr, stream));
  SPT_HIP(hipSetDevice(dn->device));
  return run_bank(dn, dn->rgb, dn->se, dn->rgb_b, dn->se_b, dn->albedo, dn->normal, dn->depth, cands, n_cands,
                  bank, out_dev, mse_dev, choice_dev, (hipStream_t)stream);
}

extern "C" spt_status spt_denoise_bank_summary(spt_denoiser* dn, const float* mse_dev, const uint8_t* choice_dev,
                                               spt_bank_summary* out, void* stream_v) {
  if (!dn || !mse_dev || !choice_dev || !out) return fail(SPT_ERR_INVALID_ARG, "denoise_bank_summary: null argument");
  SPT_TRY(pair_scratch(dn));
  SPT_TRY(bank_scratch(dn));
  hipStream_t stream = (hipStream_t)stream_v;
  SPT_HIP(hipSetDevice(dn->device));
  BankPartial* total_dev = (BankPartial*)(dn->bank_parts + 7 * (size_t)dn->n_parts);
  hipLaunchKernelGGL(denoise_bank_partials_kernel, dim3(dn->n_parts), dim3(kBlock), 0, stream, mse_dev, choice_dev,
                     dn->npix, dn->bank_parts);
  SPT_HIP(hipGetLastError());
  hipLaunchKernelGGL(denoise_bank_total_kernel, dim3(1), dim3(kBlock), 0, stream, (const double*)dn->bank_parts,
                     dn->n_parts, total_dev);
  SPT_HIP(hipGetLastError());
  BankPartial total = bank_partial_zero();
  SPT_HIP(hipMemcpyAsync(&total, total_dev, sizeof total, hipMemcpyDeviceToHost, stream));
  SPT_HIP(hipStreamSynchronize(stream));
  bank_summary_finish(total, dn->npix, out);
  return SPT_OK;
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
// The same two for the pair filter. spt_denoise_pair_bench_form: g_pair_form. spt_denoise_pair_bench_kernel,
// which: 0 the pair pack of the seven planes, 1 the pair variance pass over (cv[0], cb[0]), 2 a pair a-trous
// pass into (cv[1], cb[1]), 3 the pair a-trous pass with the finish fused in, into out / se_out / diff.
extern "C" spt_status spt_denoise_pair_bench_form(int32_t form) {
  if (form < 0 || form > 2) return fail(SPT_ERR_INVALID_ARG, "form: 0, 1 or 2");
  g_pair_form = form;
  return SPT_OK;
}
extern "C" spt_status spt_denoise_pair_bench_kernel(spt_denoiser* dn, int32_t which, int32_t step, int32_t form,
                                                    const float* rgb_a, const float* se_a, const float* rgb_b,
                                                    const float* se_b, const float* albedo, const float* normal,
                                                    const float* depth, const spt_denoise_params* params,
                                                    uint32_t pair_flags, float* out, float* se_out, float* diff,
                                                    void* stream_v) {
  if (!dn || params_error(params) || pair_flags_error(pair_flags) || which < 0 || which > 3 || step < 1 ||
      step > 32 || (step & (step - 1)) || form < 1 || form > 2 || (form == 2 && step > 2))
    return fail(SPT_ERR_INVALID_ARG, "pair_bench_kernel: bad argument");
  SPT_TRY(pair_scratch(dn));
  hipStream_t stream = (hipStream_t)stream_v;
  const Args A = make_args(params);
  const int32_t own = (pair_flags & SPT_DENOISE_PAIR_OWN_WEIGHTS) ? 1 : 0;
  const dim3 grid((unsigned)tiles_of(dn->width, dn->height, kTileX, kTileY)), block(kBlock);
  SPT_HIP(hipSetDevice(dn->device));
  if (which == 0)
    hipLaunchKernelGGL(denoise_pair_pack_kernel, grid, block, 0, stream, rgb_a, se_a, rgb_b, se_b, albedo, normal,
                       depth, dn->width, dn->height, A, dn->cv[0], dn->cb[0], dn->nz, dn->av, dn->grad);
  else if (which == 1)
    hipLaunchKernelGGL(denoise_pair_variance_kernel, grid, block, 0, stream, (const f4*)dn->cv[0],
                       (const f4*)dn->cb[0], dn->av, dn->vtb, dn->width, dn->height);
  else
    launch_atrous_pair(dn, dn->cv[0], dn->cb[0], step, which == 3, A, own, which == 3 ? nullptr : dn->cv[1],
                       which == 3 ? nullptr : dn->cb[1], which == 3 ? out : nullptr, which == 3 ? se_out : nullptr,
                       which == 3 ? diff : nullptr, form, stream);
  SPT_HIP(hipGetLastError());
  return SPT_OK;
}
// One launch of one bank kernel on the scratch a bank call has left (call spt_denoise_bank_async first).
// which: 0 the error kernel of candidate 0 over the scratch's halves, 1 a smoothing pass of step `step`
// from one estimate plane into the other, 2 the choice-and-blend kernel of n_cands candidates into out /
// mse / choice, 3 the halves-storing pair pass of step `step` over (cv[0], cb[0]).
extern "C" spt_status spt_denoise_bank_bench_kernel(spt_denoiser* dn, int32_t which, int32_t step, int32_t n_cands,
                                                    const float* rgb_a, const float* se_a, const float* rgb_b,
                                                    const float* se_b, const spt_denoise_params* params,
                                                    float* out, float* mse, uint8_t* choice, void* stream_v) {
  if (!dn || !dn->bank_base || params_error(params) || which < 0 || which > 3 || step < 1 || step > 32 ||
      (step & (step - 1)) || n_cands < 1 || n_cands > kMaxCands || (which == 2 && !out) ||
      (which == 0 && (!rgb_a || !se_a || !rgb_b || !se_b)))
    return fail(SPT_ERR_INVALID_ARG, "bank_bench_kernel: bad argument, or no bank call before");
  hipStream_t stream = (hipStream_t)stream_v;
  const Args A = make_args(params);
  const int32_t w = dn->width, h = dn->height;
  const dim3 grid((unsigned)tiles_of(w, h, kTileX, kTileY)), block(kBlock);
  SPT_HIP(hipSetDevice(dn->device));
  if (which == 0)
    hipLaunchKernelGGL(denoise_bank_error_kernel, dim3(dn->n_parts), block, 0, stream, (const float*)dn->oa,
                       (const float*)dn->ob, rgb_a, se_a, rgb_b, se_b, dn->npix, 0, dn->bm[0], dn->outk);
  else if (which == 1)
    hipLaunchKernelGGL(denoise_bank_smooth_kernel, grid, block, 0, stream, (const f4*)dn->bm[0], (const f4*)dn->nz,
                       (const f4*)dn->av, (const float2*)dn->grad, w, h, step, A, n_cands, dn->bm[1]);
  else if (which == 2)
    hipLaunchKernelGGL(denoise_bank_blend_kernel, grid, block, 0, stream, (const f4*)dn->bm[0], (const f4*)dn->nz,
                       (const f4*)dn->av, (const float2*)dn->grad, w, h, A, n_cands, (const float*)dn->outk,
                       dn->outk_stride, out, mse, choice);
  else
    hipLaunchKernelGGL(denoise_atrous_pair_halves_kernel, grid, block, 0, stream, (const f4*)dn->cv[0],
                       (const f4*)dn->cb[0], (const f4*)dn->nz, (const f4*)dn->av, (const float*)dn->vtb,
                       (const float2*)dn->grad, w, h, step, A, 1, dn->oa, dn->ob);
  SPT_HIP(hipGetLastError());
  return SPT_OK;
}
#endif

// spt_denoise.hip — the edge-stopping a-trous filter on the device (include/spt.h, SPT_HAS_DENOISE), the
// two-half filter (SPT_HAS_DENOISE_PAIR) and the filter bank (SPT_HAS_DENOISE_BANK): the denoiser object
// that owns the scratch, the kernels and the spt_denoise_* / spt_film_*denoise* calls. The arithmetic is
// spt_denoise.h's, shared with the CPU statement (spt_denoise_host.cpp): the kernels only decide which
// lane takes which pixel. Each kernel is a name and a parameter list around shared device pieces: the
// tile -> pixel mapping (TileOf), the pack (pack_pixel), the halo staging (stage_tile), a single or a pair
// iteration with its finish (atrous_pixel, pair_pixel) and the two-stage reduction (Sum policies). The
// calls share one argument check, one scratch carver, one film-pair staging and one form dispatcher.
#include <hip/hip_runtime.h>

#include <type_traits>

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

// The two tilings, 256 lanes each: 64 x 4 (a wave covers 64 consecutive x) for the kernels that load
// from global memory, 32 x 8 for those that stage their tile and its halo in LDS.
constexpr int kTileX = 64, kTileY = 4, kBlock = kTileX * kTileY;
constexpr int kLdsX = 32, kLdsY = 8;

using DevPlanes = Planes<RowMajor>;

// The block's tile of TX x TY pixels and this lane's pixel in it. Blocks are a 1-D grid over the tiles,
// rows of tiles first.
template <int TX, int TY>
struct TileOf {
  uint32_t tx, ty;
  __device__ __forceinline__ explicit TileOf(int32_t w) {
    const uint32_t tiles_x = ((uint32_t)w + TX - 1) / TX;
    ty = blockIdx.x / tiles_x;
    tx = blockIdx.x - ty * tiles_x;
  }
  __device__ __forceinline__ bool pixel(int32_t w, int32_t h, int32_t* x, int32_t* y) const {
    *x = (int32_t)(tx * TX + (threadIdx.x & (TX - 1)));
    *y = (int32_t)(ty * TY + threadIdx.x / TX);
    return *x < w && *y < h;
  }
};

__device__ __forceinline__ bool pixel_of(int32_t w, int32_t h, int32_t* x, int32_t* y) {
  return TileOf<kTileX, kTileY>(w).pixel(w, h, x, y);
}

// The staged region of a 32 x 8 tile at spacing STEP: the tile and a halo of 2 * STEP pixels.
template <int STEP>
struct Halo {
  static constexpr int kHalo = 2 * STEP, kW = kLdsX + 2 * kHalo, kH = kLdsY + 2 * kHalo, kN = kW * kH;
};

template <class T>
struct Staged {
  T* lds;
  const T* src;
};

// Stage the block's tile plus halo of every plane in LDS, in one loop (places outside the image are left
// unwritten: the per-tap bounds test is the image's, so they are never read). -> where a pixel lies in it.
template <int STEP, class... T>
__device__ __forceinline__ Tile<Halo<STEP>::kW> stage_tile(const TileOf<kLdsX, kLdsY>& t, int32_t w, int32_t h,
                                                           Staged<T>... planes) {
  using H = Halo<STEP>;
  const Tile<H::kW> at{(int32_t)(t.tx * kLdsX) - H::kHalo, (int32_t)(t.ty * kLdsY) - H::kHalo};
  for (int e = (int)threadIdx.x; e < H::kN; e += kBlock) {
    const int ly = e / H::kW, lx = e - ly * H::kW;
    const int32_t gx = at.x0 + lx, gy = at.y0 + ly;
    if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
      const size_t g = (size_t)gy * w + gx;
      ((planes.lds[e] = planes.src[g]), ...);
    }
  }
  __syncthreads();
  return at;
}

// The guides and the gradient of pixel i into the packed planes. albedo: the pixel's own three floats,
// which its kernel has loaded for prepare().
__device__ __forceinline__ void pack_pixel(const float* normal, const float* depth, const float* albedo,
                                           int32_t x, int32_t y, int32_t w, int32_t h, size_t i, f4* nz, f4* av,
                                           float2* grad) {
  float2 g;
  pack_guides(normal, depth, albedo, x, y, w, h, i, nz + i, av + i, &g.x, &g.y);
  grad[i] = g;
}

// One iteration at one pixel, from global memory or a staged copy. LAST: the finish instead of the other
// ping-pong plane.
template <bool LAST, class P>
__device__ __forceinline__ void atrous_pixel(const P& pl, int32_t x, int32_t y, int32_t w, int32_t h,
                                             int32_t step, const float2* grad, const Args& A, f4* cv_out,
                                             float* out, float* se_out) {
  const size_t i = (size_t)y * w + x;
  const float2 g = grad[i];
  const f4 r = iterate(pl, x, y, w, h, step, g.x, g.y, A);
  if constexpr (LAST)
    finish(r, pl.av_own(x, y, i), A, out + 3 * i, se_out ? se_out + 3 * i : nullptr);
  else
    cv_out[i] = r;
}

// How a pair iteration ends: the other ping-pong planes, the pair's finish (o0, o1, o2 = out, se_out,
// diff), or the finish with the halves kept (o0, o1 = o^A, o^B: the bank's).
enum PairEnd { kNext, kFinish, kHalves };

template <PairEnd END, class P>
__device__ __forceinline__ void pair_pixel(const P& pl, int32_t x, int32_t y, int32_t w, int32_t h, int32_t step,
                                           const float2* grad, const Args& A, int32_t own, f4* ca_out,
                                           f4* cb_out, float* o0, float* o1, float* o2) {
  const size_t i = (size_t)y * w + x;
  const float2 g = grad[i];
  f4 ra, rb;
  iterate_pair(pl, x, y, w, h, step, g.x, g.y, A, own != 0, &ra, &rb);
  if constexpr (END == kFinish) {
    finish_pair(ra, rb, pl.av_own(x, y, i), A, o0 + 3 * i, o1 ? o1 + 3 * i : nullptr, o2 ? o2 + 3 * i : nullptr);
  } else if constexpr (END == kHalves) {
    finish_halves(ra, rb, pl.av_own(x, y, i), A, o0 + 3 * i, o1 + 3 * i);
  } else {
    ca_out[i] = ra;
    cb_out[i] = rb;
  }
}

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
  cv[i] = prepare(c, e, a, A);
  pack_pixel(normal, depth, a, x, y, w, h, i, nz, av, grad);
}

// vt of the current v into av.w, before the iteration that reads it at both ends of every tap.
__global__ void __launch_bounds__(kBlock)
denoise_variance_kernel(const f4* __restrict__ cv, f4* __restrict__ av, int32_t w, int32_t h) {
  int32_t x, y;
  if (!pixel_of(w, h, &x, &y)) return;
  av[(size_t)y * w + x].w = variance_filter(DevPlanes{{w}, nullptr, nullptr, cv}, x, y, w, h);
}

// One iteration: a pixel per lane, three 16-byte loads per tap (a wave's lanes read one contiguous
// row segment), the bounds test per tap.
template <bool LAST>
__global__ void __launch_bounds__(kBlock)
denoise_atrous_kernel(const f4* __restrict__ cv, const f4* __restrict__ nz, const f4* __restrict__ av,
                      const float2* __restrict__ grad, int32_t w, int32_t h, int32_t step, Args A,
                      f4* __restrict__ cv_out, float* __restrict__ out, float* __restrict__ se_out) {
  int32_t x, y;
  if (!pixel_of(w, h, &x, &y)) return;
  atrous_pixel<LAST>(DevPlanes{{w}, nz, av, cv}, x, y, w, h, step, grad, A, cv_out, out, se_out);
}

// The LDS-tiled form of one iteration, for the steps whose halo (2 * STEP pixels) is smaller than the
// tile: a block stages its 32 x 8 tile plus halo of the three packed planes in LDS, then every lane runs
// the same iterate() on the staged copy. Same operations in the same order: same bits.
template <int STEP, bool LAST>
__global__ void __launch_bounds__(kBlock)
denoise_atrous_lds_kernel(const f4* __restrict__ cv, const f4* __restrict__ nz, const f4* __restrict__ av,
                          const float2* __restrict__ grad, int32_t w, int32_t h, Args A,
                          f4* __restrict__ cv_out, float* __restrict__ out, float* __restrict__ se_out) {
  using H = Halo<STEP>;
  __shared__ f4 s_cv[H::kN], s_nz[H::kN], s_av[H::kN];
  const TileOf<kLdsX, kLdsY> t(w);
  const auto at = stage_tile<STEP>(t, w, h, Staged<f4>{s_cv, cv}, Staged<f4>{s_nz, nz}, Staged<f4>{s_av, av});
  int32_t x, y;
  if (!t.pixel(w, h, &x, &y)) return;
  atrous_pixel<LAST>(Planes<Tile<H::kW>>{at, s_nz, s_av, s_cv}, x, y, w, h, STEP, grad, A, cv_out, out, se_out);
}

// ---- the two-half filter (SPT_HAS_DENOISE_PAIR): iterate_pair() on the same two tilings ----

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
  ca[i] = prepare(c0, e0, a, A);
  cb[i] = prepare(c1, e1, a, A);
  pack_pixel(normal, depth, a, x, y, w, h, i, nz, av, grad);
}

// vt of both halves' current v: half A's into av.w, half B's into its own plane.
__global__ void __launch_bounds__(kBlock)
denoise_pair_variance_kernel(const f4* __restrict__ ca, const f4* __restrict__ cb, f4* __restrict__ av,
                             float* __restrict__ vtb, int32_t w, int32_t h) {
  int32_t x, y;
  if (!pixel_of(w, h, &x, &y)) return;
  av[(size_t)y * w + x].w = variance_filter(DevPlanes{{w}, nullptr, nullptr, ca}, x, y, w, h);
  vtb[(size_t)y * w + x] = variance_filter(DevPlanes{{w}, nullptr, nullptr, cb}, x, y, w, h);
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
  pair_pixel<LAST ? kFinish : kNext>(DevPlanes{{w}, nz, av, ca, cb, vtb}, x, y, w, h, step, grad, A, own, ca_out,
                                     cb_out, out, se_out, diff);
}

// The LDS-tiled form of one pair iteration, for steps 1 and 2 (as denoise_atrous_lds_kernel): the 32 x 8
// tile plus halo of the four packed planes and vt^B staged in LDS (29 KB at step 1, 43.5 KB at step 2),
// then the same iterate_pair() on the staged copy. Same operations in the same order: same bits.
template <int STEP, bool LAST>
__global__ void __launch_bounds__(kBlock)
denoise_atrous_pair_lds_kernel(const f4* __restrict__ ca, const f4* __restrict__ cb, const f4* __restrict__ nz,
                               const f4* __restrict__ av, const float* __restrict__ vtb,
                               const float2* __restrict__ grad, int32_t w, int32_t h, Args A, int32_t own,
                               f4* __restrict__ ca_out, f4* __restrict__ cb_out, float* __restrict__ out,
                               float* __restrict__ se_out, float* __restrict__ diff) {
  using H = Halo<STEP>;
  __shared__ f4 s_ca[H::kN], s_cb[H::kN], s_nz[H::kN], s_av[H::kN];
  __shared__ float s_vtb[H::kN];
  const TileOf<kLdsX, kLdsY> t(w);
  const auto at = stage_tile<STEP>(t, w, h, Staged<f4>{s_ca, ca}, Staged<f4>{s_cb, cb}, Staged<f4>{s_nz, nz},
                                   Staged<f4>{s_av, av}, Staged<float>{s_vtb, vtb});
  int32_t x, y;
  if (!t.pixel(w, h, &x, &y)) return;
  pair_pixel<LAST ? kFinish : kNext>(Planes<Tile<H::kW>>{at, s_nz, s_av, s_ca, s_cb, s_vtb}, x, y, w, h, STEP, grad,
                                     A, own, ca_out, cb_out, out, se_out, diff);
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

// ---- the summaries: one two-stage reduction, in the film noise summary's shape ----
// A Sum policy names the partial of an image, its zero, how a pixel enters it and how two merge, and
// how it is stored between the stages: as kPlanes planes of doubles, plane k of a partial by get / set.
struct PairSum {
  using Partial = PairPartial;
  static constexpr int kPlanes = 4;
  static SPT_FILM_FN Partial zero() { return pair_partial_zero(); }
  static SPT_FILM_FN void add(Partial& p, size_t px, const float* diff) { pair_partial_add(p, diff + 3 * px); }
  static SPT_FILM_FN void merge(Partial& a, const Partial& b) { pair_partial_merge(a, b); }
  static SPT_FILM_FN double get(const Partial& p, int k) { return k < 3 ? p.s[k] : (double)p.diff_max; }
  static SPT_FILM_FN void set(Partial& p, int k, double v) {
    if (k < 3)
      p.s[k] = v;
    else
      p.diff_max = (float)v;
  }
};

struct BankSum {
  using Partial = BankPartial;
  static constexpr int kPlanes = 7;
  static SPT_FILM_FN Partial zero() { return bank_partial_zero(); }
  static SPT_FILM_FN void add(Partial& p, size_t px, const float* mse, const uint8_t* choice) {
    bank_partial_add(p, mse[px], choice[px]);
  }
  static SPT_FILM_FN void merge(Partial& a, const Partial& b) { bank_partial_merge(a, b); }
  static SPT_FILM_FN double get(const Partial& p, int k) {
    return k == 0 ? p.sum : k < 5 ? p.count[k - 1] : (double)(k == 5 ? p.mn : p.mx);
  }
  static SPT_FILM_FN void set(Partial& p, int k, double v) {
    if (k == 0)
      p.sum = v;
    else if (k < 5)
      p.count[k - 1] = v;
    else
      (k == 5 ? p.mn : p.mx) = (float)v;
  }
};

// The block's 256 partials combined pairwise, in an order fixed by the thread index alone.
template <class S>
__device__ __forceinline__ const typename S::Partial& block_total(const typename S::Partial& v) {
  __shared__ typename S::Partial s_p[kBlock];
  s_p[threadIdx.x] = v;
  for (uint32_t w = kBlock / 2; w > 0; w >>= 1) {
    __syncthreads();
    if (threadIdx.x < w) S::merge(s_p[threadIdx.x], s_p[threadIdx.x + w]);
  }
  __syncthreads();
  return s_p[0];
}

// Stage 1: one pixel per thread, one partial per block, as kPlanes planes of nb = gridDim.x doubles.
template <class S, class... In>
__device__ __forceinline__ void block_partial(size_t npix, double* out, In... in) {
  const size_t px = (size_t)blockIdx.x * kBlock + threadIdx.x;
  typename S::Partial v = S::zero();
  if (px < npix) S::add(v, px, in...);
  const typename S::Partial& t = block_total<S>(v);
  if (threadIdx.x == 0)
    for (int k = 0; k < S::kPlanes; ++k) out[(size_t)k * gridDim.x + blockIdx.x] = S::get(t, k);
}

// Stage 2, one block: thread t merges the partials t, t + 256, ... in that order; *total = the image's.
template <class S>
__device__ __forceinline__ void image_total(const double* parts, uint32_t n, typename S::Partial* total) {
  typename S::Partial v = S::zero();
  for (uint32_t i = threadIdx.x; i < n; i += kBlock) {
    typename S::Partial b;
    for (int k = 0; k < S::kPlanes; ++k) S::set(b, k, parts[(size_t)k * n + i]);
    S::merge(v, b);
  }
  const typename S::Partial& t = block_total<S>(v);
  if (threadIdx.x == 0) *total = t;
}

__global__ void __launch_bounds__(kBlock)
denoise_pair_partials_kernel(const float* __restrict__ diff, size_t npix, double* __restrict__ out) {
  block_partial<PairSum>(npix, out, diff);
}

__global__ void __launch_bounds__(kBlock)
denoise_pair_total_kernel(const double* __restrict__ parts, uint32_t n, PairPartial* __restrict__ total) {
  image_total<PairSum>(parts, n, total);
}

__global__ void __launch_bounds__(kBlock)
denoise_bank_partials_kernel(const float* __restrict__ mse, const uint8_t* __restrict__ choice, size_t npix,
                             double* __restrict__ out) {
  block_partial<BankSum>(npix, out, mse, choice);
}

__global__ void __launch_bounds__(kBlock)
denoise_bank_total_kernel(const double* __restrict__ parts, uint32_t n, BankPartial* __restrict__ total) {
  image_total<BankSum>(parts, n, total);
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
  pair_pixel<kHalves>(DevPlanes{{w}, nz, av, ca, cb, vtb}, x, y, w, h, step, grad, A, own, nullptr, nullptr, oa,
                      ob, nullptr);
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

// One smoothing pass of the estimates: a pixel per lane, three 16-byte loads per tap (the estimates,
// (n, z), (albedo, .)), the bounds test per tap.
__global__ void __launch_bounds__(kBlock)
denoise_bank_smooth_kernel(const f4* __restrict__ m, const f4* __restrict__ nz, const f4* __restrict__ av,
                           const float2* __restrict__ grad, int32_t w, int32_t h, int32_t step, Args A,
                           int32_t n, f4* __restrict__ m_out) {
  int32_t x, y;
  if (!pixel_of(w, h, &x, &y)) return;
  const size_t i = (size_t)y * w + x;
  const DevPlanes P{{w}, nz, av, nullptr, nullptr, nullptr, m};
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
  const DevPlanes P{{w}, nz, av, nullptr, nullptr, nullptr, m};
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

// ---- the calls ----

size_t tiles_of(int32_t w, int32_t h, int tile_x, int tile_y) {
  return (((size_t)w + tile_x - 1) / tile_x) * (((size_t)h + tile_y - 1) / tile_y);
}
// A launch holds fewer than 2^32 threads: both tilings must fit (spt_denoiser_create refuses otherwise).
constexpr size_t kMaxTiles = 0xFFFFFFFFull / kBlock;

dim3 grid_of(const spt_denoiser* dn, int tile_x = kTileX, int tile_y = kTileY) {
  return dim3((unsigned)tiles_of(dn->width, dn->height, tile_x, tile_y));
}

// A scratch allocation's layout: planes of one element per pixel (the 16-byte ones first), float planes
// padded to 16 bytes (n4 floats per channel), then whatever follows. Without a base it only measures.
struct Carver {
  size_t n, n4, blocks, off = 0;
  char* base;
  explicit Carver(size_t npix, void* b = nullptr)
      : n(npix), n4((npix + 3) & ~(size_t)3), blocks((npix + kBlock - 1) / kBlock), base((char*)b) {}
  template <class T>
  T* take(size_t count) {
    T* p = base ? (T*)(base + off) : nullptr;
    off += count * sizeof(T);
    return p;
  }
  f4* quad() { return take<f4>(n); }
  float* floats(int channels) { return take<float>(channels * n4); }
  // a summary's partials (16-byte aligned: every plane before them is a multiple of 16 bytes) and its total
  template <class S>
  double* partials() {
    double* p = take<double>(S::kPlanes * blocks);
    take<typename S::Partial>(1);
    return p;
  }
};

// Measure `layout`, allocate it on the denoiser's device and lay it out. what: the allocation's name.
template <class Layout>
spt_status alloc_scratch(const spt_denoiser* dn, void** base, const char* what, const Layout& layout) {
  Carver measure(dn->npix);
  layout(measure);
  SPT_HIP(hipSetDevice(dn->device));
  void* b = nullptr;
  const hipError_t e = hipMalloc(&b, measure.off);
  if (e != hipSuccess) return fail(SPT_ERR_OOM, std::string(what) + " alloc: " + hipGetErrorString(e));
  Carver carve(dn->npix, *base = b);
  layout(carve);
  return SPT_OK;
}

// The pair scratch, allocated once per denoiser at its first pair call (spt.h: 60 bytes per pixel and
// the summary's partials).
spt_status pair_scratch(spt_denoiser* dn) {
  if (dn->pair_base) return SPT_OK;
  return alloc_scratch(dn, &dn->pair_base, "denoiser pair scratch", [dn](Carver& c) {
    dn->cb[0] = c.quad();
    dn->cb[1] = c.quad();
    dn->rgb_b = c.floats(3);
    dn->se_b = c.floats(3);
    dn->vtb = c.floats(1);
    dn->parts = c.partials<PairSum>();
    dn->n_parts = (uint32_t)c.blocks;
  });
}

// The bank scratch, allocated once per denoiser at its first bank call (spt.h: 104 bytes per pixel and the
// summary's partials).
spt_status bank_scratch(spt_denoiser* dn) {
  if (dn->bank_base) return SPT_OK;
  return alloc_scratch(dn, &dn->bank_base, "denoiser bank scratch", [dn](Carver& c) {
    dn->bm[0] = c.quad();
    dn->bm[1] = c.quad();
    dn->oa = c.floats(3);
    dn->ob = c.floats(3);
    dn->outk = c.floats(3 * kMaxCands);
    dn->outk_stride = 3 * c.n4;
    dn->bank_parts = c.partials<BankSum>();
  });
}

// What every call asks first: a denoiser, parameters in range (perr: what is wrong with them, or NULL),
// the output `outs` begins with, distinct outputs, and inputs that are planes and no output's.
spt_status check_call(const spt_denoiser* dn, const char* who, const char* perr, PlaneList outs, PlaneList ins) {
  if (!dn) return fail(SPT_ERR_INVALID_ARG, "null denoiser");
  const char* e = perr ? perr : !*outs.begin() ? "null output plane" : outputs_error(outs);
  if (!e) e = inputs_error(outs, ins);
  return e ? fail(SPT_ERR_INVALID_ARG, std::string(who) + ": " + e) : SPT_OK;
}

const char* pair_error(const spt_denoise_params* p, uint32_t pair_flags) {
  const char* e = params_error(p);
  return e ? e : pair_flags_error(pair_flags);
}

// The summary of an image: stage 1 (launched by the caller's stage1(grid, block)), stage 2, the total
// copied to the host and waited for.
template <class S, class Stage1>
spt_status sum_image(spt_denoiser* dn, double* parts, const Stage1& stage1,
                     void (*stage2)(const double*, uint32_t, typename S::Partial*), hipStream_t stream,
                     typename S::Partial* total) {
  SPT_HIP(hipSetDevice(dn->device));
  typename S::Partial* total_dev = (typename S::Partial*)(parts + S::kPlanes * (size_t)dn->n_parts);
  stage1(dim3(dn->n_parts), dim3(kBlock));
  SPT_HIP(hipGetLastError());
  hipLaunchKernelGGL(stage2, dim3(1), dim3(kBlock), 0, stream, (const double*)parts, dn->n_parts, total_dev);
  SPT_HIP(hipGetLastError());
  *total = S::zero();
  SPT_HIP(hipMemcpyAsync(total, total_dev, sizeof *total, hipMemcpyDeviceToHost, stream));
  SPT_HIP(hipStreamSynchronize(stream));
  return SPT_OK;
}

// Which form an iteration takes: 0 = by step (the tiled form for steps 1 and 2), 1 = plain loads
// always, 2 = the tiled form where it exists. Only the bench library can change them.
int g_form = 0, g_pair_form = 0;

// One iteration's kernel among plain / tiled step 1 / tiled step 2, each last or not: plain(LAST) or
// tiled(STEP, LAST) is called with the choice as integral constants.
template <class Plain, class Tiled>
void launch_form(int32_t step, bool last, int form, const Plain& plain, const Tiled& tiled) {
  using One = std::integral_constant<int, 1>;
  using Two = std::integral_constant<int, 2>;
  const auto either = [&](auto of_last) { last ? of_last(std::true_type{}) : of_last(std::false_type{}); };
  if (form == 1 || step > 2)
    either(plain);
  else if (step == 1)
    either([&](auto l) { tiled(One{}, l); });
  else
    either([&](auto l) { tiled(Two{}, l); });
}

// One a-trous iteration of step `step` from `cur` into cv_out (or, last, into out / se_out).
void launch_atrous(const spt_denoiser* dn, const f4* cur, int32_t step, bool last, const Args& A,
                   f4* cv_out, float* out, float* se_out, int form, hipStream_t stream) {
  const int32_t w = dn->width, h = dn->height;
  const f4 *nz = dn->nz, *av = dn->av;
  const float2* grad = dn->grad;
  launch_form(
      step, last, form,
      [&](auto l) {
        hipLaunchKernelGGL(denoise_atrous_kernel<decltype(l)::value>, grid_of(dn), dim3(kBlock), 0, stream, cur, nz,
                           av, grad, w, h, step, A, cv_out, out, se_out);
      },
      [&](auto s, auto l) {
        hipLaunchKernelGGL((denoise_atrous_lds_kernel<decltype(s)::value, decltype(l)::value>),
                           grid_of(dn, kLdsX, kLdsY), dim3(kBlock), 0, stream, cur, nz, av, grad, w, h, A, cv_out, out,
                           se_out);
      });
}

// One pair iteration of step `step` from (ca, cb) into (ca_out, cb_out) (or, last, into out / se_out / diff).
void launch_atrous_pair(const spt_denoiser* dn, const f4* ca, const f4* cb, int32_t step, bool last, const Args& A,
                        int32_t own, f4* ca_out, f4* cb_out, float* out, float* se_out, float* diff, int form,
                        hipStream_t stream) {
  const int32_t w = dn->width, h = dn->height;
  const f4 *nz = dn->nz, *av = dn->av;
  const float* vtb = dn->vtb;
  const float2* grad = dn->grad;
  launch_form(
      step, last, form,
      [&](auto l) {
        hipLaunchKernelGGL(denoise_atrous_pair_kernel<decltype(l)::value>, grid_of(dn), dim3(kBlock), 0, stream, ca,
                           cb, nz, av, vtb, grad, w, h, step, A, own, ca_out, cb_out, out, se_out, diff);
      },
      [&](auto s, auto l) {
        hipLaunchKernelGGL((denoise_atrous_pair_lds_kernel<decltype(s)::value, decltype(l)::value>),
                           grid_of(dn, kLdsX, kLdsY), dim3(kBlock), 0, stream, ca, cb, nz, av, vtb, grad, w, h, A, own,
                           ca_out, cb_out, out, se_out, diff);
      });
}

void launch_pack(const spt_denoiser* dn, const float* rgb, const float* se, const float* albedo,
                 const float* normal, const float* depth, const Args& A, hipStream_t stream) {
  hipLaunchKernelGGL(denoise_pack_kernel, grid_of(dn), dim3(kBlock), 0, stream, rgb, se, albedo, normal, depth,
                     dn->width, dn->height, A, dn->cv[0], dn->nz, dn->av, dn->grad);
}

void launch_variance(const spt_denoiser* dn, const f4* cur, hipStream_t stream) {
  hipLaunchKernelGGL(denoise_variance_kernel, grid_of(dn), dim3(kBlock), 0, stream, cur, dn->av, dn->width,
                     dn->height);
}

void launch_pair_pack(const spt_denoiser* dn, const float* rgb_a, const float* se_a, const float* rgb_b,
                      const float* se_b, const float* albedo, const float* normal, const float* depth,
                      const Args& A, hipStream_t stream) {
  hipLaunchKernelGGL(denoise_pair_pack_kernel, grid_of(dn), dim3(kBlock), 0, stream, rgb_a, se_a, rgb_b, se_b,
                     albedo, normal, depth, dn->width, dn->height, A, dn->cv[0], dn->cb[0], dn->nz, dn->av, dn->grad);
}

void launch_pair_variance(const spt_denoiser* dn, const f4* ca, const f4* cb, hipStream_t stream) {
  hipLaunchKernelGGL(denoise_pair_variance_kernel, grid_of(dn), dim3(kBlock), 0, stream, ca, cb, dn->av, dn->vtb,
                     dn->width, dn->height);
}

void launch_halves(const spt_denoiser* dn, const f4* ca, const f4* cb, int32_t step, const Args& A, int32_t own,
                   hipStream_t stream) {
  hipLaunchKernelGGL(denoise_atrous_pair_halves_kernel, grid_of(dn), dim3(kBlock), 0, stream, ca, cb,
                     (const f4*)dn->nz, (const f4*)dn->av, (const float*)dn->vtb, (const float2*)dn->grad, dn->width,
                     dn->height, step, A, own, dn->oa, dn->ob);
}

void launch_smooth(const spt_denoiser* dn, const f4* m, int32_t step, const Args& A, int32_t n, f4* m_out,
                   hipStream_t stream) {
  hipLaunchKernelGGL(denoise_bank_smooth_kernel, grid_of(dn), dim3(kBlock), 0, stream, m, (const f4*)dn->nz,
                     (const f4*)dn->av, (const float2*)dn->grad, dn->width, dn->height, step, A, n, m_out);
}

void launch_blend(const spt_denoiser* dn, const f4* m, const Args& A, int32_t n, float* out, float* mse,
                  uint8_t* choice, hipStream_t stream) {
  hipLaunchKernelGGL(denoise_bank_blend_kernel, grid_of(dn), dim3(kBlock), 0, stream, m, (const f4*)dn->nz,
                     (const f4*)dn->av, (const float2*)dn->grad, dn->width, dn->height, A, n, (const float*)dn->outk,
                     dn->outk_stride, out, mse, choice);
}

void launch_error(const spt_denoiser* dn, const float* oa, const float* ob, const float* rgb_a, const float* se_a,
                  const float* rgb_b, const float* se_b, int32_t k, hipStream_t stream) {
  hipLaunchKernelGGL(denoise_bank_error_kernel, dim3(dn->n_parts), dim3(kBlock), 0, stream, oa, ob, rgb_a, se_a,
                     rgb_b, se_b, dn->npix, k, dn->bm[0], dn->outk + (size_t)k * dn->outk_stride);
}

// The filter of five device planes, already validated.
spt_status run(spt_denoiser* dn, const float* rgb, const float* se, const float* albedo,
               const float* normal, const float* depth, const spt_denoise_params* p, float* out,
               float* se_out, hipStream_t stream) {
  SPT_HIP(hipSetDevice(dn->device));
  const size_t bytes = dn->npix * 3 * sizeof(float);
  if (p->iterations == 0) {
    SPT_HIP(hipMemcpyAsync(out, rgb, bytes, hipMemcpyDeviceToDevice, stream));
    if (se_out) SPT_HIP(hipMemcpyAsync(se_out, se, bytes, hipMemcpyDeviceToDevice, stream));
    return SPT_OK;
  }
  const Args A = make_args(p);
  launch_pack(dn, rgb, se, albedo, normal, depth, A, stream);
  for (int32_t it = 0; it < p->iterations; ++it) {
    const f4* cur = dn->cv[it & 1];
    launch_variance(dn, cur, stream);
    const bool last = it == p->iterations - 1;
    launch_atrous(dn, cur, (int32_t)1 << it, last, A, last ? nullptr : dn->cv[(it + 1) & 1],
                  last ? out : nullptr, last ? se_out : nullptr, g_form, stream);
  }
  SPT_HIP(hipGetLastError());
  return SPT_OK;
}

// The pack and the p->iterations > 0 iterations of a pair run over seven device planes. Every step but
// the last goes into the other ping-pong planes; the last is the caller's: last_step(ca, cb, step).
template <class LastStep>
void pair_iterations(spt_denoiser* dn, const float* rgb_a, const float* se_a, const float* rgb_b,
                     const float* se_b, const float* albedo, const float* normal, const float* depth,
                     const spt_denoise_params* p, const Args& A, int32_t own, hipStream_t stream,
                     const LastStep& last_step) {
  launch_pair_pack(dn, rgb_a, se_a, rgb_b, se_b, albedo, normal, depth, A, stream);
  for (int32_t it = 0; it < p->iterations; ++it) {
    const f4 *ca = dn->cv[it & 1], *cb = dn->cb[it & 1];
    launch_pair_variance(dn, ca, cb, stream);
    if (it < p->iterations - 1)
      launch_atrous_pair(dn, ca, cb, (int32_t)1 << it, false, A, own, dn->cv[(it + 1) & 1], dn->cb[(it + 1) & 1],
                         nullptr, nullptr, nullptr, g_pair_form, stream);
    else
      last_step(ca, cb, (int32_t)1 << it);
  }
}

int32_t own_of(uint32_t pair_flags) { return (pair_flags & SPT_DENOISE_PAIR_OWN_WEIGHTS) ? 1 : 0; }

// The pair filter of seven device planes, already validated, the pair scratch in place.
spt_status run_pair(spt_denoiser* dn, const float* rgb_a, const float* se_a, const float* rgb_b,
                    const float* se_b, const float* albedo, const float* normal, const float* depth,
                    const spt_denoise_params* p, uint32_t pair_flags, float* out, float* se_out, float* diff,
                    hipStream_t stream) {
  SPT_HIP(hipSetDevice(dn->device));
  if (p->iterations == 0) {
    hipLaunchKernelGGL(denoise_pair_zero_kernel, dim3(dn->n_parts), dim3(kBlock), 0, stream, rgb_a, se_a, rgb_b,
                       se_b, dn->npix, out, se_out, diff);
  } else {
    const Args A = make_args(p);
    const int32_t own = own_of(pair_flags);
    pair_iterations(dn, rgb_a, se_a, rgb_b, se_b, albedo, normal, depth, p, A, own, stream,
                    [&](const f4* ca, const f4* cb, int32_t step) {
                      launch_atrous_pair(dn, ca, cb, step, true, A, own, nullptr, nullptr, out, se_out, diff,
                                         g_pair_form, stream);
                    });
  }
  SPT_HIP(hipGetLastError());
  return SPT_OK;
}

// The bank of seven device planes, already validated, the pair and the bank scratch in place.
spt_status run_bank(spt_denoiser* dn, const float* rgb_a, const float* se_a, const float* rgb_b,
                    const float* se_b, const float* albedo, const float* normal, const float* depth,
                    const spt_denoise_params* cands, int32_t n_cands, const spt_bank_params* bank, float* out,
                    float* mse, uint8_t* choice, hipStream_t stream) {
  SPT_HIP(hipSetDevice(dn->device));
  const int32_t own = own_of(bank->pair_flags);
  for (int32_t k = 0; k < n_cands; ++k) {
    const spt_denoise_params* p = cands + k;
    const Args A = make_args(p);
    if (p->iterations > 0)
      pair_iterations(dn, rgb_a, se_a, rgb_b, se_b, albedo, normal, depth, p, A, own, stream,
                      [&](const f4* ca, const f4* cb, int32_t step) {
                        launch_halves(dn, ca, cb, step, A, own, stream);
                      });
    // iterations == 0: the halves as given
    launch_error(dn, p->iterations > 0 ? dn->oa : rgb_a, p->iterations > 0 ? dn->ob : rgb_b, rgb_a, se_a, rgb_b,
                 se_b, k, stream);
  }
  const Args A0 = make_args(cands);
  if (cands[n_cands - 1].iterations == 0)  // no candidate's pack left the guides in the scratch
    launch_pair_pack(dn, rgb_a, se_a, rgb_b, se_b, albedo, normal, depth, A0, stream);
  const f4* cur = dn->bm[0];
  for (int32_t it = 0; it < bank->error_iterations; ++it) {
    f4* nxt = dn->bm[(it + 1) & 1];
    launch_smooth(dn, cur, (int32_t)1 << it, A0, n_cands, nxt, stream);
    cur = nxt;
  }
  launch_blend(dn, cur, A0, n_cands, out, mse, choice, stream);
  SPT_HIP(hipGetLastError());
  return SPT_OK;
}

// What a film-pair call (`who`) asks of its two films and its guide, then the scratch and the seven
// planes resolved into it. A film's own faults are reported as film_pair_denoise's by both calls.
spt_status stage_pair_films(const char* who, const spt_film* film_a, const spt_film* film_b,
                            const spt_guide* guide, spt_denoiser* dn, bool bank, void* stream) {
  const auto bad = [who](const char* msg) { return fail(SPT_ERR_INVALID_ARG, std::string(who) + ": " + msg); };
  if (film_a == film_b) return bad("the two halves are one film");
  if (guide->samples_done == 0) return bad("the guide holds no sample");
  for (const spt_film* film : {film_a, film_b}) {
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
  }
  if (film_a->spp_total != film_b->spp_total) return bad("the films' spp_total differ");
  SPT_TRY(pair_scratch(dn));
  if (bank) SPT_TRY(bank_scratch(dn));
  SPT_TRY(spt_film_resolve(film_a, dn->rgb, stream));
  SPT_TRY(spt_film_noise_map(film_a, dn->se, stream));
  SPT_TRY(spt_film_resolve(film_b, dn->rgb_b, stream));
  SPT_TRY(spt_film_noise_map(film_b, dn->se_b, stream));
  return spt_guide_resolve(guide, dn->albedo, dn->normal, dn->depth, nullptr, stream);
}

}  // namespace

extern "C" spt_status spt_denoiser_create(int32_t device, int32_t width, int32_t height,
                                          spt_denoiser** out) {
  if (!out) return fail(SPT_ERR_INVALID_ARG, "null argument");
  if (const char* e = size_error(width, height)) return fail(SPT_ERR_INVALID_ARG, std::string("denoiser: ") + e);
  if (tiles_of(width, height, kTileX, kTileY) > kMaxTiles || tiles_of(width, height, kLdsX, kLdsY) > kMaxTiles)
    return fail(SPT_ERR_INVALID_ARG, "denoiser: the image is too narrow or too flat for one launch (spt.h)");
  SPT_TRY(spt::open_device(device));
  spt_denoiser* dn = new spt_denoiser();
  dn->device = device;
  dn->width = width;
  dn->height = height;
  dn->npix = (size_t)width * (size_t)height;
  // 4 f4 planes, the gradient, 13 floats of film planes: 124 bytes per pixel, 16-byte planes first
  const spt_status st = alloc_scratch(dn, &dn->base, "denoiser", [dn](Carver& c) {
    dn->cv[0] = c.quad();
    dn->cv[1] = c.quad();
    dn->nz = c.quad();
    dn->av = c.quad();
    dn->grad = c.take<float2>(c.n + (c.n & 1));
    dn->rgb = c.floats(3);
    dn->se = c.floats(3);
    dn->albedo = c.floats(3);
    dn->normal = c.floats(3);
    dn->depth = c.floats(1);
  });
  if (st != SPT_OK) {
    delete dn;
    return st;
  }
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
  SPT_TRY(check_call(dn, "denoise", params_error(params), {out_dev, se_out_dev},
                     {rgb_dev, se_dev, albedo_dev, normal_dev, depth_dev}));
  return run(dn, rgb_dev, se_dev, albedo_dev, normal_dev, depth_dev, params, out_dev, se_out_dev,
             (hipStream_t)stream);
}

extern "C" spt_status spt_film_denoise(const spt_film* film, const spt_guide* guide, spt_denoiser* dn,
                                       const spt_denoise_params* params, float* out_dev,
                                       float* se_out_dev, void* stream) {
  if (!film || !guide) return fail(SPT_ERR_INVALID_ARG, "film_denoise: null film or guide");
  SPT_TRY(check_call(dn, "denoise", params_error(params), {out_dev, se_out_dev}, {}));
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
  return run(dn, dn->rgb, dn->se, dn->albedo, dn->normal, dn->depth, params, out_dev, se_out_dev,
             (hipStream_t)stream);
}

extern "C" spt_status spt_denoise_pair_async(spt_denoiser* dn, const float* rgb_a_dev, const float* se_a_dev,
                                             const float* rgb_b_dev, const float* se_b_dev,
                                             const float* albedo_dev, const float* normal_dev,
                                             const float* depth_dev, const spt_denoise_params* params,
                                             uint32_t pair_flags, float* out_dev, float* se_out_dev,
                                             float* diff_dev, void* stream) {
  SPT_TRY(check_call(dn, "denoise_pair", pair_error(params, pair_flags), {out_dev, se_out_dev, diff_dev},
                     {rgb_a_dev, se_a_dev, rgb_b_dev, se_b_dev, albedo_dev, normal_dev, depth_dev}));
  SPT_TRY(pair_scratch(dn));
  return run_pair(dn, rgb_a_dev, se_a_dev, rgb_b_dev, se_b_dev, albedo_dev, normal_dev, depth_dev, params,
                  pair_flags, out_dev, se_out_dev, diff_dev, (hipStream_t)stream);
}

extern "C" spt_status spt_film_pair_denoise(const spt_film* film_a, const spt_film* film_b,
                                            const spt_guide* guide, spt_denoiser* dn,
                                            const spt_denoise_params* params, uint32_t pair_flags,
                                            float* out_dev, float* se_out_dev, float* diff_dev, void* stream) {
  if (!film_a || !film_b || !guide) return fail(SPT_ERR_INVALID_ARG, "film_pair_denoise: null film or guide");
  SPT_TRY(check_call(dn, "denoise_pair", pair_error(params, pair_flags), {out_dev, se_out_dev, diff_dev}, {}));
  SPT_TRY(stage_pair_films("film_pair_denoise", film_a, film_b, guide, dn, false, stream));
  return run_pair(dn, dn->rgb, dn->se, dn->rgb_b, dn->se_b, dn->albedo, dn->normal, dn->depth, params,
                  pair_flags, out_dev, se_out_dev, diff_dev, (hipStream_t)stream);
}

extern "C" spt_status spt_denoise_pair_summary(spt_denoiser* dn, const float* diff_dev, spt_pair_summary* out,
                                               void* stream_v) {
  if (!dn || !diff_dev || !out) return fail(SPT_ERR_INVALID_ARG, "denoise_pair_summary: null argument");
  SPT_TRY(pair_scratch(dn));
  hipStream_t stream = (hipStream_t)stream_v;
  PairPartial total;
  SPT_TRY(sum_image<PairSum>(
      dn, dn->parts,
      [&](dim3 grid, dim3 block) {
        hipLaunchKernelGGL(denoise_pair_partials_kernel, grid, block, 0, stream, diff_dev, dn->npix, dn->parts);
      },
      denoise_pair_total_kernel, stream, &total));
  pair_summary_finish(total, dn->npix, out);
  return SPT_OK;
}

extern "C" spt_status spt_denoise_bank_async(spt_denoiser* dn, const float* rgb_a_dev, const float* se_a_dev,
                                             const float* rgb_b_dev, const float* se_b_dev,
                                             const float* albedo_dev, const float* normal_dev,
                                             const float* depth_dev, const spt_denoise_params* cands,
                                             int32_t n_cands, const spt_bank_params* bank, float* out_dev,
                                             float* mse_dev, uint8_t* choice_dev, void* stream) {
  SPT_TRY(check_call(dn, "denoise_bank", bank_error(cands, n_cands, bank), {out_dev, mse_dev, choice_dev},
                     {rgb_a_dev, se_a_dev, rgb_b_dev, se_b_dev, albedo_dev, normal_dev, depth_dev}));
  SPT_TRY(pair_scratch(dn));
  SPT_TRY(bank_scratch(dn));
  return run_bank(dn, rgb_a_dev, se_a_dev, rgb_b_dev, se_b_dev, albedo_dev, normal_dev, depth_dev, cands, n_cands,
                  bank, out_dev, mse_dev, choice_dev, (hipStream_t)stream);
}

extern "C" spt_status spt_film_pair_denoise_bank(const spt_film* film_a, const spt_film* film_b,
                                                 const spt_guide* guide, spt_denoiser* dn,
                                                 const spt_denoise_params* cands, int32_t n_cands,
                                                 const spt_bank_params* bank, float* out_dev, float* mse_dev,
                                                 uint8_t* choice_dev, void* stream) {
  if (!film_a || !film_b || !guide) return fail(SPT_ERR_INVALID_ARG, "film_pair_denoise_bank: null film or guide");
  SPT_TRY(check_call(dn, "denoise_bank", bank_error(cands, n_cands, bank), {out_dev, mse_dev, choice_dev}, {}));
  SPT_TRY(stage_pair_films("film_pair_denoise_bank", film_a, film_b, guide, dn, true, stream));
  return run_bank(dn, dn->rgb, dn->se, dn->rgb_b, dn->se_b, dn->albedo, dn->normal, dn->depth, cands, n_cands,
                  bank, out_dev, mse_dev, choice_dev, (hipStream_t)stream);
}

extern "C" spt_status spt_denoise_bank_summary(spt_denoiser* dn, const float* mse_dev, const uint8_t* choice_dev,
                                               spt_bank_summary* out, void* stream_v) {
  if (!dn || !mse_dev || !choice_dev || !out) return fail(SPT_ERR_INVALID_ARG, "denoise_bank_summary: null argument");
  SPT_TRY(pair_scratch(dn));
  SPT_TRY(bank_scratch(dn));
  hipStream_t stream = (hipStream_t)stream_v;
  BankPartial total;
  SPT_TRY(sum_image<BankSum>(
      dn, dn->bank_parts,
      [&](dim3 grid, dim3 block) {
        hipLaunchKernelGGL(denoise_bank_partials_kernel, grid, block, 0, stream, mse_dev, choice_dev, dn->npix,
                           dn->bank_parts);
      },
      denoise_bank_total_kernel, stream, &total));
  bank_summary_finish(total, dn->npix, out);
  return SPT_OK;
}

#ifdef SPT_DENOISE_BENCH  // tools/denoise_bench.py's library only: never in the shipped libspt.so
namespace {
// The form setters' body. 0 = by step, 1 = plain loads always, 2 = the tiled form where it exists.
spt_status set_form(int* g, int32_t form) {
  if (form < 0 || form > 2) return fail(SPT_ERR_INVALID_ARG, "form: 0, 1 or 2");
  *g = form;
  return SPT_OK;
}
// What the single and the pair bench kernels ask of which, step (a power of two up to 32) and form.
bool bench_args_ok(int32_t which, int32_t step, int32_t form) {
  return which >= 0 && which <= 3 && step >= 1 && step <= 32 && !(step & (step - 1)) && form >= 1 && form <= 2 &&
         !(form == 2 && step > 2);
}
}  // namespace

extern "C" spt_status spt_denoise_bench_form(int32_t form) { return set_form(&g_form, form); }
extern "C" spt_status spt_denoise_pair_bench_form(int32_t form) { return set_form(&g_pair_form, form); }

// One launch of one kernel on the denoiser's scratch, for a timing of that kernel alone. which: 0 the
// pack of the five planes, 1 the variance pass over cv[0], 2 an a-trous pass cv[0] -> cv[1], 3 the
// a-trous pass with the finish fused in, cv[0] -> out / se_out. form as above (plain or tiled).
extern "C" spt_status spt_denoise_bench_kernel(spt_denoiser* dn, int32_t which, int32_t step, int32_t form,
                                               const float* rgb, const float* se, const float* albedo,
                                               const float* normal, const float* depth,
                                               const spt_denoise_params* params, float* out, float* se_out,
                                               void* stream_v) {
  if (!dn || params_error(params) || !bench_args_ok(which, step, form))
    return fail(SPT_ERR_INVALID_ARG, "bench_kernel: bad argument");
  hipStream_t stream = (hipStream_t)stream_v;
  const Args A = make_args(params);
  const bool last = which == 3;
  SPT_HIP(hipSetDevice(dn->device));
  if (which == 0)
    launch_pack(dn, rgb, se, albedo, normal, depth, A, stream);
  else if (which == 1)
    launch_variance(dn, dn->cv[0], stream);
  else
    launch_atrous(dn, dn->cv[0], step, last, A, last ? nullptr : dn->cv[1], last ? out : nullptr,
                  last ? se_out : nullptr, form, stream);
  SPT_HIP(hipGetLastError());
  return SPT_OK;
}
// The same for the pair filter. which: 0 the pair pack of the seven planes, 1 the pair variance pass over
// (cv[0], cb[0]), 2 a pair a-trous pass into (cv[1], cb[1]), 3 the pair a-trous pass with the finish fused
// in, into out / se_out / diff.
extern "C" spt_status spt_denoise_pair_bench_kernel(spt_denoiser* dn, int32_t which, int32_t step, int32_t form,
                                                    const float* rgb_a, const float* se_a, const float* rgb_b,
                                                    const float* se_b, const float* albedo, const float* normal,
                                                    const float* depth, const spt_denoise_params* params,
                                                    uint32_t pair_flags, float* out, float* se_out, float* diff,
                                                    void* stream_v) {
  if (!dn || pair_error(params, pair_flags) || !bench_args_ok(which, step, form))
    return fail(SPT_ERR_INVALID_ARG, "pair_bench_kernel: bad argument");
  SPT_TRY(pair_scratch(dn));
  hipStream_t stream = (hipStream_t)stream_v;
  const Args A = make_args(params);
  const bool last = which == 3;
  SPT_HIP(hipSetDevice(dn->device));
  if (which == 0)
    launch_pair_pack(dn, rgb_a, se_a, rgb_b, se_b, albedo, normal, depth, A, stream);
  else if (which == 1)
    launch_pair_variance(dn, dn->cv[0], dn->cb[0], stream);
  else
    launch_atrous_pair(dn, dn->cv[0], dn->cb[0], step, last, A, own_of(pair_flags), last ? nullptr : dn->cv[1],
                       last ? nullptr : dn->cb[1], last ? out : nullptr, last ? se_out : nullptr,
                       last ? diff : nullptr, form, stream);
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
  if (!dn || !dn->bank_base || params_error(params) || !bench_args_ok(which, step, 1) || n_cands < 1 ||
      n_cands > kMaxCands || (which == 2 && !out) || (which == 0 && (!rgb_a || !se_a || !rgb_b || !se_b)))
    return fail(SPT_ERR_INVALID_ARG, "bank_bench_kernel: bad argument, or no bank call before");
  hipStream_t stream = (hipStream_t)stream_v;
  const Args A = make_args(params);
  SPT_HIP(hipSetDevice(dn->device));
  if (which == 0)
    launch_error(dn, dn->oa, dn->ob, rgb_a, se_a, rgb_b, se_b, 0, stream);
  else if (which == 1)
    launch_smooth(dn, dn->bm[0], step, A, n_cands, dn->bm[1], stream);
  else if (which == 2)
    launch_blend(dn, dn->bm[0], A, n_cands, out, mse, choice, stream);
  else
    launch_halves(dn, dn->cv[0], dn->cb[0], step, A, 1, stream);
  SPT_HIP(hipGetLastError());
  return SPT_OK;
}
#endif

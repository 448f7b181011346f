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
//   noise       a noise film's moment plane (accumulate also does M2 += P^2, 128 bits), its error map
//               and the image's RMSE estimate (a two-stage reduction in a fixed order)
//   adaptive    an adaptive film's counts plane: passes over the active list scatter their sums, the
//               selection retires pixels and compacts the rest, and the resolve, the map and the
//               summary take every pixel's own batch count (the last section of this file)
//   pool        the error pooled over a pixel's neighbourhood: its map, and the selection that retires
//               on it (two streaming passes through a scratch plane of row sums)
//
// All three stream: one pass over the sums at 16 bytes per access (two sums, or four floats),
// 256 threads per block, no reuse -- HBM-bound. -ffp-contract=off (the Makefile) keeps the preview two
// separate multiplies, as spt_film_resolve_host and a numpy restatement compute it. The per-element
// arithmetic is spt_film_math.h's, shared with the CPU statements (spt_film_host.cpp).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "spt_film.h"
#include "spt_film_math.h"

using spt::copy_and_wait;
using spt::fail;

namespace {

using namespace spt_film_math;
constexpr int kBlock = 256;
constexpr uint32_t kQuadLanes = 192;  // 3 * kBlock sums per block / 4 per lane

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

// The same wait for one 16-byte load (an element of the moment plane).
__device__ __forceinline__ void load_landed(ulonglong2& a) {
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(a.x), "+v"(a.y)::"memory");
}

// One sum of the accumulate's phase 2 (a run's unaligned head or tail).
template <bool NOISE>
__device__ __forceinline__ void acc_one(u64* __restrict__ film, const u64* __restrict__ accum,
                                        ulonglong2* __restrict__ m2, float* __restrict__ rgb,
                                        size_t e, u64 add, bool capped, float r, int full) {
  float f = __builtin_nanf("");
  if (!capped) {
    const u64 v = film[e] + add + accum[e];
    film[e] = v;
    f = film_resolve1(v, r, full);
    if constexpr (NOISE) {  // the pass's own sum, squared into the moment plane
      ulonglong2 m = m2[e];
      load_landed(m);
      m2_add_square(m, add + accum[e]);
      m2[e] = m;
    }
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
//
// NOISE (a noise film, m2 = its moment plane): the pass's own sum P = slots + accumulator of every
// element is also squared into m2[e] (+= P^2, 128 bits): one more 16-byte load and store per sum,
// as a group of its own behind the film's (loads, the full wait, stores). m2 is the last parameter
// and every NOISE step is compiled out of the <false> instantiation, the one a plain film launches:
// its instructions are what they were before the moment plane existed.
template <bool NOISE>
__global__ void __launch_bounds__(kBlock)
film_accumulate_kernel(const u64* __restrict__ accum, const u64* __restrict__ slots,
                       u64* __restrict__ film, float* __restrict__ rgb, uint32_t npix,
                       uint32_t n_chunks, uint32_t scr_k, uint32_t scr_q,
                       const u64* __restrict__ stats, float r, int full, int rgb_vec,
                       ulonglong2* __restrict__ m2) {
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
      if constexpr (NOISE) {  // a second group of the same shape: four loads, the full wait, four stores
        ulonglong2 q0 = m2[e], q1 = m2[e + 1], q2 = m2[e + 2], q3 = m2[e + 3];
        loads_landed(q0, q1);
        loads_landed(q2, q3);
        m2_add_square(q0, a0.x + s[0]);
        m2_add_square(q1, a0.y + s[1]);
        m2_add_square(q2, a1.x + s[2]);
        m2_add_square(q3, a1.y + s[3]);
        m2[e] = q0;
        m2[e + 1] = q1;
        m2[e + 2] = q2;
        m2[e + 3] = q3;
      }
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
    if constexpr (NOISE) {  // at most three sums at either end: unrolled, no loop around a 16-byte load
#pragma unroll
      for (uint32_t u = 0; u < 3; ++u)
        if (u < h) acc_one<true>(film, accum, m2, rgb, e0 + u, capped ? 0ull : s[u], capped, r, full);
#pragma unroll
      for (uint32_t u = 0; u < 3; ++u) {
        const uint32_t idx = body_end + u;
        if (idx < n) acc_one<true>(film, accum, m2, rgb, e0 + idx, capped ? 0ull : s[idx], capped, r, full);
      }
    } else {
      for (uint32_t idx = 0; idx < h; ++idx)
        acc_one<false>(film, accum, m2, rgb, e0 + idx, capped ? 0ull : s[idx], capped, r, full);
      for (uint32_t idx = body_end; idx < n; ++idx)
        acc_one<false>(film, accum, m2, rgb, e0 + idx, capped ? 0ull : s[idx], capped, r, full);
    }
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

// dst.M2 += src.M2 with carry: one 128-bit element per thread, 16-byte loads and store.
__global__ void __launch_bounds__(kBlock)
film_merge_m2_kernel(ulonglong2* dst, const ulonglong2* src, size_t n) {
  const size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (e < n) {
    ulonglong2 d = dst[e], s = src[e];
    loads_landed(d, s);
    const u64 lo = d.x + s.x;
    d.y += s.y + (u64)(lo < s.x);
    d.x = lo;
    dst[e] = d;
  }
}

// The error map: one element per thread, its NoiseArgs from the count source (UniformCount: a noise
// film's one, passed by value; PixelCount: the row of the pixel's own count, an adaptive film).
template <class Counts>
__global__ void __launch_bounds__(kBlock)
film_noise_map_kernel(const u64* sums, const ulonglong2* m2, float* se, size_t n, Counts cs) {
  const size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (e < n) {
    ulonglong2 m = m2[e];
    load_landed(m);
    const NoiseArgs A = cs.at(e / 3);
    bool c;
    se[e] = noise_se(noise_d(sums[e], m, A, &c), A);
  }
}

// p[0] = the block's 256 partials combined pairwise, in an order fixed by the thread index alone.
__device__ __forceinline__ void noise_block_reduce(NoisePartial* p) {
  for (uint32_t w = kBlock / 2; w > 0; w >>= 1) {
    __syncthreads();
    if (threadIdx.x < w) {
      NoisePartial& a = p[threadIdx.x];
      const NoisePartial& b = p[threadIdx.x + w];
      a.s[0] += b.s[0];
      a.s[1] += b.s[1];
      a.s[2] += b.s[2];
      a.se_max = fmaxf(a.se_max, b.se_max);
      a.clamped += b.clamped;
    }
  }
  __syncthreads();
}

// Stage 1: one pixel per thread (three sums, three moments), one partial per block. The partials
// are five planes of nb = gridDim.x 8-byte words (s[0], s[1], s[2], se_max as a double, clamped), so
// that stage 2 reads them with 8-byte loads. The pixel's NoiseArgs come from the count source.
template <class Counts>
__global__ void __launch_bounds__(kBlock)
film_noise_partials_kernel(const u64* sums, const ulonglong2* m2, size_t npix, Counts cs,
                           double* out) {
  __shared__ NoisePartial s_p[kBlock];
  const size_t px = (size_t)blockIdx.x * kBlock + threadIdx.x;
  NoisePartial v{};
  if (px < npix) {
    ulonglong2 m0 = m2[3 * px], m1 = m2[3 * px + 1], mm = m2[3 * px + 2];
    loads_landed(m0, m1);
    load_landed(mm);
    const ulonglong2 m[3] = {m0, m1, mm};
    const NoiseArgs A = cs.at(px);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      bool cl;
      const double d = noise_d(sums[3 * px + c], m[c], A, &cl);
      v.s[c] = d * A.k2;
      v.se_max = fmaxf(v.se_max, noise_se(d, A));
      v.clamped += cl ? 1u : 0u;
    }
  }
  s_p[threadIdx.x] = v;
  noise_block_reduce(s_p);
  if (threadIdx.x == 0) {
    const size_t nb = gridDim.x;
    out[blockIdx.x] = s_p[0].s[0];
    out[nb + blockIdx.x] = s_p[0].s[1];
    out[2 * nb + blockIdx.x] = s_p[0].s[2];
    out[3 * nb + blockIdx.x] = (double)s_p[0].se_max;
    ((u64*)out)[4 * nb + blockIdx.x] = s_p[0].clamped;
  }
}

// Stage 2, one block: thread t adds the partials t, t + 256, ... in that order; *total = the image's.
__global__ void __launch_bounds__(kBlock)
film_noise_total_kernel(const double* parts, uint32_t n, NoisePartial* total) {
  __shared__ NoisePartial s_p[kBlock];
  NoisePartial v{};
  for (uint32_t i = threadIdx.x; i < n; i += kBlock) {
    v.s[0] += parts[i];
    v.s[1] += parts[(size_t)n + i];
    v.s[2] += parts[2 * (size_t)n + i];
    v.se_max = fmaxf(v.se_max, (float)parts[3 * (size_t)n + i]);
    v.clamped += ((const u64*)parts)[4 * (size_t)n + i];
  }
  s_p[threadIdx.x] = v;
  noise_block_reduce(s_p);
  if (threadIdx.x == 0) *total = s_p[0];
}

// ---- the adaptive film's kernels: listed accumulate, per-pixel resolve, selection ----

// The pass over the active list: thread t sums the slots of unit-order virtual pixel t (as the
// unlisted kernel's phase 1), v = its spread virtual pixel (the accumulator's index), g = list[v]
// the film's pixel. A scatter: 8-byte accesses of the sums, one 16-byte load and store per moment
// (straight-line, the full wait before any register is used), the pixel's count + 1. No two threads
// share a g (the list holds every pixel once). A guarded launch adds nothing.
// The slot sum is written out in both accumulate kernels: called as a shared inline function the loop
// is rotated before it is inlined, and film_accumulate_kernel comes out with its blocks in another
// order and other registers (HISTORY.md, round 15); its instructions are to stay the parent's.
__global__ void __launch_bounds__(kBlock)
film_accumulate_listed_kernel(const u64* __restrict__ accum, const u64* __restrict__ slots,
                              u64* __restrict__ film, ulonglong2* __restrict__ m2,
                              uint32_t* __restrict__ cnt, const uint32_t* __restrict__ list,
                              uint32_t npix, uint32_t n_chunks, uint32_t scr_k, uint32_t scr_q,
                              const u64* __restrict__ stats) {
  const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (stats[0] != 0 || t >= npix) return;
  u64 v0 = 0, v1 = 0, v2 = 0;
  for (uint32_t j = 0; j < n_chunks; ++j) {
    const u64* q = slots + 3ull * ((size_t)j * npix + t);
    v0 += q[0];
    v1 += q[1];
    v2 += q[2];
  }
  const uint32_t v = ((uint32_t)t & ((1u << scr_k) - 1u)) * scr_q + ((uint32_t)t >> scr_k);
  const size_t g = list[v];
  v0 += accum[3ull * v];
  v1 += accum[3ull * v + 1];
  v2 += accum[3ull * v + 2];
  ulonglong2 q0 = m2[3 * g], q1 = m2[3 * g + 1], q2 = m2[3 * g + 2];
  loads_landed(q0, q1);
  load_landed(q2);
  film[3 * g] += v0;
  film[3 * g + 1] += v1;
  film[3 * g + 2] += v2;
  m2_add_square(q0, v0);
  m2_add_square(q1, v1);
  m2_add_square(q2, v2);
  m2[3 * g] = q0;
  m2[3 * g + 1] = q1;
  m2[3 * g + 2] = q2;
  cnt[g] += 1u;
}

// film -> float with every pixel's own factor: one pixel per thread. stats (optional): the words of
// the pass this resolve follows; a guarded pass leaves rgb all NaN, as the unlisted pass does.
__global__ void __launch_bounds__(kBlock)
film_adapt_resolve_kernel(const u64* __restrict__ sums, const uint32_t* __restrict__ cnt,
                          const NoiseArgs* __restrict__ tab, float* __restrict__ rgb, size_t npix,
                          const u64* __restrict__ stats) {
  const size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= npix) return;
  if (stats && stats[0] != 0) {
    rgb[3 * p] = rgb[3 * p + 1] = rgb[3 * p + 2] = __builtin_nanf("");
    return;
  }
  const NoiseArgs A = PixelCount{cnt, tab}.at(p);
  rgb[3 * p] = film_resolve1(sums[3 * p], A.r, A.full);
  rgb[3 * p + 1] = film_resolve1(sums[3 * p + 1], A.r, A.full);
  rgb[3 * p + 2] = film_resolve1(sums[3 * p + 2], A.r, A.full);
}

// The selection's first step: an active pixel that the mask drops, or none of whose channels is above
// the threshold, gets bit 31. One pixel per thread; the moments are loaded by every thread in range
// (straight-line), used or not.
__global__ void __launch_bounds__(kBlock)
film_adapt_mark_kernel(const u64* sums, const ulonglong2* m2, uint32_t* cnt, const NoiseArgs* tab,
                       const uint8_t* keep, size_t npix, double thr2, int all) {
  const size_t px = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (px >= npix) return;
  ulonglong2 m0 = m2[3 * px], m1 = m2[3 * px + 1], mm = m2[3 * px + 2];
  loads_landed(m0, m1);
  load_landed(mm);
  const uint32_t c = cnt[px];
  if (c & kRetired) return;
  bool stay = keep ? keep[px] != 0 : true;
  if (stay && !all) {
    const ulonglong2 m[3] = {m0, m1, mm};
    const u64 S[3] = {sums[3 * px], sums[3 * px + 1], sums[3 * px + 2]};
    stay = adapt_noisy(S, m, PixelCount{cnt, tab}.row(c), thr2);
  }
  if (!stay) cnt[px] = c | kRetired;
}

// The compaction of the active pixels into the ascending list, in three kernels and without an
// atomic: (1) every block counts its active pixels from its waves' ballots, (2) one block turns the
// counts into exclusive offsets (counts[nblk] = the total), (3) every active pixel goes to its
// block's offset + the waves before it + its rank among its wave's active lanes.
__device__ __forceinline__ uint32_t ballot_rank(u64 b) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}

__global__ void __launch_bounds__(kBlock)
film_adapt_count_kernel(const uint32_t* cnt, size_t npix, uint32_t* counts) {
  __shared__ uint32_t s_w[kBlock / 64];
  const size_t px = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const bool active = px < npix && !(cnt[px] & kRetired);
  const u64 b = __ballot(active);
  if ((threadIdx.x & 63u) == 0) s_w[threadIdx.x >> 6] = (uint32_t)__popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

__global__ void __launch_bounds__(kBlock)
film_adapt_scan_kernel(uint32_t* counts, uint32_t nblk) {
  __shared__ uint32_t s_t[kBlock];
  const uint32_t per = (nblk + kBlock - 1) / kBlock;  // a thread's run of consecutive blocks
  const uint32_t b0 = min(threadIdx.x * per, nblk), b1 = min(b0 + per, nblk);
  uint32_t sum = 0;
  for (uint32_t i = b0; i < b1; ++i) sum += counts[i];
  s_t[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (uint32_t i = 0; i < (uint32_t)kBlock; ++i) {
      const uint32_t t = s_t[i];
      s_t[i] = run;
      run += t;
    }
    counts[nblk] = run;
  }
  __syncthreads();
  uint32_t run = s_t[threadIdx.x];
  for (uint32_t i = b0; i < b1; ++i) {
    const uint32_t t = counts[i];
    counts[i] = run;
    run += t;
  }
}

__global__ void __launch_bounds__(kBlock)
film_adapt_scatter_kernel(const uint32_t* cnt, size_t npix, const uint32_t* offs, uint32_t* list) {
  __shared__ uint32_t s_w[kBlock / 64];
  const size_t px = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const bool active = px < npix && !(cnt[px] & kRetired);
  const u64 b = __ballot(active);
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) s_w[wave] = (uint32_t)__popcll(b);
  __syncthreads();
  uint32_t at = offs[blockIdx.x];
  for (uint32_t w = 0; w < wave; ++w) at += s_w[w];
  if (active) list[at + ballot_rank(b)] = (uint32_t)px;  // at + rank < the total <= npix
}

// ---- the pooled error's kernels (spt.h SPT_HAS_FILM_POOL) ----
//
// Two streaming passes. (1) film_pool_rows_kernel reads what the error map reads (24 B of sums, 48 B of
// moments, the count), evaluates u once per place of its tile and forms the row sums h over the
// window's columns through LDS. (2) film_pool_mark_kernel / film_pool_map_kernel add h over the
// window's rows and decide. Pass 2 reads only the scratch planes pass 1 wrote and its own pixel's
// count, so the selection marks in place and still decides every pixel from the planes as they were
// before it marked anything. The additions run in the stated order (spt.h): no atomics, no sliding sums.

// A block covers kBlock consecutive columns of one row, the R-column halo on either side included:
// thread t evaluates column tile * (kBlock - 2R) - R + t (0.0 and uncounted outside the row: u is
// never -0.0, so adding 0.0 for a clipped column changes no bit) and the kBlock - 2R threads in the
// middle add their 2R + 1 columns, ascending. LDS: three planes of doubles, one per channel, so that a
// wave's 8-byte reads are consecutive, and one of counts: 7 KB.
template <class Counts>
__global__ void __launch_bounds__(kBlock)
film_pool_rows_kernel(const u64* __restrict__ sums, const ulonglong2* __restrict__ m2, Counts cs,
                      uint32_t w, uint32_t tiles, uint32_t R, size_t npix, double* __restrict__ u_out,
                      double* __restrict__ h_out, uint32_t* __restrict__ hn_out) {
  __shared__ double s_u[3][kBlock];
  __shared__ uint32_t s_n[kBlock];
  const uint32_t t = threadIdx.x;
  const uint32_t row = blockIdx.x / tiles, tile = blockIdx.x - row * tiles;
  const int64_t x = (int64_t)tile * (int64_t)(kBlock - 2u * R) - (int64_t)R + (int64_t)t;
  const bool in = x >= 0 && x < (int64_t)w;
  const size_t px = (size_t)row * w + (size_t)(in ? x : 0);
  double u0 = 0.0, u1 = 0.0, u2 = 0.0;
  uint32_t counted = 0;
  if (in) {
    ulonglong2 m0 = m2[3 * px], m1 = m2[3 * px + 1], mm = m2[3 * px + 2];
    loads_landed(m0, m1);
    load_landed(mm);
    const NoiseArgs A = cs.at(px);
    u0 = pool_u(sums[3 * px], m0, A);
    u1 = pool_u(sums[3 * px + 1], m1, A);
    u2 = pool_u(sums[3 * px + 2], mm, A);
    counted = A.B >= 2 ? 1u : 0u;
  }
  s_u[0][t] = u0;
  s_u[1][t] = u1;
  s_u[2][t] = u2;
  s_n[t] = counted;
  __syncthreads();
  if (!in || t < R || t >= kBlock - R) return;
  double h0 = 0.0, h1 = 0.0, h2 = 0.0;
  uint32_t n = 0;
  for (uint32_t j = t - R; j <= t + R; ++j) {  // inside [0, kBlock): R <= t < kBlock - R
    h0 = h0 + s_u[0][j];
    h1 = h1 + s_u[1][j];
    h2 = h2 + s_u[2][j];
    n += s_n[j];
  }
  u_out[px] = u0;
  u_out[npix + px] = u1;
  u_out[2 * npix + px] = u2;
  h_out[px] = h0;
  h_out[npix + px] = h1;
  h_out[2 * npix + px] = h2;
  hn_out[px] = n;
}

// g and n of pixel px: the row sums of its column over the window's rows, ascending; the centre out
// on request. u and h are the planes of film_pool_rows_kernel.
__device__ __forceinline__ void pool_gather(const double* __restrict__ u, const double* __restrict__ h,
                                            const uint32_t* __restrict__ hn, size_t npix, uint32_t w,
                                            uint32_t rows, int32_t band_rows, int32_t R, uint32_t flags,
                                            size_t px, bool counted, double g[3], uint32_t* n) {
  const int32_t y = (int32_t)((uint32_t)px / w);  // a film has at most 2^32 - 1 pixels
  int32_t y0, y1;
  pool_row_window(y, (int32_t)rows, band_rows, R, &y0, &y1);
  g[0] = g[1] = g[2] = 0.0;
  *n = 0;
  size_t q = px - (size_t)(y - y0) * w;
  for (int32_t yy = y0; yy <= y1; ++yy, q += w) {
    g[0] = g[0] + h[q];
    g[1] = g[1] + h[npix + q];
    g[2] = g[2] + h[2 * npix + q];
    *n += hn[q];
  }
  if (flags & SPT_POOL_EXCLUDE_CENTER) {
    const double uc[3] = {u[px], u[npix + px], u[2 * npix + px]};
    pool_exclude_center(g, n, uc, counted);
  }
}

// The pooled selection's mark: film_adapt_mark_kernel with the pooled clause. One pixel per thread.
// Where the window counts nothing the pixel's own rule decides (rare: the moments are loaded there,
// straight-line behind the full wait).
__global__ void __launch_bounds__(kBlock)
film_pool_mark_kernel(const u64* __restrict__ sums, const ulonglong2* __restrict__ m2,
                      uint32_t* __restrict__ cnt, const NoiseArgs* __restrict__ tab,
                      const uint8_t* __restrict__ keep, const double* __restrict__ u,
                      const double* __restrict__ h, const uint32_t* __restrict__ hn, size_t npix,
                      uint32_t w, uint32_t rows, int32_t band_rows, int32_t R, uint32_t flags,
                      double thr2) {
  const size_t px = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (px >= npix) return;
  const uint32_t c = cnt[px];
  if (c & kRetired) return;
  bool stay = keep ? keep[px] != 0 : true;
  if (stay) {
    double g[3];
    uint32_t n;
    pool_gather(u, h, hn, npix, w, rows, band_rows, R, flags, px, c >= 2u, g, &n);
    if (n) {
      stay = pool_noisy(g, n, (u64)c, thr2);
    } else {
      ulonglong2 m0 = m2[3 * px], m1 = m2[3 * px + 1], mm = m2[3 * px + 2];
      loads_landed(m0, m1);
      load_landed(mm);
      const ulonglong2 m[3] = {m0, m1, mm};
      const u64 S[3] = {sums[3 * px], sums[3 * px + 1], sums[3 * px + 2]};
      stay = adapt_noisy(S, m, PixelCount{cnt, tab}.row(c), thr2);
    }
  }
  if (!stay) cnt[px] = c | kRetired;
}

// The pooled error map: one pixel per thread, three floats.
template <class Counts>
__global__ void __launch_bounds__(kBlock)
film_pool_map_kernel(Counts cs, const double* __restrict__ u, const double* __restrict__ h,
                     const uint32_t* __restrict__ hn, size_t npix, uint32_t w, uint32_t rows,
                     int32_t band_rows, int32_t R, uint32_t flags, float* __restrict__ se) {
  const size_t px = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (px >= npix) return;
  const u64 B = cs.at(px).B;
  double g[3];
  uint32_t n;
  pool_gather(u, h, hn, npix, w, rows, band_rows, R, flags, px, B >= 2, g, &n);
  se[3 * px] = pool_se(g[0], n, B);
  se[3 * px + 1] = pool_se(g[1], n, B);
  se[3 * px + 2] = pool_se(g[2], n, B);
}

unsigned quad_blocks(size_t n) { return (unsigned)(((n + 3) / 4 + kBlock - 1) / kBlock); }
unsigned tail_blocks(size_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }
bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// A device plane of `bytes` bytes, zeroed on request. *p stays null when the allocation fails.
template <class T>
hipError_t plane_alloc(T** p, size_t bytes, bool zero) {
  hipError_t e = hipMalloc(p, bytes);
  if (e == hipSuccess && zero) e = hipMemset(*p, 0, bytes);
  return e;
}

// Free the planes of the film's layers named in `layers` (and forget them).
enum : unsigned { kSumsPlane = 1, kNoisePlanes = 2, kAdaptPlanes = 4, kPoolPlanes = 8, kAllPlanes = 15 };
void free_planes(spt_film* f, unsigned layers) {
  auto drop = [](auto*& p) {
    if (p) (void)hipFree(p);
    p = nullptr;
  };
  if (layers & kSumsPlane) drop(f->sums);
  if (layers & kNoisePlanes) drop(f->m2), drop(f->partials);
  if (layers & kAdaptPlanes) drop(f->cnt), drop(f->list), drop(f->scan), drop(f->table);
  if (layers & kPoolPlanes) drop(f->pool);
}

// The 16-byte kernel over the `body` whole quads it may take, the one-sum kernel over [body, n).
// quad(blocks) / tail(blocks) enqueue them.
template <class Quad, class Tail>
spt_status launch_quads_and_tail(size_t body, size_t n, Quad quad, Tail tail) {
  if (body) {
    quad(quad_blocks(body));
    SPT_HIP(hipGetLastError());
  }
  if (body < n) {
    tail(tail_blocks(n - body));
    SPT_HIP(hipGetLastError());
  }
  return SPT_OK;
}

// Count a pass of s_count samples over npix pixels into the film (spt_film_rollback is the inverse).
// c: the context that rendered it and may take it back; nullptr when nothing was launched.
void count_pass(spt_film* f, spt_context* c, uint32_t npix, int32_t s_count) {
  f->samples_done += s_count;
  if (f->batch) f->batches_done += 1;  // a pass of a noise film is one batch
  if (f->adaptive) {
    f->last_pass_samples = (int64_t)npix * s_count;
    f->samples_total += f->last_pass_samples;
  }
  if (!c) return;
  if (f->last_ctx && f->last_ctx != c) spt_context_forget_film(f->last_ctx, f);
  f->last_ctx = c;
}

// The adaptive film's count source. The public calls that only read a film take it const; bringing
// the counts plane up to date writes the film's cnt_front, so those calls cast here, once.
spt_film* counts_owner(const spt_film* f) { return const_cast<spt_film*>(f); }

// While nothing has retired the passes leave the counts plane alone (every count is the front):
// write it before anything reads it.
void sync_counts(spt_film* f, hipStream_t stream) {
  if (!f->adaptive || f->any_retired || f->n == 0 || f->cnt_front == f->batches_done) return;
  (void)hipMemsetD32Async((hipDeviceptr_t)f->cnt, (int)f->batches_done, f->n / 3, stream);
  f->cnt_front = f->batches_done;
}

PixelCount pixel_counts(spt_film* f, hipStream_t stream) {
  sync_counts(f, stream);
  return PixelCount{f->cnt, (const NoiseArgs*)f->table};
}

UniformCount uniform_count(const spt_film* f) {
  return UniformCount{noise_args(f->spp_total, f->samples_done, f->batch, f->batches_done)};
}

// film -> float with every pixel's own factor. stats: the words of the pass it follows, or null.
spt_status adaptive_resolve(spt_film* f, float* rgb_dev, const u64* stats, hipStream_t stream) {
  const PixelCount cs = pixel_counts(f, stream);
  hipLaunchKernelGGL(film_adapt_resolve_kernel, dim3(tail_blocks(f->n / 3)), dim3(kBlock), 0, stream,
                     (const u64*)f->sums, cs.cnt, cs.tab, rgb_dev, f->n / 3, stats);
  SPT_HIP(hipGetLastError());
  return SPT_OK;
}

template <class Counts>
spt_status noise_map_launch(const spt_film* f, const Counts& cs, float* se_dev, hipStream_t stream) {
  hipLaunchKernelGGL(film_noise_map_kernel<Counts>, dim3(tail_blocks(f->n)), dim3(kBlock), 0, stream,
                     (const u64*)f->sums, (const ulonglong2*)f->m2, se_dev, f->n, cs);
  SPT_HIP(hipGetLastError());
  return SPT_OK;
}

// The summary's two stages and the copy of the image's partial into *total (not waited for).
template <class Counts>
spt_status noise_summary_launch(const spt_film* f, const Counts& cs, NoisePartial* total,
                                hipStream_t stream) {
  double* parts = (double*)f->partials;
  NoisePartial* total_dev = (NoisePartial*)(parts + 5 * (size_t)f->n_partials);
  hipLaunchKernelGGL(film_noise_partials_kernel<Counts>, dim3(f->n_partials), dim3(kBlock), 0, stream,
                     (const u64*)f->sums, (const ulonglong2*)f->m2, f->n / 3, cs, parts);
  SPT_HIP(hipGetLastError());
  hipLaunchKernelGGL(film_noise_total_kernel, dim3(1), dim3(kBlock), 0, stream, (const double*)parts,
                     (uint32_t)f->n_partials, total_dev);
  SPT_HIP(hipGetLastError());
  SPT_HIP(hipMemcpyAsync(total, total_dev, sizeof *total, hipMemcpyDeviceToHost, stream));
  return SPT_OK;
}

// f->list = the active pixels ascending, f->n_active their number. Waits on the stream.
spt_status rebuild_list(spt_film* f, hipStream_t stream) {
  const size_t npix = f->n / 3;
  const unsigned nblk = tail_blocks(npix);
  hipLaunchKernelGGL(film_adapt_count_kernel, dim3(nblk), dim3(kBlock), 0, stream,
                     (const uint32_t*)f->cnt, npix, f->scan);
  SPT_HIP(hipGetLastError());
  hipLaunchKernelGGL(film_adapt_scan_kernel, dim3(1), dim3(kBlock), 0, stream, f->scan, (uint32_t)nblk);
  SPT_HIP(hipGetLastError());
  hipLaunchKernelGGL(film_adapt_scatter_kernel, dim3(nblk), dim3(kBlock), 0, stream,
                     (const uint32_t*)f->cnt, npix, (const uint32_t*)f->scan, f->list);
  SPT_HIP(hipGetLastError());
  uint32_t total = 0;
  SPT_HIP(hipMemcpyAsync(&total, f->scan + nblk, sizeof total, hipMemcpyDeviceToHost, stream));
  SPT_HIP(hipStreamSynchronize(stream));
  f->n_active = (int64_t)total;
  return SPT_OK;
}

// The pooled calls' arguments, and the scratch: allocated once, at the film's first pooled call.
spt_status pool_args(int32_t radius, uint32_t flags) {
  if (radius < 1 || radius > SPT_POOL_MAX_RADIUS)
    return fail(SPT_ERR_INVALID_ARG, "radius outside [1, SPT_POOL_MAX_RADIUS]");
  if (flags & ~SPT_POOL_EXCLUDE_CENTER) return fail(SPT_ERR_INVALID_ARG, "unknown pool flag bits");
  return SPT_OK;
}

spt_status pool_scratch(spt_film* f) {
  if (f->pool) return SPT_OK;
  const size_t npix = f->n / 3;
  const hipError_t e = plane_alloc(&f->pool, npix * (6 * sizeof(double) + sizeof(uint32_t)), false);
  if (e != hipSuccess) {
    free_planes(f, kPoolPlanes);
    return fail(SPT_ERR_OOM, std::string("pool scratch alloc: ") + hipGetErrorString(e));
  }
  return SPT_OK;
}

// A window never crosses a tile of a sharded film: its compact rows are image neighbours inside one.
int32_t pool_band_rows(const spt_film* f) { return f->shard_count > 1 ? f->tile_rows : 0; }

// Pass 1 of a pooled call: u, h and hn of every pixel into the scratch.
template <class Counts>
spt_status pool_rows_launch(const spt_film* f, const Counts& cs, int32_t R, hipStream_t stream) {
  const size_t npix = f->n / 3;
  const uint32_t w = (uint32_t)f->width, out_w = (uint32_t)kBlock - 2u * (uint32_t)R;
  const uint32_t tiles = (w + out_w - 1) / out_w;
  const uint64_t blocks = (uint64_t)f->rows * tiles;
  if (blocks > 0x7FFFFFFFull) return fail(SPT_ERR_INVALID_ARG, "film too large for a pooled pass");
  hipLaunchKernelGGL(film_pool_rows_kernel<Counts>, dim3((unsigned)blocks), dim3(kBlock), 0, stream,
                     (const u64*)f->sums, (const ulonglong2*)f->m2, cs, w, tiles, (uint32_t)R, npix,
                     f->pool, f->pool + 3 * npix, (uint32_t*)(f->pool + 6 * npix));
  SPT_HIP(hipGetLastError());
  return SPT_OK;
}

template <class Counts>
spt_status pool_map_launch(const spt_film* f, const Counts& cs, int32_t R, uint32_t flags, float* se_dev,
                           hipStream_t stream) {
  SPT_TRY(pool_rows_launch(f, cs, R, stream));
  const size_t npix = f->n / 3;
  hipLaunchKernelGGL(film_pool_map_kernel<Counts>, dim3(tail_blocks(npix)), dim3(kBlock), 0, stream, cs,
                     (const double*)f->pool, (const double*)(f->pool + 3 * npix),
                     (const uint32_t*)(f->pool + 6 * npix), npix, (uint32_t)f->width, (uint32_t)f->rows,
                     pool_band_rows(f), R, flags, se_dev);
  SPT_HIP(hipGetLastError());
  return SPT_OK;
}

// An adaptive film with every pixel active at count 0.
void adaptive_reset(spt_film* f) {
  f->any_retired = false;
  f->cnt_front = 0;
  f->n_active = (int64_t)(f->n / 3);
  f->samples_total = 0;
  f->last_pass_samples = 0;
}

}  // namespace

extern "C" spt_status spt_film_create(int32_t device, const spt_params* p, spt_film** out) {
  if (!p || !out) return fail(SPT_ERR_INVALID_ARG, "null argument");
  spt::WindowShape shape;
  SPT_TRY(spt::shape_from_params(p, 0xFFFFFFFFull, &shape));
  SPT_TRY(spt::open_device(device));
  spt_film* f = new spt_film();
  static_cast<spt::WindowShape&>(*f) = shape;
  f->device = device;
  f->n = 3ull * (size_t)f->rows * (size_t)f->width;
  if (f->n) {
    const hipError_t e = plane_alloc(&f->sums, f->n * sizeof(u64), true);
    if (e != hipSuccess) {
      free_planes(f, kAllPlanes);
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
  if (f->n) (void)hipSetDevice(f->device);
  free_planes(f, kAllPlanes);
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
    SPT_HIP(hipSetDevice(f->device));
    SPT_HIP(hipMemsetAsync(f->sums, 0, f->n * sizeof(u64), (hipStream_t)stream));
    if (f->m2) SPT_HIP(hipMemsetAsync(f->m2, 0, f->n * sizeof(ulonglong2), (hipStream_t)stream));
    if (f->cnt) SPT_HIP(hipMemsetAsync(f->cnt, 0, f->n / 3 * sizeof(uint32_t), (hipStream_t)stream));
  }
  if (f->adaptive) adaptive_reset(f);  // the list is rebuilt by the next select
  f->samples_done = 0;
  f->batches_done = 0;
  return SPT_OK;
}

spt_status spt_film_accumulate(spt_film* f, spt_context* c, const spt_film_launch& L, float* rgb_dev,
                               int32_t s_count, void* stream_v) {
  hipStream_t stream = (hipStream_t)stream_v;
  const dim3 grid((L.npix + kBlock - 1) / kBlock), block(kBlock);
  // once a pixel has retired the pass is over the active list; until then it is a noise film's
  const bool listed = f->adaptive && f->any_retired;
  if (listed) {
    if ((int64_t)L.npix != f->n_active)
      return fail(SPT_ERR_INVALID_ARG, "the launch is not over the film's active list");
    hipLaunchKernelGGL(film_accumulate_listed_kernel, grid, block, 0, stream, L.accum, L.slots, f->sums,
                       (ulonglong2*)f->m2, f->cnt, (const uint32_t*)f->list, L.npix, L.n_chunks,
                       L.scr_k, L.scr_q, L.stats);
  } else {
    if (f->n != 3ull * L.npix)
      return fail(SPT_ERR_INVALID_ARG, "the film does not have the launch's pixels");
    int full = 0;
    const float r = resolve_factor(f->spp_total, f->samples_done + s_count, &full);
    if (f->batch)  // a noise film: the same pass also squares its sums into the moment plane
      hipLaunchKernelGGL(film_accumulate_kernel<true>, grid, block, 0, stream, L.accum, L.slots, f->sums,
                         rgb_dev, L.npix, L.n_chunks, L.scr_k, L.scr_q, L.stats, r, full,
                         (int)aligned16(rgb_dev), (ulonglong2*)f->m2);
    else
      hipLaunchKernelGGL(film_accumulate_kernel<false>, grid, block, 0, stream, L.accum, L.slots,
                         f->sums, rgb_dev, L.npix, L.n_chunks, L.scr_k, L.scr_q, L.stats, r, full,
                         (int)aligned16(rgb_dev), (ulonglong2*)nullptr);
  }
  SPT_HIP(hipGetLastError());
  count_pass(f, c, L.npix, s_count);
  if (listed && rgb_dev) return adaptive_resolve(f, rgb_dev, L.stats, stream);
  return SPT_OK;
}

void spt_film_rollback(spt_film* f, const spt_context* c, int32_t s_count) {
  if (f->last_ctx == c && f->samples_done >= s_count) {  // count_pass, taken back
    f->samples_done -= s_count;
    if (f->batch && f->batches_done > 0) f->batches_done -= 1;
    if (f->adaptive) {  // the front goes back; the guarded pass incremented no count
      f->samples_total -= f->last_pass_samples;
      f->last_pass_samples = 0;
      if (!f->any_retired && f->cnt_front > f->batches_done) f->cnt_front = -1;
    }
  }
}

void spt_film_forget_context(spt_film* f, const spt_context* c) {
  if (f->last_ctx == c) f->last_ctx = nullptr;
}

extern "C" spt_status spt_film_render_async(spt_context* ctx, spt_film* f, const spt_prim* prims,
                                            int32_t n_prims, const spt_camera* cam,
                                            const spt_params* p, int32_t sample_base,
                                            int32_t sample_count, float* rgb_dev, void* stream) {
  if (!ctx || !f || !p) return fail(SPT_ERR_INVALID_ARG, "null context/film/params");
  SPT_TRY(spt::shape_accepts(*f, p, sample_base, sample_count, "film"));
  if (f->batch && (sample_count != f->batch || sample_base % f->batch != 0))
    return fail(SPT_ERR_INVALID_ARG, "a noise film takes whole batches: sample_count == batch, sample_base % batch == 0");
  if (f->adaptive) {
    if ((int64_t)sample_base != f->batches_done * f->batch)
      return fail(SPT_ERR_INVALID_ARG, "an adaptive film takes the next window only: sample_base == front * batch");
    if (f->n && f->n_active == 0)
      return fail(SPT_ERR_INVALID_ARG, "the adaptive film has no active pixel");
  }
  // once a pixel has retired the pass runs over the active list (spt_film_accumulate)
  const bool listed = f->adaptive && f->any_retired;
  SPT_TRY(spt_render_window(ctx, prims, n_prims, cam, p, sample_base, sample_count, rgb_dev, f, stream,
                            listed ? f->list : nullptr, listed ? (uint32_t)f->n_active : 0u));
  if (f->rows == 0) count_pass(f, nullptr, 0, sample_count);  // a shard without rows: still counted
  return SPT_OK;
}

extern "C" spt_status spt_film_resolve(const spt_film* f, float* rgb_dev, void* stream_v) {
  if (!f) return fail(SPT_ERR_INVALID_ARG, "null film");
  if (f->n == 0) return SPT_OK;
  if (!rgb_dev) return fail(SPT_ERR_INVALID_ARG, "null output");
  hipStream_t stream = (hipStream_t)stream_v;
  SPT_HIP(hipSetDevice(f->device));
  if (f->adaptive) return adaptive_resolve(counts_owner(f), rgb_dev, nullptr, stream);
  int full = 0;
  const float r = resolve_factor(f->spp_total, f->samples_done, &full);
  const u64* sums = f->sums;
  const size_t n = f->n, body = aligned16(rgb_dev) ? n & ~(size_t)3 : 0;  // sums the 16-byte kernel takes
  return launch_quads_and_tail(
      body, n,
      [&](unsigned blocks) {
        hipLaunchKernelGGL(film_resolve_kernel, dim3(blocks), dim3(kBlock), 0, stream, sums, rgb_dev,
                           body, r, full);
      },
      [&](unsigned blocks) {
        hipLaunchKernelGGL(film_resolve_tail_kernel, dim3(blocks), dim3(kBlock), 0, stream, sums,
                           rgb_dev, body, n, r, full);
      });
}

extern "C" spt_status spt_film_merge(spt_film* dst, const spt_film* src, void* stream_v) {
  if (!dst || !src || dst == src) return fail(SPT_ERR_INVALID_ARG, "merge needs two films");
  if (dst->width != src->width || dst->rows != src->rows || dst->spp_total != src->spp_total)
    return fail(SPT_ERR_INVALID_ARG, "films of unequal width/rows/spp");
  if (dst->device != src->device)
    return fail(SPT_ERR_INVALID_ARG, "films on different devices: download one and upload it beside the other");
  if (dst->samples_done + src->samples_done > dst->spp_total)
    return fail(SPT_ERR_INVALID_ARG, "the merged film would hold more than spp samples");
  if (dst->adaptive || src->adaptive)
    return fail(SPT_ERR_INVALID_ARG, "an adaptive film cannot be merged: its pixels hold different sample ranges");
  if (dst->batch != src->batch)
    return fail(SPT_ERR_INVALID_ARG, "merge needs two plain films or two noise films of equal batch");
  if (dst->n) {
    hipStream_t stream = (hipStream_t)stream_v;
    SPT_HIP(hipSetDevice(dst->device));
    u64* d = dst->sums;
    const u64* s = src->sums;
    const size_t n = dst->n, body = n & ~(size_t)3;
    SPT_TRY(launch_quads_and_tail(
        body, n,
        [&](unsigned blocks) {
          hipLaunchKernelGGL(film_merge_kernel, dim3(blocks), dim3(kBlock), 0, stream, d, s, body);
        },
        [&](unsigned blocks) {
          hipLaunchKernelGGL(film_merge_tail_kernel, dim3(blocks), dim3(kBlock), 0, stream, d, s, body, n);
        }));
    if (dst->batch) {
      hipLaunchKernelGGL(film_merge_m2_kernel, dim3(tail_blocks(n)), dim3(kBlock), 0, stream,
                         (ulonglong2*)dst->m2, (const ulonglong2*)src->m2, n);
      SPT_HIP(hipGetLastError());
    }
  }
  dst->batches_done += src->batches_done;
  dst->samples_done += src->samples_done;
  return SPT_OK;
}

extern "C" spt_status spt_film_download(const spt_film* f, uint64_t* host_sums, void* stream) {
  if (!f) return fail(SPT_ERR_INVALID_ARG, "null film");
  if (f->n == 0) return SPT_OK;
  if (!host_sums) return fail(SPT_ERR_INVALID_ARG, "null output");
  return copy_and_wait(f->device, host_sums, f->sums, f->n * sizeof(u64), hipMemcpyDeviceToHost, stream);
}

extern "C" spt_status spt_film_upload(spt_film* f, const uint64_t* host_sums, int64_t samples_done,
                                      void* stream) {
  if (!f) return fail(SPT_ERR_INVALID_ARG, "null film");
  if (samples_done < 0 || samples_done > f->spp_total)
    return fail(SPT_ERR_INVALID_ARG, "samples_done outside [0, spp]");
  if (f->batch && samples_done % f->batch != 0)
    return fail(SPT_ERR_INVALID_ARG, "a noise film holds whole batches: samples_done % batch != 0");
  if (f->n) {
    if (!host_sums) return fail(SPT_ERR_INVALID_ARG, "null input");
    SPT_TRY(copy_and_wait(f->device, f->sums, host_sums, f->n * sizeof(u64), hipMemcpyHostToDevice, stream));
  }
  f->samples_done = samples_done;
  return SPT_OK;
}

// ---- the noise film: moment plane, error map, image figures (include/spt.h SPT_HAS_FILM_NOISE) ----

extern "C" spt_status spt_film_noise_enable(spt_film* f, int32_t batch) {
  if (!f) return fail(SPT_ERR_INVALID_ARG, "null film");
  if (f->batch) return fail(SPT_ERR_INVALID_ARG, "the film is a noise film already");
  if (f->samples_done != 0) return fail(SPT_ERR_INVALID_ARG, "noise is enabled on an empty film only");
  if (batch < 1 || f->spp_total % batch != 0 || f->spp_total / batch < 2)
    return fail(SPT_ERR_INVALID_ARG, "batch must divide spp into at least two batches");
  if (f->n) {
    SPT_HIP(hipSetDevice(f->device));
    const unsigned blocks = tail_blocks(f->n / 3);
    hipError_t e = plane_alloc(&f->m2, f->n * sizeof(ulonglong2), true);
    if (e == hipSuccess)  // five planes of 8-byte words, then the total
      e = plane_alloc(&f->partials, 5 * (size_t)blocks * sizeof(double) + sizeof(NoisePartial), false);
    if (e != hipSuccess) {
      free_planes(f, kNoisePlanes);
      return fail(SPT_ERR_OOM, std::string("moment plane alloc: ") + hipGetErrorString(e));
    }
    f->n_partials = blocks;
  }
  f->batch = batch;
  f->batches_done = 0;
  return SPT_OK;
}

extern "C" spt_status spt_film_noise_info_get(const spt_film* f, spt_film_noise_info* out) {
  if (!f || !out) return fail(SPT_ERR_INVALID_ARG, "null argument");
  out->enabled = f->batch != 0;
  out->batch = f->batch;
  out->batches_done = f->batches_done;
  return SPT_OK;
}

extern "C" spt_status spt_film_noise_download(const spt_film* f, uint64_t* host_m2, void* stream) {
  if (!f) return fail(SPT_ERR_INVALID_ARG, "null film");
  if (!f->batch) return fail(SPT_ERR_INVALID_ARG, "not a noise film");
  if (f->n == 0) return SPT_OK;
  if (!host_m2) return fail(SPT_ERR_INVALID_ARG, "null output");
  return copy_and_wait(f->device, host_m2, f->m2, f->n * sizeof(ulonglong2), hipMemcpyDeviceToHost, stream);
}

extern "C" spt_status spt_film_noise_upload(spt_film* f, const uint64_t* host_m2, int64_t batches_done,
                                            void* stream) {
  if (!f) return fail(SPT_ERR_INVALID_ARG, "null film");
  if (!f->batch) return fail(SPT_ERR_INVALID_ARG, "not a noise film");
  if (batches_done < 0 || batches_done > f->spp_total / f->batch)
    return fail(SPT_ERR_INVALID_ARG, "batches_done outside [0, spp / batch]");
  if (f->n) {
    if (!host_m2) return fail(SPT_ERR_INVALID_ARG, "null input");
    SPT_TRY(copy_and_wait(f->device, f->m2, host_m2, f->n * sizeof(ulonglong2), hipMemcpyHostToDevice, stream));
  }
  f->batches_done = batches_done;
  return SPT_OK;
}

extern "C" spt_status spt_film_noise_map(const spt_film* f, float* se_dev, void* stream_v) {
  if (!f) return fail(SPT_ERR_INVALID_ARG, "null film");
  if (!f->batch) return fail(SPT_ERR_INVALID_ARG, "not a noise film");
  if (f->batches_done < 2) return fail(SPT_ERR_INVALID_ARG, "the error needs at least two batches");
  if (f->n == 0) return SPT_OK;
  if (!se_dev) return fail(SPT_ERR_INVALID_ARG, "null output");
  hipStream_t stream = (hipStream_t)stream_v;
  SPT_HIP(hipSetDevice(f->device));
  if (f->adaptive) return noise_map_launch(f, pixel_counts(counts_owner(f), stream), se_dev, stream);
  return noise_map_launch(f, uniform_count(f), se_dev, stream);
}

extern "C" spt_status spt_film_noise_summary(spt_film* f, spt_noise_summary* out, void* stream_v) {
  if (!f || !out) return fail(SPT_ERR_INVALID_ARG, "null argument");
  if (!f->batch) return fail(SPT_ERR_INVALID_ARG, "not a noise film");
  if (f->batches_done < 2) return fail(SPT_ERR_INVALID_ARG, "the error needs at least two batches");
  hipStream_t stream = (hipStream_t)stream_v;
  NoisePartial total{};
  if (f->n) {
    SPT_HIP(hipSetDevice(f->device));
    SPT_TRY(f->adaptive ? noise_summary_launch(f, pixel_counts(f, stream), &total, stream)
                        : noise_summary_launch(f, uniform_count(f), &total, stream));
  }
  SPT_HIP(hipStreamSynchronize(stream));
  noise_finish(total, f->n / 3, f->batches_done, out);
  return SPT_OK;
}

// ---- the adaptive film: counts plane, listed accumulate, selection (spt.h SPT_HAS_FILM_ADAPTIVE) ----

extern "C" spt_status spt_film_adaptive_enable(spt_film* f) {
  if (!f) return fail(SPT_ERR_INVALID_ARG, "null film");
  if (!f->batch) return fail(SPT_ERR_INVALID_ARG, "adaptive sampling needs a noise film");
  if (f->adaptive) return fail(SPT_ERR_INVALID_ARG, "the film is adaptive already");
  if (f->samples_done != 0 || f->batches_done != 0)
    return fail(SPT_ERR_INVALID_ARG, "adaptive sampling is enabled on an empty film only");
  const int32_t b_max = f->spp_total / f->batch;
  if (b_max > kAdaptMaxBatches)
    return fail(SPT_ERR_INVALID_ARG, "adaptive sampling takes at most 4096 batches: raise batch");
  std::vector<NoiseArgs> tab;
  try {
    tab = noise_table(f->spp_total, f->batch);
  } catch (const std::bad_alloc&) {
    return fail(SPT_ERR_OOM, "table alloc");
  }
  if (f->n) {
    const size_t npix = f->n / 3;
    const size_t tab_bytes = tab.size() * sizeof(NoiseArgs);
    hipError_t e = hipSetDevice(f->device);
    if (e == hipSuccess) e = plane_alloc(&f->cnt, npix * sizeof(uint32_t), true);
    if (e == hipSuccess) e = plane_alloc(&f->list, npix * sizeof(uint32_t), false);
    if (e == hipSuccess)
      e = plane_alloc(&f->scan, ((size_t)tail_blocks(npix) + 1) * sizeof(uint32_t), false);
    if (e == hipSuccess) e = plane_alloc(&f->table, tab_bytes, false);
    if (e == hipSuccess) e = hipMemcpy(f->table, tab.data(), tab_bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      free_planes(f, kAdaptPlanes);
      return fail(SPT_ERR_OOM, std::string("adaptive planes alloc: ") + hipGetErrorString(e));
    }
  }
  f->b_max = b_max;
  f->adaptive = true;
  adaptive_reset(f);
  return SPT_OK;
}

extern "C" spt_status spt_film_adaptive_info_get(const spt_film* f, spt_film_adaptive_info* out) {
  if (!f || !out) return fail(SPT_ERR_INVALID_ARG, "null argument");
  out->enabled = f->adaptive ? 1 : 0;
  out->reserved = 0;
  out->front = f->adaptive ? f->batches_done : 0;
  out->n_active = f->adaptive ? f->n_active : 0;
  out->samples_total = f->adaptive ? f->samples_total : 0;
  return SPT_OK;
}

extern "C" spt_status spt_film_adaptive_select(spt_film* f, double se_threshold,
                                               const uint8_t* keep_dev, int64_t* n_active,
                                               void* stream_v) {
  if (!f || !n_active) return fail(SPT_ERR_INVALID_ARG, "null argument");
  if (!f->adaptive) return fail(SPT_ERR_INVALID_ARG, "not an adaptive film");
  if (se_threshold != se_threshold) return fail(SPT_ERR_INVALID_ARG, "the threshold is NaN");
  if (f->batches_done < 2) return fail(SPT_ERR_INVALID_ARG, "the selection needs at least two batches");
  hipStream_t stream = (hipStream_t)stream_v;
  if (f->n == 0) {
    *n_active = 0;
    return SPT_OK;
  }
  SPT_HIP(hipSetDevice(f->device));
  sync_counts(f, stream);
  const size_t npix = f->n / 3;
  const int all = se_threshold < 0.0;
  const double thr2 = se_threshold * se_threshold;  // once, in double
  if (keep_dev || !all) {
    hipLaunchKernelGGL(film_adapt_mark_kernel, dim3(tail_blocks(npix)), dim3(kBlock), 0, stream,
                       (const u64*)f->sums, (const ulonglong2*)f->m2, f->cnt,
                       (const NoiseArgs*)f->table, keep_dev, npix, thr2, all);
    SPT_HIP(hipGetLastError());
  }
  SPT_TRY(rebuild_list(f, stream));
  if ((size_t)f->n_active != npix) f->any_retired = true;
  *n_active = f->n_active;
  return SPT_OK;
}

extern "C" spt_status spt_film_adaptive_download(const spt_film* f, uint32_t* host_counts,
                                                 void* stream) {
  if (!f) return fail(SPT_ERR_INVALID_ARG, "null film");
  if (!f->adaptive) return fail(SPT_ERR_INVALID_ARG, "not an adaptive film");
  if (f->n == 0) return SPT_OK;
  if (!host_counts) return fail(SPT_ERR_INVALID_ARG, "null output");
  SPT_HIP(hipSetDevice(f->device));
  sync_counts(counts_owner(f), (hipStream_t)stream);
  return copy_and_wait(f->device, host_counts, f->cnt, f->n / 3 * sizeof(uint32_t), hipMemcpyDeviceToHost,
                       stream);
}

extern "C" spt_status spt_film_adaptive_upload(spt_film* f, const uint32_t* host_counts,
                                               void* stream) {
  if (!f) return fail(SPT_ERR_INVALID_ARG, "null film");
  if (!f->adaptive) return fail(SPT_ERR_INVALID_ARG, "not an adaptive film");
  if (f->n == 0) return SPT_OK;
  if (!host_counts) return fail(SPT_ERR_INVALID_ARG, "null input");
  const size_t npix = f->n / 3;
  // the invariant: the active pixels share one count, the front; a retired one holds 2 .. front
  int64_t front = -1, top = 0, total = 0;
  size_t retired = 0;
  for (size_t p = 0; p < npix; ++p) {
    const int64_t B = host_counts[p] & kCntMask;
    if (B > f->b_max) return fail(SPT_ERR_INVALID_ARG, "a count above spp_total / batch");
    total += B;
    top = B > top ? B : top;
    if (host_counts[p] & kRetired) {
      ++retired;
    } else if (front < 0) {
      front = B;
    } else if (B != front) {
      return fail(SPT_ERR_INVALID_ARG, "the active pixels do not share one count");
    }
  }
  if (front < 0) front = top;
  if (top > front) return fail(SPT_ERR_INVALID_ARG, "a retired pixel holds more batches than the front");
  SPT_TRY(copy_and_wait(f->device, f->cnt, host_counts, npix * sizeof(uint32_t), hipMemcpyHostToDevice,
                             stream));
  f->batches_done = front;
  f->samples_done = front * (int64_t)f->batch;
  f->cnt_front = front;
  f->any_retired = retired != 0;
  f->n_active = (int64_t)(npix - retired);
  f->samples_total = total * (int64_t)f->batch;  // what the counts imply
  f->last_pass_samples = 0;
  if (f->any_retired) return rebuild_list(f, (hipStream_t)stream);
  return SPT_OK;
}

// ---- the pooled error: map and selection over a pixel's neighbourhood (spt.h SPT_HAS_FILM_POOL) ----

extern "C" spt_status spt_film_noise_pool_map(const spt_film* f, int32_t radius, uint32_t flags,
                                              float* se_dev, void* stream_v) {
  if (!f) return fail(SPT_ERR_INVALID_ARG, "null film");
  if (!f->batch) return fail(SPT_ERR_INVALID_ARG, "not a noise film");
  if (f->batches_done < 2) return fail(SPT_ERR_INVALID_ARG, "the error needs at least two batches");
  SPT_TRY(pool_args(radius, flags));
  if (f->n == 0) return SPT_OK;
  if (!se_dev) return fail(SPT_ERR_INVALID_ARG, "null output");
  hipStream_t stream = (hipStream_t)stream_v;
  SPT_HIP(hipSetDevice(f->device));
  SPT_TRY(pool_scratch(counts_owner(f)));
  if (f->adaptive)
    return pool_map_launch(f, pixel_counts(counts_owner(f), stream), radius, flags, se_dev, stream);
  return pool_map_launch(f, uniform_count(f), radius, flags, se_dev, stream);
}

extern "C" spt_status spt_film_adaptive_select_pooled(spt_film* f, double se_threshold, int32_t radius,
                                                      uint32_t flags, const uint8_t* keep_dev,
                                                      int64_t* n_active, void* stream_v) {
  if (!f || !n_active) return fail(SPT_ERR_INVALID_ARG, "null argument");
  if (!f->adaptive) return fail(SPT_ERR_INVALID_ARG, "not an adaptive film");
  if (se_threshold != se_threshold) return fail(SPT_ERR_INVALID_ARG, "the threshold is NaN");
  if (f->batches_done < 2) return fail(SPT_ERR_INVALID_ARG, "the selection needs at least two batches");
  SPT_TRY(pool_args(radius, flags));
  // without a threshold no error is looked at: the selection by the mask alone
  if (se_threshold < 0.0 || f->n == 0)
    return spt_film_adaptive_select(f, se_threshold, keep_dev, n_active, stream_v);
  hipStream_t stream = (hipStream_t)stream_v;
  SPT_HIP(hipSetDevice(f->device));
  SPT_TRY(pool_scratch(f));
  const PixelCount cs = pixel_counts(f, stream);
  SPT_TRY(pool_rows_launch(f, cs, radius, stream));
  const size_t npix = f->n / 3;
  const double thr2 = se_threshold * se_threshold;  // once, in double
  hipLaunchKernelGGL(film_pool_mark_kernel, dim3(tail_blocks(npix)), dim3(kBlock), 0, stream,
                     (const u64*)f->sums, (const ulonglong2*)f->m2, f->cnt, cs.tab, keep_dev,
                     (const double*)f->pool, (const double*)(f->pool + 3 * npix),
                     (const uint32_t*)(f->pool + 6 * npix), npix, (uint32_t)f->width, (uint32_t)f->rows,
                     pool_band_rows(f), radius, flags, thr2);
  SPT_HIP(hipGetLastError());
  SPT_TRY(rebuild_list(f, stream));
  if ((size_t)f->n_active != npix) f->any_retired = true;
  *n_active = f->n_active;
  return SPT_OK;
}

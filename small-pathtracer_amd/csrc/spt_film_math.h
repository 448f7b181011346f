// spt_film_math.h — the film's per-element arithmetic, stated once for the kernels (spt_film.hip)
// and for the CPU statements (spt_film_host.cpp, plain C++: it runs under the host sanitizers).
// Internal: the public statement is include/spt.h. Needs -ffp-contract=off on both sides.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/spt.h"

#if defined(__HIPCC__)  // every source of libspt.so is compiled as HIP; the check program is not
#include <hip/hip_runtime.h>
#define SPT_FILM_FN __host__ __device__ __forceinline__
using m2_t = ulonglong2;  // an element of the moment plane: (lo, hi), one 16-byte load
#else
#define SPT_FILM_FN inline
struct alignas(16) m2_t {
  unsigned long long x, y;
};
#endif

namespace spt_film_math {

using u64 = unsigned long long;

// An adaptive film's counts: low 31 bits the batches a pixel holds, bit 31 retired.
constexpr uint32_t kRetired = 0x80000000u, kCntMask = 0x7FFFFFFFu;
constexpr int32_t kAdaptMaxBatches = 4096;

SPT_FILM_FN float film_resolve1(u64 v, float r, int full) {
  float f = (float)v * 0x1p-31f;
  if (!full) f = f * r;
  return f > 1.0f ? 1.0f : f;
}

// The preview factor spp_total / samples_done, rounded once; *full = no factor at all.
SPT_FILM_FN float resolve_factor(int32_t spp_total, int64_t done, int* full) {
  *full = done == (int64_t)spp_total;
  return done > 0 ? (float)((double)spp_total / (double)done) : 0.0f;
}

// 64 x 64 -> high 64 bits.
SPT_FILM_FN u64 mulhi64(u64 a, u64 b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (u64)(((unsigned __int128)a * b) >> 64);
#endif
}

// m += p^2 in 128 bits, m = (lo, hi). Exact: p <= batch * 2^31 (the moment plane's bound, spt.h).
SPT_FILM_FN void m2_add_square(m2_t& m, u64 p) {
  const u64 lo = p * p, nl = m.x + lo;
  m.y += mulhi64(p, p) + (u64)(nl < lo);
  m.x = nl;
}

// Element e of a host moment plane (pairs (lo, hi) of uint64).
inline m2_t m2_at(const uint64_t* m2, size_t e) {
  m2_t m;
  m.x = m2[2 * e];
  m.y = m2[2 * e + 1];
  return m;
}

// What the resolve, the error map and the summary take for a pixel that holds B batches: the factor
// k of spt.h and its square (both rounded once, in double), the resolve's factor for the clamp rule.
struct NoiseArgs {
  u64 B;
  double k, k2;
  float r;
  int full;
};

// Computed once on the host in double; kernels and host statements read the same values.
// se = sqrt(d) * k. Fewer than two batches: k = k2 = 0, the standard error reads 0.
inline NoiseArgs noise_args(int32_t spp_total, int64_t samples_done, int32_t batch, int64_t B) {
  NoiseArgs A{};
  A.B = (u64)B;
  if (B >= 2) {
    A.k = (double)spp_total / ((double)batch * 0x1p31 * (double)B * std::sqrt((double)(B - 1)));
    A.k2 = A.k * A.k;
  }
  A.r = resolve_factor(spp_total, samples_done, &A.full);
  return A;
}

// An adaptive film's table: row B for a pixel that holds B batches, B = 0 .. spp_total / batch.
inline std::vector<NoiseArgs> noise_table(int32_t spp_total, int32_t batch) {
  std::vector<NoiseArgs> tab((size_t)(spp_total / batch) + 1);
  for (size_t B = 0; B < tab.size(); ++B)
    tab[B] = noise_args(spp_total, (int64_t)B * batch, batch, (int64_t)B);
  return tab;
}

// The count source: which NoiseArgs a pixel takes. Uniform: the film's one; per pixel: the table's
// row of the pixel's own count.
struct UniformCount {
  NoiseArgs A;
  SPT_FILM_FN const NoiseArgs& at(size_t) const { return A; }
};
struct PixelCount {
  const uint32_t* cnt;
  const NoiseArgs* tab;
  // B is the count itself (the row holds the same value), and B <= kAdaptMaxBatches: with that said
  // a kernel keeps B in one register and the row's byte offset in 32 bits.
  SPT_FILM_FN NoiseArgs row(uint32_t B) const {
    NoiseArgs A = tab[B & (2u * kAdaptMaxBatches - 1u)];
    A.B = B;
    return A;
  }
  SPT_FILM_FN NoiseArgs at(size_t px) const { return row(cnt[px] & kCntMask); }
};

// One element: D = B * M2 - S^2 in 128 bits as a double, or 0 with *clamped set where the resolved
// value is the clamp. The summary adds d * k2.
SPT_FILM_FN double noise_d(u64 S, m2_t m, const NoiseArgs& A, bool* clamped) {
  *clamped = film_resolve1(S, A.r, A.full) == 1.0f;
  if (*clamped) return 0.0;
  const u64 blo = A.B * m.x, bhi = A.B * m.y + mulhi64(A.B, m.x);
  const u64 slo = S * S, shi = mulhi64(S, S);
  const u64 lo = blo - slo, hi = bhi - shi - (u64)(blo < slo);
  return (double)hi * 0x1p64 + (double)lo;
}

// ... and its standard error.
SPT_FILM_FN float noise_se(double d, const NoiseArgs& A) { return (float)(sqrt(d) * A.k); }

// Is some channel of the pixel above the threshold? d * k2 > thr2, no square root: the same IEEE
// operations on the host and on the device (-ffp-contract=off).
SPT_FILM_FN bool adapt_noisy(const u64* S, const m2_t* m, const NoiseArgs& A, double thr2) {
  bool noisy = false;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int c = 0; c < 3; ++c) {
    bool cl;
    const double d = noise_d(S[c], m[c], A, &cl);
    noisy = noisy || d * A.k2 > thr2;
  }
  return noisy;
}

// ---- the pooled error (spt.h SPT_HAS_FILM_POOL) ----

// u: the estimated variance of a one-batch estimate of this element, in resolved units. 0 for a
// clamped channel (noise_d) and for a pixel with fewer than two batches. Never negative and never
// -0.0 (d >= +0), so a window sum may take 0.0 for a place outside the film: x + 0.0 is x.
SPT_FILM_FN double pool_u(u64 S, m2_t m, const NoiseArgs& A) {
  if (A.B < 2) return 0.0;
  bool cl;
  return (noise_d(S, m, A, &cl) * A.k2) * (double)A.B;
}

// The rows of pixel row y's window: y - R .. y + R clipped to the film and to the row's band (written
// so that nothing overflows 32 bits).
SPT_FILM_FN void pool_row_window(int32_t y, int32_t rows, int32_t band_rows, int32_t R, int32_t* y0,
                                 int32_t* y1) {
  int32_t b0 = 0, b1 = rows;
  if (band_rows > 0) {
    b0 = y - y % band_rows;
    b1 = rows - b0 > band_rows ? b0 + band_rows : rows;
  }
  *y0 = y - b0 > R ? y - R : b0;
  *y1 = b1 - 1 - y > R ? y + R : b1 - 1;
}

// The centre taken out of its own window: one subtraction per channel; counted = B_p >= 2.
SPT_FILM_FN void pool_exclude_center(double g[3], uint32_t* n, const double u[3], bool counted) {
  g[0] = g[0] - u[0];
  g[1] = g[1] - u[1];
  g[2] = g[2] - u[2];
  if (counted) *n -= 1u;
}

// Is some channel's pooled error above the threshold? g / (n B) > thr2 without the division. n >= 1.
SPT_FILM_FN bool pool_noisy(const double g[3], uint32_t n, u64 B, double thr2) {
  const double t = (thr2 * (double)n) * (double)B;
  return g[0] > t || g[1] > t || g[2] > t;
}

SPT_FILM_FN float pool_se(double g, uint32_t n, u64 B) {
  if (n == 0 || B < 2) return 0.0f;
  return (float)sqrt(g / ((double)n * (double)B));
}

// The summary's partial sums: of a block (stage 1), of the image (stage 2).
struct NoisePartial {
  double s[3];  // per channel: sum of d * k2
  float se_max;
  uint32_t pad;
  u64 clamped;
};

inline void noise_finish(const NoisePartial& t, size_t npix, int64_t B, spt_noise_summary* out) {
  const double n = npix ? (double)npix : 1.0;
  for (int c = 0; c < 3; ++c) out->rmse[c] = std::sqrt(t.s[c] / n);
  out->rmse_all = std::sqrt((t.s[0] + t.s[1] + t.s[2]) / (3.0 * n));
  out->se_max = t.se_max;
  out->clamped = t.clamped;
  out->batches_done = B;
}

}  // namespace spt_film_math

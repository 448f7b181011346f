// spt_film_host.cpp — the film's CPU statements (include/spt.h: spt_film_*_host). What the tests
// treat as the definition of the film: the arithmetic of spt_film_math.h, element by element, in plain
// C++ with no HIP in it, so that tests/probe/spt_film_check.cpp runs it under the host sanitizers.
#include <new>
#include <string>
#include <vector>

#include "spt_film_math.h"
#include "spt_status.h"

using namespace spt_film_math;
using spt::fail;

namespace {

// Which film a statement speaks of: a plain one (no noise info), a noise film, or an adaptive film
// (per-pixel counts; its samples_done is implied by the counts and not looked at).
enum FilmKind { kPlain, kNoise, kAdaptive };

// The one validator of (info, noise[, counts]): *n = the film's elements and, for an adaptive film,
// *tab = the table for noise->batch. No count indexes the table before all of them are checked.
spt_status host_args(FilmKind kind, const spt_film_info* info, const spt_film_noise_info* noise,
                     const uint32_t* counts, size_t* n, std::vector<NoiseArgs>* tab) {
  if (!info || (kind != kPlain && !noise)) return fail(SPT_ERR_INVALID_ARG, "null info");
  if (info->width <= 0 || info->rows < 0 || info->spp_total <= 0 ||
      (kind != kAdaptive && (info->samples_done < 0 || info->samples_done > info->spp_total)))
    return fail(SPT_ERR_INVALID_ARG, "bad film info");
  if (kind == kNoise) {
    if (!noise->enabled || noise->batch < 1) return fail(SPT_ERR_INVALID_ARG, "not a noise film");
    if (noise->batches_done < 2)
      return fail(SPT_ERR_INVALID_ARG, "the error needs at least two batches");
  }
  if (kind == kAdaptive &&
      (!noise->enabled || noise->batch < 1 || info->spp_total % noise->batch != 0 ||
       info->spp_total / noise->batch > kAdaptMaxBatches))
    return fail(SPT_ERR_INVALID_ARG, "not an adaptive film's batch");
  *n = 3ull * (size_t)info->rows * (size_t)info->width;
  if (kind != kAdaptive) return SPT_OK;
  if (*n && !counts) return fail(SPT_ERR_INVALID_ARG, "null counts");
  const uint32_t b_max = (uint32_t)(info->spp_total / noise->batch);
  for (size_t p = 0; p < *n / 3; ++p)
    if ((counts[p] & kCntMask) > b_max)
      return fail(SPT_ERR_INVALID_ARG, "a count above spp_total / batch");
  try {
    *tab = noise_table(info->spp_total, noise->batch);
  } catch (const std::bad_alloc&) {
    return fail(SPT_ERR_OOM, "table alloc");
  }
  return SPT_OK;
}

// The three per-element loops, each for either count source.
template <class Counts>
void resolve_loop(const uint64_t* sums, size_t n, const Counts& cs, float* rgb_out) {
  for (size_t e = 0; e < n; ++e) {
    const NoiseArgs& A = cs.at(e / 3);
    rgb_out[e] = film_resolve1((u64)sums[e], A.r, A.full);
  }
}

template <class Counts>
void map_loop(const uint64_t* sums, const uint64_t* m2, size_t n, const Counts& cs, float* se_out) {
  for (size_t e = 0; e < n; ++e) {
    const NoiseArgs& A = cs.at(e / 3);
    bool c;
    se_out[e] = noise_se(noise_d((u64)sums[e], m2_at(m2, e), A, &c), A);
  }
}

template <class Counts>
void summary_loop(const uint64_t* sums, const uint64_t* m2, size_t n, const Counts& cs,
                  int64_t batches_done, spt_noise_summary* out) {
  NoisePartial t{};
  for (size_t e = 0; e < n; ++e) {
    const NoiseArgs& A = cs.at(e / 3);
    bool c;
    const double d = noise_d((u64)sums[e], m2_at(m2, e), A, &c);
    t.s[e % 3] += d * A.k2;
    t.se_max = std::fmax(t.se_max, noise_se(d, A));
    t.clamped += c ? 1u : 0u;
  }
  noise_finish(t, n / 3, batches_done, out);
}

UniformCount uniform(const spt_film_info* info, const spt_film_noise_info* noise) {
  return UniformCount{noise_args(info->spp_total, info->samples_done, noise->batch, noise->batches_done)};
}

bool has_pixels(const spt_film_info* info) { return info && info->rows > 0 && info->width > 0; }

}  // namespace

extern "C" spt_status spt_film_resolve_host(const uint64_t* sums, const spt_film_info* info,
                                            float* rgb_out) {
  size_t n = 0;
  SPT_TRY(host_args(kPlain, info, nullptr, nullptr, &n, nullptr));
  if (n == 0) return SPT_OK;
  if (!sums || !rgb_out) return fail(SPT_ERR_INVALID_ARG, "null sums/output");
  UniformCount cs{};
  cs.A.r = resolve_factor(info->spp_total, info->samples_done, &cs.A.full);
  resolve_loop(sums, n, cs, rgb_out);
  return SPT_OK;
}

extern "C" spt_status spt_film_noise_map_host(const uint64_t* sums, const uint64_t* m2,
                                              const spt_film_info* info,
                                              const spt_film_noise_info* noise, float* se_out) {
  size_t n = 0;
  SPT_TRY(host_args(kNoise, info, noise, nullptr, &n, nullptr));
  if (n == 0) return SPT_OK;
  if (!sums || !m2 || !se_out) return fail(SPT_ERR_INVALID_ARG, "null sums/moments/output");
  map_loop(sums, m2, n, uniform(info, noise), se_out);
  return SPT_OK;
}

extern "C" spt_status spt_film_noise_summary_host(const uint64_t* sums, const uint64_t* m2,
                                                  const spt_film_info* info,
                                                  const spt_film_noise_info* noise,
                                                  spt_noise_summary* out) {
  size_t n = 0;
  SPT_TRY(host_args(kNoise, info, noise, nullptr, &n, nullptr));
  if (!out || (n && (!sums || !m2))) return fail(SPT_ERR_INVALID_ARG, "null sums/moments/output");
  summary_loop(sums, m2, n, uniform(info, noise), noise->batches_done, out);
  return SPT_OK;
}

extern "C" spt_status spt_film_adaptive_resolve_host(const uint64_t* sums, const uint32_t* counts,
                                                     const spt_film_info* info,
                                                     const spt_film_noise_info* noise, float* rgb_out) {
  size_t n = 0;
  std::vector<NoiseArgs> tab;
  if (has_pixels(info) && (!sums || !rgb_out)) return fail(SPT_ERR_INVALID_ARG, "null sums/output");
  SPT_TRY(host_args(kAdaptive, info, noise, counts, &n, &tab));
  resolve_loop(sums, n, PixelCount{counts, tab.data()}, rgb_out);
  return SPT_OK;
}

extern "C" spt_status spt_film_adaptive_noise_map_host(const uint64_t* sums, const uint64_t* m2,
                                                       const uint32_t* counts,
                                                       const spt_film_info* info,
                                                       const spt_film_noise_info* noise,
                                                       float* se_out) {
  size_t n = 0;
  std::vector<NoiseArgs> tab;
  if (has_pixels(info) && (!sums || !m2 || !se_out))
    return fail(SPT_ERR_INVALID_ARG, "null sums/moments/output");
  SPT_TRY(host_args(kAdaptive, info, noise, counts, &n, &tab));
  map_loop(sums, m2, n, PixelCount{counts, tab.data()}, se_out);
  return SPT_OK;
}

extern "C" spt_status spt_film_adaptive_noise_summary_host(const uint64_t* sums, const uint64_t* m2,
                                                           const uint32_t* counts,
                                                           const spt_film_info* info,
                                                           const spt_film_noise_info* noise,
                                                           spt_noise_summary* out) {
  size_t n = 0;
  std::vector<NoiseArgs> tab;
  if (!out || (has_pixels(info) && (!sums || !m2)))
    return fail(SPT_ERR_INVALID_ARG, "null sums/moments/output");
  SPT_TRY(host_args(kAdaptive, info, noise, counts, &n, &tab));
  summary_loop(sums, m2, n, PixelCount{counts, tab.data()}, noise->batches_done, out);
  return SPT_OK;
}

extern "C" spt_status spt_film_adaptive_select_host(const uint64_t* sums, const uint64_t* m2,
                                                    const uint32_t* counts, const spt_film_info* info,
                                                    const spt_film_noise_info* noise,
                                                    double se_threshold, const uint8_t* keep,
                                                    uint32_t* counts_out, uint32_t* list_out,
                                                    int64_t* n_active) {
  size_t n = 0;
  std::vector<NoiseArgs> tab;
  if (!n_active) return fail(SPT_ERR_INVALID_ARG, "null n_active");
  if (se_threshold != se_threshold) return fail(SPT_ERR_INVALID_ARG, "the threshold is NaN");
  if (noise && noise->batches_done < 2)
    return fail(SPT_ERR_INVALID_ARG, "the selection needs at least two batches");
  if (has_pixels(info) && (!sums || !m2 || !counts_out || !list_out))
    return fail(SPT_ERR_INVALID_ARG, "null sums/moments/output");
  SPT_TRY(host_args(kAdaptive, info, noise, counts, &n, &tab));
  const bool all = se_threshold < 0.0;
  const double thr2 = se_threshold * se_threshold;  // once, in double
  int64_t na = 0;
  for (size_t px = 0; px < n / 3; ++px) {
    uint32_t c = counts[px];
    if (!(c & kRetired)) {
      bool stay = keep ? keep[px] != 0 : true;
      if (stay && !all) {
        const m2_t m[3] = {m2_at(m2, 3 * px), m2_at(m2, 3 * px + 1), m2_at(m2, 3 * px + 2)};
        const u64 S[3] = {(u64)sums[3 * px], (u64)sums[3 * px + 1], (u64)sums[3 * px + 2]};
        stay = adapt_noisy(S, m, tab[c], thr2);
      }
      if (stay)
        list_out[na++] = (uint32_t)px;
      else
        c |= kRetired;
    }
    counts_out[px] = c;
  }
  *n_active = na;
  return SPT_OK;
}

// ---- the pooled error (spt.h SPT_HAS_FILM_POOL): u, its row sums h, the window sums g and n ----

namespace {

spt_status pool_args(int32_t band_rows, int32_t radius, uint32_t flags) {
  if (radius < 1 || radius > SPT_POOL_MAX_RADIUS)
    return fail(SPT_ERR_INVALID_ARG, "radius outside [1, SPT_POOL_MAX_RADIUS]");
  if (flags & ~SPT_POOL_EXCLUDE_CENTER) return fail(SPT_ERR_INVALID_ARG, "unknown pool flag bits");
  if (band_rows < 0) return fail(SPT_ERR_INVALID_ARG, "band_rows < 0");
  return SPT_OK;
}

// The planes every pooled statement starts from: u per element, counted per pixel (B >= 2), and the
// row sums over the columns of the window, ascending.
struct PoolPlanes {
  std::vector<double> u, h;
  std::vector<uint32_t> counted, hn;
};

template <class Counts>
void pool_planes(const uint64_t* sums, const uint64_t* m2, int64_t w, int64_t rows, const Counts& cs,
                 int32_t R, PoolPlanes* P) {
  const size_t npix = (size_t)(w * rows);
  P->u.assign(3 * npix, 0.0);
  P->h.assign(3 * npix, 0.0);
  P->counted.assign(npix, 0u);
  P->hn.assign(npix, 0u);
  for (size_t px = 0; px < npix; ++px) {
    const NoiseArgs& A = cs.at(px);
    P->counted[px] = A.B >= 2 ? 1u : 0u;
    for (size_t c = 0; c < 3; ++c)
      P->u[3 * px + c] = pool_u((u64)sums[3 * px + c], m2_at(m2, 3 * px + c), A);
  }
  for (int64_t y = 0; y < rows; ++y)
    for (int64_t x = 0; x < w; ++x) {
      const int64_t x0 = x - R > 0 ? x - R : 0, x1 = x + R < w - 1 ? x + R : w - 1;
      double h[3] = {0.0, 0.0, 0.0};
      uint32_t n = 0;
      for (int64_t xx = x0; xx <= x1; ++xx) {
        const size_t q = (size_t)(y * w + xx);
        for (int c = 0; c < 3; ++c) h[c] = h[c] + P->u[3 * q + c];
        n += P->counted[q];
      }
      const size_t px = (size_t)(y * w + x);
      for (int c = 0; c < 3; ++c) P->h[3 * px + c] = h[c];
      P->hn[px] = n;
    }
}

// g and n of pixel (y, x): the row sums over the window's rows, ascending; the centre out on request.
void pool_window(const PoolPlanes& P, int64_t w, int64_t rows, int32_t band_rows, int32_t R,
                 uint32_t flags, int64_t y, int64_t x, double g[3], uint32_t* n) {
  int32_t y0, y1;
  pool_row_window((int32_t)y, (int32_t)rows, band_rows, R, &y0, &y1);
  g[0] = g[1] = g[2] = 0.0;
  *n = 0;
  for (int64_t yy = y0; yy <= y1; ++yy) {
    const size_t q = (size_t)(yy * w + x);
    for (int c = 0; c < 3; ++c) g[c] = g[c] + P.h[3 * q + c];
    *n += P.hn[q];
  }
  const size_t px = (size_t)(y * w + x);
  if (flags & SPT_POOL_EXCLUDE_CENTER) pool_exclude_center(g, n, &P.u[3 * px], P.counted[px] != 0);
}

template <class Counts>
spt_status pool_map_loop(const uint64_t* sums, const uint64_t* m2, const spt_film_info* info,
                         const Counts& cs, int32_t band_rows, int32_t R, uint32_t flags,
                         float* se_out) {
  PoolPlanes P;
  try {
    pool_planes(sums, m2, info->width, info->rows, cs, R, &P);
  } catch (const std::bad_alloc&) {
    return fail(SPT_ERR_OOM, "pool planes alloc");
  }
  for (int64_t y = 0; y < info->rows; ++y)
    for (int64_t x = 0; x < info->width; ++x) {
      double g[3];
      uint32_t n;
      pool_window(P, info->width, info->rows, band_rows, R, flags, y, x, g, &n);
      const size_t px = (size_t)(y * info->width + x);
      const u64 B = cs.at(px).B;
      for (int c = 0; c < 3; ++c) se_out[3 * px + c] = pool_se(g[c], n, B);
    }
  return SPT_OK;
}

}  // namespace

extern "C" spt_status spt_film_noise_pool_map_host(const uint64_t* sums, const uint64_t* m2,
                                                   const uint32_t* counts,
                                                   const spt_film_info* info,
                                                   const spt_film_noise_info* noise,
                                                   int32_t band_rows, int32_t radius, uint32_t flags,
                                                   float* se_out) {
  size_t n = 0;
  std::vector<NoiseArgs> tab;
  SPT_TRY(pool_args(band_rows, radius, flags));
  if (has_pixels(info) && (!sums || !m2 || !se_out))
    return fail(SPT_ERR_INVALID_ARG, "null sums/moments/output");
  SPT_TRY(counts ? host_args(kAdaptive, info, noise, counts, &n, &tab)
                 : host_args(kNoise, info, noise, nullptr, &n, nullptr));
  if (n == 0) return SPT_OK;
  if (counts)
    return pool_map_loop(sums, m2, info, PixelCount{counts, tab.data()}, band_rows, radius, flags,
                         se_out);
  return pool_map_loop(sums, m2, info, uniform(info, noise), band_rows, radius, flags, se_out);
}

extern "C" spt_status spt_film_adaptive_select_pooled_host(
    const uint64_t* sums, const uint64_t* m2, const uint32_t* counts, const spt_film_info* info,
    const spt_film_noise_info* noise, int32_t band_rows, double se_threshold, int32_t radius,
    uint32_t flags, const uint8_t* keep, uint32_t* counts_out, uint32_t* list_out,
    int64_t* n_active) {
  size_t n = 0;
  std::vector<NoiseArgs> tab;
  if (!n_active) return fail(SPT_ERR_INVALID_ARG, "null n_active");
  SPT_TRY(pool_args(band_rows, radius, flags));
  if (se_threshold != se_threshold) return fail(SPT_ERR_INVALID_ARG, "the threshold is NaN");
  if (noise && noise->batches_done < 2)
    return fail(SPT_ERR_INVALID_ARG, "the selection needs at least two batches");
  if (has_pixels(info) && (!sums || !m2 || !counts_out || !list_out))
    return fail(SPT_ERR_INVALID_ARG, "null sums/moments/output");
  SPT_TRY(host_args(kAdaptive, info, noise, counts, &n, &tab));
  const bool all = se_threshold < 0.0;
  const double thr2 = se_threshold * se_threshold;  // once, in double
  PoolPlanes P;
  if (n && !all) {  // every decision below reads these planes, made before anything is marked
    try {
      pool_planes(sums, m2, info->width, info->rows, PixelCount{counts, tab.data()}, radius, &P);
    } catch (const std::bad_alloc&) {
      return fail(SPT_ERR_OOM, "pool planes alloc");
    }
  }
  int64_t na = 0;
  for (size_t px = 0; px < n / 3; ++px) {
    uint32_t c = counts[px];
    if (!(c & kRetired)) {
      bool stay = keep ? keep[px] != 0 : true;
      if (stay && !all) {
        double g[3];
        uint32_t cnt_n;
        pool_window(P, info->width, info->rows, band_rows, radius, flags,
                    (int64_t)(px / (size_t)info->width), (int64_t)(px % (size_t)info->width), g, &cnt_n);
        if (cnt_n) {
          stay = pool_noisy(g, cnt_n, (u64)c, thr2);
        } else {  // nothing to pool: the pixel's own rule
          const m2_t m[3] = {m2_at(m2, 3 * px), m2_at(m2, 3 * px + 1), m2_at(m2, 3 * px + 2)};
          const u64 S[3] = {(u64)sums[3 * px], (u64)sums[3 * px + 1], (u64)sums[3 * px + 2]};
          stay = adapt_noisy(S, m, tab[c], thr2);
        }
      }
      if (stay)
        list_out[na++] = (uint32_t)px;
      else
        c |= kRetired;
    }
    counts_out[px] = c;
  }
  *n_active = na;
  return SPT_OK;
}

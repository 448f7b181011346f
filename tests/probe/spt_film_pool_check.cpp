// spt_film_pool_check.cpp — TEST INFRASTRUCTURE ONLY: a stand-alone host program over the pooled
// error's CPU statements (spt_film_noise_pool_map_host, spt_film_adaptive_select_pooled_host in
// spt_film_host.cpp, with spt_dispatch.cpp for spt_last_error), built with
// -fsanitize=address,undefined by tests/probe/pool_check.mk and run by tests/test_film_pool_host.py.
// No HIP, no device, never loaded into Python. Every buffer is a std::vector of exactly the size the
// statement may touch, so a window that leaves the film is a sanitizer report.
//   * border windows: every pixel of 5x3 and 9x7 films at R = 1 and 2;
//   * R larger than the film: R = 16 on 5x3, where every window is the film and one n holds for all;
//   * bands with a short last band: 9x7 with band_rows = 3 (3, 3, 1 rows), band_rows = 1, and
//     band_rows above the rows; a window never sees a pixel across a band's edge;
//   * the 1x1 film: with the centre excluded n == 0, the map reads 0 and the own rule decides;
//   * a count of 1 (uploaded) is not counted; rows = 0; the refused arguments.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/spt.h"

static int g_failed = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                            \
    }                                                                        \
  } while (0)

using u64 = uint64_t;
typedef unsigned __int128 u128;
constexpr uint32_t kRetired = 0x80000000u;
constexpr int32_t kBatch = 3, kBMax = 6, kSpp = kBatch * kBMax;
constexpr u64 kTop = (u64)kBatch << 31;  // the bound of one batch sum

struct HostFilm {
  int32_t w, rows;
  std::vector<u64> sums, m2;
  std::vector<uint32_t> counts;
  size_t npix() const { return (size_t)w * (size_t)rows; }
  // Pixel p holds B(p) batches of dim, spread sums from a small generator; the active pixels (no bit
  // 31) share the front kBMax.
  HostFilm(int32_t w_, int32_t rows_, uint32_t seed) : w(w_), rows(rows_) {
    sums.resize(3 * npix());
    m2.resize(6 * npix());
    counts.resize(npix());
    uint32_t s = seed;
    auto next = [&s]() { return s = s * 1664525u + 1013904223u; };
    for (size_t p = 0; p < npix(); ++p) {
      const uint32_t B = (next() >> 16) % 3 == 0 ? 2 + (next() >> 16) % (kBMax - 1) : kBMax;
      counts[p] = B < (uint32_t)kBMax || (next() >> 16) % 5 == 0 ? B | kRetired : B;
      for (size_t c = 0; c < 3; ++c) {
        u64 S = 0;
        u128 M = 0;
        for (uint32_t b = 0; b < B; ++b) {
          const u64 v = (u64)(next() >> 8) * (kTop / 200) >> 24;
          S += v;
          M += (u128)v * v;
        }
        sums[3 * p + c] = S;
        m2[2 * (3 * p + c)] = (u64)M;
        m2[2 * (3 * p + c) + 1] = (u64)(M >> 64);
      }
    }
  }
  spt_film_info info() const { return spt_film_info{w, rows, kSpp, (int64_t)kSpp}; }
};

static spt_film_noise_info noise() { return spt_film_noise_info{1, kBatch, kBMax}; }

// The checks below are about structure (which pixels a window may see, what a selection must keep);
// the arithmetic is compared with Python floats in tests/test_film_pool.py.
static std::vector<float> pool_map(const HostFilm& f, int32_t band, int32_t R, uint32_t flags) {
  std::vector<float> se(3 * f.npix(), -1.0f);
  const spt_film_info i = f.info();
  const spt_film_noise_info n = noise();
  CHECK(spt_film_noise_pool_map_host(f.sums.data(), f.m2.data(), f.counts.data(), &i, &n, band, R, flags,
                                     se.data()) == SPT_OK);
  return se;
}

struct Selection {
  std::vector<uint32_t> counts, list;
  int64_t n = -1;
};

static Selection pool_select(const HostFilm& f, int32_t band, double thr, int32_t R, uint32_t flags,
                             const std::vector<uint8_t>* keep = nullptr) {
  Selection s;
  s.counts.assign(f.npix(), 0xFFFFFFFFu);
  s.list.resize(f.npix());
  const spt_film_info i = f.info();
  const spt_film_noise_info n = noise();
  CHECK(spt_film_adaptive_select_pooled_host(f.sums.data(), f.m2.data(), f.counts.data(), &i, &n, band,
                                             thr, R, flags, keep ? keep->data() : nullptr,
                                             s.counts.data(), s.list.data(), &s.n) == SPT_OK);
  CHECK(s.n >= 0 && (size_t)s.n <= f.npix());
  s.list.resize(s.n < 0 ? 0 : (size_t)s.n);
  return s;
}

// What a selection must keep whatever the threshold: counts' low bits, the retired, an ascending list
// of exactly the pixels without bit 31.
static void check_selection(const HostFilm& f, const Selection& s) {
  size_t k = 0;
  for (size_t p = 0; p < f.npix(); ++p) {
    CHECK((s.counts[p] & ~kRetired) == (f.counts[p] & ~kRetired));
    CHECK((s.counts[p] & kRetired) >= (f.counts[p] & kRetired));
    if (!(s.counts[p] & kRetired)) {
      CHECK(k < s.list.size() && s.list[k] == p);
      ++k;
    }
  }
  CHECK(k == s.list.size());
}

// Changing pixel q's samples changes the pooled error of p if and only if q lies in p's window.
static void check_reach(int32_t w, int32_t rows, int32_t band, int32_t R, uint32_t flags, uint32_t seed) {
  const HostFilm f(w, rows, seed);
  const std::vector<float> base = pool_map(f, band, R, flags);
  for (size_t q = 0; q < f.npix(); ++q) {
    HostFilm g = f;
    // one more spread-out element: channel 0 of q becomes two unequal batches at count 2
    g.counts[q] = 2u | kRetired;
    const u64 a = kTop / 300, b = kTop / 900;
    g.sums[3 * q] = a + b;
    const u128 M = (u128)a * a + (u128)b * b;
    g.m2[6 * q] = (u64)M;
    g.m2[6 * q + 1] = (u64)(M >> 64);
    const std::vector<float> se = pool_map(g, band, R, flags);
    const int32_t qy = (int32_t)(q / (size_t)w), qx = (int32_t)(q % (size_t)w);
    for (size_t p = 0; p < f.npix(); ++p) {
      const int32_t py = (int32_t)(p / (size_t)w), px = (int32_t)(p % (size_t)w);
      bool inside = std::abs(px - qx) <= R && std::abs(py - qy) <= R;
      if (band > 0) inside = inside && py / band == qy / band;
      if (p == q) continue;  // its own count changed: its figure is another pixel's
      if (!inside)
        CHECK(std::memcmp(&se[3 * p], &base[3 * p], 3 * sizeof(float)) == 0);
      else  // ... and does change it there: the window reaches its every corner
        CHECK(se[3 * p] != base[3 * p]);
    }
  }
}

int main() {
  // border windows, R above the film, bands with a short last band
  for (uint32_t flags = 0; flags <= SPT_POOL_EXCLUDE_CENTER; ++flags) {
    for (int32_t R : {1, 2, 16}) {
      check_reach(5, 3, 0, R, flags, 11u);
      for (int32_t band : {0, 1, 3, 8}) check_reach(9, 7, band, R, flags, 12u);
    }
  }
  {  // R = 16 on 5x3: one window, so one n; every counted pixel at the front reads one value per channel
    HostFilm f(5, 3, 21u);
    for (size_t p = 0; p < f.npix(); ++p) f.counts[p] = kBMax;
    const std::vector<float> se = pool_map(f, 0, 16, 0);
    for (size_t p = 1; p < f.npix(); ++p) CHECK(std::memcmp(&se[3 * p], &se[0], 3 * sizeof(float)) == 0);
    CHECK(se[0] > 0.0f && se[1] > 0.0f && se[2] > 0.0f);
    // a threshold above it retires all, one below none
    Selection s = pool_select(f, 0, 2.0 * std::fmax(se[0], std::fmax(se[1], se[2])), 16, 0);
    CHECK(s.n == 0);
    check_selection(f, s);
    s = pool_select(f, 0, 0.5 * std::fmax(se[0], std::fmax(se[1], se[2])), 16, 0);
    CHECK(s.n == (int64_t)f.npix());
    check_selection(f, s);
    f.counts[7] = 1u | kRetired;  // an uploaded count of 1: not counted, and its own figure is 0
    const std::vector<float> se1 = pool_map(f, 0, 16, 0);
    CHECK(se1[21] == 0.0f && se1[22] == 0.0f && se1[23] == 0.0f);
    CHECK(se1[0] != se[0]);
  }
  // selections over every shape, threshold and flag: the invariants, a keep mask, threshold < 0
  for (uint32_t flags = 0; flags <= SPT_POOL_EXCLUDE_CENTER; ++flags)
    for (int32_t R : {1, 2, 16})
      for (int32_t band : {0, 3}) {
        const HostFilm f(9, 7, 31u + (uint32_t)R);
        const std::vector<float> se = pool_map(f, band, R, flags);
        float top = 0.0f;
        for (float v : se) top = std::fmax(top, v);
        CHECK(top > 0.0f);
        std::vector<uint8_t> keep(f.npix());
        for (size_t p = 0; p < keep.size(); ++p) keep[p] = p % 3 != 1;
        int64_t last = (int64_t)f.npix() + 1;
        for (double thr : {-1.0, 0.0, 0.3 * top, 0.6 * top, 2.0 * top}) {
          const Selection s = pool_select(f, band, thr, R, flags);
          check_selection(f, s);
          CHECK(s.n <= last);  // a higher threshold keeps no more
          last = s.n;
          const Selection k = pool_select(f, band, thr, R, flags, &keep);
          check_selection(f, k);
          CHECK(k.n <= s.n);
          for (uint32_t p : k.list) CHECK(keep[p] != 0);
        }
        CHECK(last == 0);
      }
  {  // 1x1: the centre excluded leaves n == 0 -- the map reads 0, the pixel's own rule decides
    HostFilm f(1, 1, 41u);
    f.counts[0] = kBMax;
    const spt_film_info i = f.info();
    const spt_film_noise_info n = noise();
    std::vector<float> own(3, -1.0f);
    CHECK(spt_film_adaptive_noise_map_host(f.sums.data(), f.m2.data(), f.counts.data(), &i, &n,
                                           own.data()) == SPT_OK);
    const float top = std::fmax(own[0], std::fmax(own[1], own[2]));
    CHECK(top > 0.0f);
    const std::vector<float> loo = pool_map(f, 0, 1, SPT_POOL_EXCLUDE_CENTER);
    CHECK(loo[0] == 0.0f && loo[1] == 0.0f && loo[2] == 0.0f);
    const std::vector<float> in = pool_map(f, 0, 16, 0);
    for (int c = 0; c < 3; ++c) CHECK(std::fabs(in[c] - own[c]) <= 0x1p-20f * own[c]);
    for (uint32_t flags = 0; flags <= SPT_POOL_EXCLUDE_CENTER; ++flags)
      for (int32_t band : {0, 1, 5}) {
        CHECK(pool_select(f, band, 0.5 * top, 1, flags).n == 1);
        CHECK(pool_select(f, band, 2.0 * top, 16, flags).n == 0);
      }
  }
  {  // rows = 0, and the refused arguments: nothing is written
    const spt_film_info i{9, 0, kSpp, kSpp};
    const spt_film_noise_info n = noise();
    int64_t na = -7;
    CHECK(spt_film_adaptive_select_pooled_host(nullptr, nullptr, nullptr, &i, &n, 0, 0.5, 2, 0, nullptr,
                                               nullptr, nullptr, &na) == SPT_OK && na == 0);
    CHECK(spt_film_noise_pool_map_host(nullptr, nullptr, nullptr, &i, &n, 0, 2, 0, nullptr) == SPT_OK);
    const HostFilm f(5, 3, 51u);
    const spt_film_info fi = f.info();
    std::vector<float> se(3 * f.npix(), -1.0f);
    std::vector<uint32_t> co(f.npix(), 7u), lo(f.npix(), 7u);
    na = -7;
    for (int32_t R : {0, -1, 17})
      CHECK(spt_film_noise_pool_map_host(f.sums.data(), f.m2.data(), f.counts.data(), &fi, &n, 0, R, 0,
                                         se.data()) == SPT_ERR_INVALID_ARG);
    CHECK(spt_film_noise_pool_map_host(f.sums.data(), f.m2.data(), f.counts.data(), &fi, &n, 0, 2, 2u,
                                       se.data()) == SPT_ERR_INVALID_ARG);
    CHECK(spt_film_noise_pool_map_host(f.sums.data(), f.m2.data(), f.counts.data(), &fi, &n, -1, 2, 0,
                                       se.data()) == SPT_ERR_INVALID_ARG);
    CHECK(spt_film_adaptive_select_pooled_host(f.sums.data(), f.m2.data(), f.counts.data(), &fi, &n, 0,
                                               std::nan(""), 2, 0, nullptr, co.data(), lo.data(),
                                               &na) == SPT_ERR_INVALID_ARG);
    CHECK(spt_film_adaptive_select_pooled_host(f.sums.data(), f.m2.data(), f.counts.data(), &fi, &n, 0,
                                               0.5, 17, 0, nullptr, co.data(), lo.data(),
                                               &na) == SPT_ERR_INVALID_ARG);
    CHECK(spt_film_adaptive_select_pooled_host(f.sums.data(), f.m2.data(), f.counts.data(), &fi, &n, 0,
                                               0.5, 2, 4u, nullptr, co.data(), lo.data(),
                                               &na) == SPT_ERR_INVALID_ARG);
    CHECK(na == -7);
    for (float v : se) CHECK(v == -1.0f);
    for (size_t p = 0; p < f.npix(); ++p) CHECK(co[p] == 7u && lo[p] == 7u);
  }
  if (g_failed) {
    std::fprintf(stderr, "spt_film_pool_check: %d check(s) failed\n", g_failed);
    return 1;
  }
  std::printf("spt_film_pool_check ok\n");
  return 0;
}

// spt_film_check.cpp — TEST INFRASTRUCTURE ONLY: a stand-alone host program over the film's CPU
// statements (spt_film_host.cpp, with spt_dispatch.cpp for spt_last_error), built with
// -fsanitize=address,undefined by tests/probe/Makefile and run by tests/test_film_host.py.
// No HIP, no device, never loaded into Python. Every buffer is a std::vector of exactly the size the
// statement may touch, so a read or write past an end is a sanitizer report.
//   * the seven statements on 1x1, 5x3 (n no multiple of 4) and rows = 0, with spp_total = 2 * batch
//     (a two-row range of the table) and 4096 * batch (the largest table);
//   * counts 0, 1, 2 and b_max with and without bit 31, and b_max + 1 refused before it indexes;
//   * every batch sum at the bound batch * 2^31 (the moment's high word set; all clamped), one batch
//     holding everything (B * M2 in 128 bits, unclamped), equal batches (d == 0), and a two-batch
//     element whose standard error is written out;
//   * the null-argument combinations the Python tests probe;
//   * with every count equal to B >= 2 the adaptive statements return the uniform ones bit for bit.
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
constexpr int32_t kBatch = 3;
constexpr u64 kTop = (u64)kBatch << 31;  // the bound of one batch sum

// A film on the host: per element the sum S and the moment M2 = (lo, hi) of B batch sums.
struct HostFilm {
  int32_t w, rows, spp_total;
  std::vector<u64> sums, m2;
  std::vector<uint32_t> counts;
  size_t n() const { return 3 * (size_t)w * (size_t)rows; }
  HostFilm(int32_t w_, int32_t rows_, int32_t spp) : w(w_), rows(rows_), spp_total(spp) {
    sums.resize(n());
    m2.resize(2 * n());
    counts.resize(n() / 3);
  }
  // element e holds the batch sums p[0 .. B)
  void set(size_t e, const std::vector<u64>& p) {
    u64 s = 0;
    u128 m = 0;
    for (u64 v : p) {
      s += v;
      m += (u128)v * v;
    }
    sums[e] = s;
    u64* pair = m2.data() + 2 * e;  // (lo, hi)
    pair[0] = (u64)m;
    pair[1] = (u64)(m >> 64);
  }
  spt_film_info info(int64_t done) const { return spt_film_info{w, rows, spp_total, done}; }
};

static spt_film_noise_info noise(int64_t batches_done) {
  return spt_film_noise_info{1, kBatch, batches_done};
}

static bool same_summary(const spt_noise_summary& a, const spt_noise_summary& b) {
  return std::memcmp(a.rmse, b.rmse, sizeof a.rmse) == 0 &&
         std::memcmp(&a.rmse_all, &b.rmse_all, sizeof a.rmse_all) == 0 &&
         std::memcmp(&a.se_max, &b.se_max, sizeof a.se_max) == 0 && a.clamped == b.clamped &&
         a.batches_done == b.batches_done;
}

// Every count = B >= 2, every batch sum at the bound: all clamped, and the adaptive statements are
// the uniform ones for batches_done = B, samples_done = B * batch.
static void at_the_bound(int32_t w, int32_t rows, int32_t b_max, int32_t B, bool retired) {
  HostFilm f(w, rows, b_max * kBatch);
  const size_t n = f.n();
  for (size_t e = 0; e < n; ++e) f.set(e, std::vector<u64>((size_t)B, kTop));
  for (uint32_t& c : f.counts) c = (uint32_t)B | (retired ? kRetired : 0u);
  if (n) CHECK(f.m2[1] != 0);  // the moment's high word
  const spt_film_info info = f.info((int64_t)B * kBatch);
  const spt_film_noise_info ni = noise(B);
  std::vector<float> ua(n, -1.0f), aa(n, -2.0f);
  CHECK(spt_film_resolve_host(f.sums.data(), &info, ua.data()) == SPT_OK);
  CHECK(spt_film_adaptive_resolve_host(f.sums.data(), f.counts.data(), &info, &ni, aa.data()) == SPT_OK);
  CHECK(n == 0 || std::memcmp(ua.data(), aa.data(), n * sizeof(float)) == 0);
  for (float v : aa) CHECK(v == 1.0f);
  CHECK(spt_film_noise_map_host(f.sums.data(), f.m2.data(), &info, &ni, ua.data()) == SPT_OK);
  CHECK(spt_film_adaptive_noise_map_host(f.sums.data(), f.m2.data(), f.counts.data(), &info, &ni,
                                         aa.data()) == SPT_OK);
  CHECK(n == 0 || std::memcmp(ua.data(), aa.data(), n * sizeof(float)) == 0);
  for (float v : aa) CHECK(v == 0.0f);  // a clamped element: se 0
  spt_noise_summary us, as;
  std::memset(&us, 0xAB, sizeof us);
  std::memset(&as, 0xCD, sizeof as);
  CHECK(spt_film_noise_summary_host(f.sums.data(), f.m2.data(), &info, &ni, &us) == SPT_OK);
  CHECK(spt_film_adaptive_noise_summary_host(f.sums.data(), f.m2.data(), f.counts.data(), &info, &ni,
                                             &as) == SPT_OK);
  CHECK(same_summary(us, as));
  CHECK(as.clamped == n && as.se_max == 0.0f && as.rmse_all == 0.0 && as.batches_done == B);
  CHECK(as.rmse[0] == 0.0 && as.rmse[1] == 0.0 && as.rmse[2] == 0.0);
}

// Unclamped elements, every count = B: equal batches (d == 0) on the even elements, one batch holding
// everything (B * M2 above 64 bits for a large B) on the odd ones. Adaptive == uniform, bit for bit.
static void below_the_clamp(int32_t w, int32_t rows, int32_t b_max, int32_t B) {
  HostFilm f(w, rows, b_max * kBatch);
  const size_t n = f.n();
  const u64 P = 0x1p30;
  for (size_t e = 0; e < n; ++e) {
    std::vector<u64> p((size_t)B, e % 2 ? 0 : P / (u64)b_max);
    if (e % 2) p[e % (size_t)B] = P * (u64)B / (u64)b_max;  // resolves to 0.5 at any depth
    f.set(e, p);
  }
  for (uint32_t& c : f.counts) c = (uint32_t)B;
  const spt_film_info info = f.info((int64_t)B * kBatch);
  const spt_film_noise_info ni = noise(B);
  std::vector<float> ua(n, -1.0f), aa(n, -2.0f);
  CHECK(spt_film_resolve_host(f.sums.data(), &info, ua.data()) == SPT_OK);
  CHECK(spt_film_adaptive_resolve_host(f.sums.data(), f.counts.data(), &info, &ni, aa.data()) == SPT_OK);
  CHECK(n == 0 || std::memcmp(ua.data(), aa.data(), n * sizeof(float)) == 0);
  CHECK(spt_film_noise_map_host(f.sums.data(), f.m2.data(), &info, &ni, ua.data()) == SPT_OK);
  CHECK(spt_film_adaptive_noise_map_host(f.sums.data(), f.m2.data(), f.counts.data(), &info, &ni,
                                         aa.data()) == SPT_OK);
  CHECK(n == 0 || std::memcmp(ua.data(), aa.data(), n * sizeof(float)) == 0);
  // S = P * B / b_max in one batch of B: D = B * S^2 - S^2 = (B - 1) * S^2, in 128 bits for B = 4096
  const double S = (double)(P * (u64)B / (u64)b_max);
  const double k = (double)(b_max * kBatch) / ((double)kBatch * 0x1p31 * (double)B * std::sqrt((double)(B - 1)));
  const float want = (float)(std::sqrt((double)(B - 1) * S * S) * k);
  for (size_t e = 0; e < n; ++e) CHECK(aa[e] == (e % 2 ? want : 0.0f));
  if (n > 1 && B == 4096)  // B * M2 of element 1 does not fit 64 bits
    CHECK((((u128)B * (((u128)f.m2[3] << 64) | f.m2[2])) >> 64) != 0);
  spt_noise_summary us, as;
  CHECK(spt_film_noise_summary_host(f.sums.data(), f.m2.data(), &info, &ni, &us) == SPT_OK);
  CHECK(spt_film_adaptive_noise_summary_host(f.sums.data(), f.m2.data(), f.counts.data(), &info, &ni,
                                             &as) == SPT_OK);
  CHECK(same_summary(us, as));
  CHECK(as.clamped == 0 && as.se_max == (n > 1 ? want : 0.0f) && as.batches_done == B);
  // the selection at threshold 0 keeps exactly the pixels with a noisy channel; below 0, all
  std::vector<uint32_t> co(n / 3, 0xFFFFFFFFu), list(n / 3, 0xFFFFFFFFu);
  int64_t na = -1;
  CHECK(spt_film_adaptive_select_host(f.sums.data(), f.m2.data(), f.counts.data(), &info, &ni, 0.0,
                                      nullptr, co.data(), list.data(), &na) == SPT_OK);
  CHECK(na == (int64_t)(n / 3));  // every pixel has an odd element
  CHECK(spt_film_adaptive_select_host(f.sums.data(), f.m2.data(), f.counts.data(), &info, &ni, 1.0,
                                      nullptr, co.data(), list.data(), &na) == SPT_OK);
  CHECK(na == 0);
  for (uint32_t c : co) CHECK(c == ((uint32_t)B | kRetired));
  std::vector<uint8_t> keep(n / 3, 0);
  if (!keep.empty()) keep.back() = 1;
  CHECK(spt_film_adaptive_select_host(f.sums.data(), f.m2.data(), f.counts.data(), &info, &ni, -1.0,
                                      keep.data(), co.data(), list.data(), &na) == SPT_OK);
  CHECK(na == (n ? 1 : 0));
  if (n) CHECK(list[0] == n / 3 - 1 && co.back() == (uint32_t)B && (n == 3 || co[0] == ((uint32_t)B | kRetired)));
}

// Counts 0, 1, 2 and b_max, with and without bit 31, on the 5x3 film; b_max + 1 is refused.
static void mixed_counts(int32_t b_max) {
  HostFilm f(5, 3, b_max * kBatch);
  const size_t n = f.n(), npix = n / 3;
  const uint32_t depth[4] = {0u, 1u, 2u, (uint32_t)b_max};
  const u64 u = (1u << 21) / (u64)b_max;  // small enough that no depth reaches the clamp
  for (size_t p = 0; p < npix; ++p) {
    const uint32_t B = depth[p % 4];
    f.counts[p] = B | (p % 8 >= 4 ? kRetired : 0u);
    // two unequal batches where there are two (D = (3u - u)^2), equal ones elsewhere
    for (int c = 0; c < 3; ++c) {
      std::vector<u64> b(B, u);
      if (B == 2) b[0] = 3 * u;
      f.set(3 * p + (size_t)c, b);
    }
  }
  const spt_film_info info = f.info(0);
  const spt_film_noise_info ni = noise(b_max);
  std::vector<float> rgb(n, -1.0f), se(n, -1.0f);
  CHECK(spt_film_adaptive_resolve_host(f.sums.data(), f.counts.data(), &info, &ni, rgb.data()) == SPT_OK);
  CHECK(spt_film_adaptive_noise_map_host(f.sums.data(), f.m2.data(), f.counts.data(), &info, &ni,
                                         se.data()) == SPT_OK);
  // B = 2: D = 4 u^2, k = spp / (batch * 2^31 * 2 * sqrt(1)), se = sqrt(D) * k (2^-10 for b_max = 2)
  const double k2b = (double)(b_max * kBatch) / ((double)kBatch * 0x1p31 * 2.0 * std::sqrt(1.0));
  const float se2 = (float)(std::sqrt(4.0 * (double)u * (double)u) * k2b);
  if (b_max == 2) CHECK(se2 == 0x1p-10f);
  for (size_t e = 0; e < n; ++e) {
    const uint32_t B = f.counts[e / 3] & ~kRetired;
    if (B == 0) CHECK(rgb[e] == 0.0f);
    if (B == (uint32_t)b_max && B != 2) CHECK(rgb[e] == (float)(B * u) * 0x1p-31f);  // no factor
    CHECK(se[e] == (B == 2 ? se2 : 0.0f));  // fewer than two batches, or equal batches: 0
  }
  spt_noise_summary s;
  CHECK(spt_film_adaptive_noise_summary_host(f.sums.data(), f.m2.data(), f.counts.data(), &info, &ni,
                                             &s) == SPT_OK);
  CHECK(s.se_max == se2 && s.clamped == 0 && s.batches_done == b_max && s.rmse_all > 0.0);
  std::vector<uint32_t> co(npix), list(npix);
  int64_t na = -1;
  CHECK(spt_film_adaptive_select_host(f.sums.data(), f.m2.data(), f.counts.data(), &info, &ni, -1.0,
                                      nullptr, co.data(), list.data(), &na) == SPT_OK);
  CHECK(na == 8 && co == f.counts);  // pixels 0-3 and 8-11 are active
  // one count above the table: refused before anything is indexed (the outputs stay untouched)
  f.counts[npix - 1] = (uint32_t)(b_max + 1) | kRetired;
  std::fill(rgb.begin(), rgb.end(), -7.0f);
  CHECK(spt_film_adaptive_resolve_host(f.sums.data(), f.counts.data(), &info, &ni, rgb.data()) ==
        SPT_ERR_INVALID_ARG);
  CHECK(std::strcmp(spt_last_error(), "a count above spp_total / batch") == 0);
  CHECK(spt_film_adaptive_noise_map_host(f.sums.data(), f.m2.data(), f.counts.data(), &info, &ni,
                                         rgb.data()) == SPT_ERR_INVALID_ARG);
  CHECK(spt_film_adaptive_noise_summary_host(f.sums.data(), f.m2.data(), f.counts.data(), &info, &ni,
                                             &s) == SPT_ERR_INVALID_ARG);
  CHECK(spt_film_adaptive_select_host(f.sums.data(), f.m2.data(), f.counts.data(), &info, &ni, 0.5,
                                      nullptr, co.data(), list.data(), &na) == SPT_ERR_INVALID_ARG);
  for (float v : rgb) CHECK(v == -7.0f);
}

// The null-argument combinations of tests/test_film.py, test_film_noise.py and test_film_adaptive.py.
static void bad_arguments() {
  HostFilm f(5, 3, 2 * kBatch);
  for (size_t e = 0; e < f.n(); ++e) f.set(e, {1u << 20, 1u << 20});
  for (uint32_t& c : f.counts) c = 2;
  const spt_film_info I = f.info(2 * kBatch), bad = f.info(2 * kBatch + 1);
  const spt_film_noise_info N = noise(2), plain{0, 0, 0}, one = noise(1);
  const u64 *a = f.sums.data(), *m = f.m2.data();
  const uint32_t* c = f.counts.data();
  std::vector<float> out(f.n());
  std::vector<uint32_t> co(f.n() / 3), list(f.n() / 3);
  spt_noise_summary s;
  int64_t na = 0;
  const spt_status E = SPT_ERR_INVALID_ARG;
  CHECK(spt_film_resolve_host(a, &I, out.data()) == SPT_OK);
  CHECK(spt_film_resolve_host(a, &bad, out.data()) == E);
  CHECK(std::strcmp(spt_last_error(), "bad film info") == 0);
  CHECK(spt_film_resolve_host(nullptr, nullptr, nullptr) == E);
  CHECK(std::strcmp(spt_last_error(), "null info") == 0);
  CHECK(spt_film_resolve_host(nullptr, &I, out.data()) == E);
  CHECK(spt_film_resolve_host(a, &I, nullptr) == E);
  CHECK(spt_film_noise_map_host(a, m, &I, &N, out.data()) == SPT_OK);
  CHECK(spt_film_noise_map_host(nullptr, m, &I, &N, out.data()) == E);
  CHECK(spt_film_noise_map_host(a, nullptr, &I, &N, out.data()) == E);
  CHECK(spt_film_noise_map_host(a, m, &I, &N, nullptr) == E);
  CHECK(spt_film_noise_map_host(a, m, nullptr, &N, out.data()) == E);
  CHECK(spt_film_noise_map_host(a, m, &I, nullptr, out.data()) == E);
  CHECK(spt_film_noise_map_host(a, m, &I, &plain, out.data()) == E);
  CHECK(std::strcmp(spt_last_error(), "not a noise film") == 0);
  CHECK(spt_film_noise_map_host(a, m, &I, &one, out.data()) == E);
  CHECK(std::strcmp(spt_last_error(), "the error needs at least two batches") == 0);
  CHECK(spt_film_noise_summary_host(a, m, &I, &N, &s) == SPT_OK);
  CHECK(spt_film_noise_summary_host(nullptr, m, &I, &N, &s) == E);
  CHECK(spt_film_noise_summary_host(a, nullptr, &I, &N, &s) == E);
  CHECK(spt_film_noise_summary_host(a, m, &I, &N, nullptr) == E);
  CHECK(spt_film_adaptive_resolve_host(a, c, &I, &N, out.data()) == SPT_OK);
  CHECK(spt_film_adaptive_resolve_host(nullptr, c, &I, &N, out.data()) == E);
  CHECK(spt_film_adaptive_resolve_host(a, nullptr, &I, &N, out.data()) == E);
  CHECK(std::strcmp(spt_last_error(), "null counts") == 0);
  CHECK(spt_film_adaptive_resolve_host(a, c, &I, &N, nullptr) == E);
  CHECK(spt_film_adaptive_resolve_host(a, c, nullptr, &N, out.data()) == E);
  CHECK(spt_film_adaptive_resolve_host(a, c, &I, &plain, out.data()) == E);
  CHECK(std::strcmp(spt_last_error(), "not an adaptive film's batch") == 0);
  CHECK(spt_film_adaptive_noise_map_host(a, nullptr, c, &I, &N, out.data()) == E);
  CHECK(spt_film_adaptive_noise_summary_host(a, m, c, &I, &N, nullptr) == E);
  CHECK(spt_film_adaptive_select_host(a, m, c, &I, &N, 0.5, nullptr, co.data(), list.data(), nullptr) == E);
  CHECK(spt_film_adaptive_select_host(a, m, c, &I, &N, std::nan(""), nullptr, co.data(), list.data(), &na) == E);
  CHECK(spt_film_adaptive_select_host(a, m, c, &I, &one, 0.5, nullptr, co.data(), list.data(), &na) == E);
  CHECK(std::strcmp(spt_last_error(), "the selection needs at least two batches") == 0);
  CHECK(spt_film_adaptive_select_host(a, m, c, &I, &N, 0.5, nullptr, nullptr, list.data(), &na) == E);
  // more than 4096 batches, and a batch that does not divide spp
  const spt_film_info big{5, 3, 4097 * kBatch, 0}, odd{5, 3, 2 * kBatch + 1, 0};
  CHECK(spt_film_adaptive_resolve_host(a, c, &big, &N, out.data()) == E);
  CHECK(spt_film_adaptive_resolve_host(a, c, &odd, &N, out.data()) == E);
}

int main() {
  for (int32_t b_max : {2, 4096}) {
    for (int32_t B : {2, b_max}) {
      at_the_bound(1, 1, b_max, B, false);
      at_the_bound(5, 3, b_max, B, true);
      at_the_bound(5, 0, b_max, B, false);  // rows = 0: nothing is touched, the summary is all zero
      below_the_clamp(1, 1, b_max, B);
      below_the_clamp(5, 3, b_max, B);
      below_the_clamp(5, 0, b_max, B);
    }
    mixed_counts(b_max);
  }
  bad_arguments();
  if (g_failed) {
    std::fprintf(stderr, "spt_film_check: %d checks failed\n", g_failed);
    return 1;
  }
  std::printf("spt_film_check ok\n");
  return 0;
}

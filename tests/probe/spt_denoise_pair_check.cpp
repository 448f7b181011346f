// spt_denoise_pair_check.cpp — TEST INFRASTRUCTURE ONLY: a stand-alone host program over the two-half
// filter's CPU statement and its summary (spt_denoise_pair_host, spt_denoise_pair_summary_host in
// spt_denoise_host.cpp, with spt_dispatch.cpp for spt_last_error), built with
// -fsanitize=address,undefined by tests/probe/denoise_pair_check.mk and run by
// tests/test_denoise_pair_host.py. No HIP, no device, never loaded into Python. Every buffer is a
// std::vector of exactly the size the statement may touch, so a read or write past a plane is a
// sanitizer report: the 3x2 image at step 32 (iterations = 6) is where an unclipped tap address would
// be caught. Sizes 1x1, 3x2, 5x1, 1x5, 17x13 and 40x56; iterations 0, 1 and 6; both flag values and both
// pair_flags; se_out and diff left NULL; equal and swapped halves; every refused argument, with the
// outputs checked for their fill pattern.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
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

namespace {

struct Planes {
  int32_t w, h;
  std::vector<float> rgb_a, se_a, rgb_b, se_b, albedo, normal, depth;
};

uint32_t g_state = 12345u;
float rnd() {  // [0, 1)
  g_state = g_state * 1664525u + 1013904223u;
  return (float)(g_state >> 8) * 0x1p-24f;
}

// Two regions with orthogonal normals, independent noise on the two halves' colours, one miss pixel
// where there is room.
Planes make(int32_t w, int32_t h) {
  Planes p{w, h, {}, {}, {}, {}, {}, {}, {}};
  const size_t n = (size_t)w * h;
  for (std::vector<float>* v : {&p.rgb_a, &p.se_a, &p.rgb_b, &p.se_b, &p.albedo, &p.normal}) v->resize(3 * n);
  p.depth.resize(n);
  for (int32_t y = 0; y < h; ++y)
    for (int32_t x = 0; x < w; ++x) {
      const size_t i = (size_t)y * w + x;
      const bool right = x >= w / 2;
      for (int k = 0; k < 3; ++k) {
        p.albedo[3 * i + k] = right ? 0.2f + 0.3f * k : 0.7f - 0.2f * k;
        p.rgb_a[3 * i + k] = p.albedo[3 * i + k] * 0.6f + 0.07f * (rnd() - 0.5f);
        p.rgb_b[3 * i + k] = p.albedo[3 * i + k] * 0.6f + 0.07f * (rnd() - 0.5f);
        p.se_a[3 * i + k] = 0.028f;
        p.se_b[3 * i + k] = 0.03f;
        p.normal[3 * i + k] = (right ? k == 0 : k == 2) ? 1.0f : 0.0f;
      }
      p.depth[i] = right ? 20.0f - 0.1f * x : 10.0f + 0.05f * x + 0.03f * y;
    }
  if (n >= 6) {  // a miss: all features zero
    const size_t i = n / 2;
    for (int k = 0; k < 3; ++k) p.albedo[3 * i + k] = p.normal[3 * i + k] = 0.0f;
    p.depth[i] = 0.0f;
  }
  return p;
}

spt_status run(const Planes& p, const spt_denoise_params& dp, uint32_t pf, float* out, float* se_out,
               float* diff) {
  return spt_denoise_pair_host(p.rgb_a.data(), p.se_a.data(), p.rgb_b.data(), p.se_b.data(), p.albedo.data(),
                               p.normal.data(), p.depth.data(), p.w, p.h, &dp, pf, out, se_out, diff);
}

bool all_are(const std::vector<float>& v, float fill) {
  for (float x : v)
    if (std::memcmp(&x, &fill, 4) != 0) return false;
  return true;
}

}  // namespace

int main() {
  static_assert(sizeof(spt_pair_summary) == 40, "spt_pair_summary");
  spt_denoise_params def;
  spt_denoise_default_params(&def);
  const int32_t sizes[6][2] = {{1, 1}, {3, 2}, {5, 1}, {1, 5}, {17, 13}, {40, 56}};
  const float fill = -7.25f;
  for (const auto& s : sizes) {
    const Planes p = make(s[0], s[1]);
    Planes swapped = p;
    swapped.rgb_a.swap(swapped.rgb_b);
    swapped.se_a.swap(swapped.se_b);
    Planes equal = p;
    equal.rgb_b = equal.rgb_a;
    equal.se_b = equal.se_a;
    const size_t n3 = p.rgb_a.size();
    for (uint32_t pf = 0; pf <= 1; ++pf)
      for (uint32_t flags = 0; flags <= 1; ++flags)
        for (int32_t it : {0, 1, 6}) {
          spt_denoise_params dp = def;
          dp.iterations = it;
          dp.flags = flags;
          std::vector<float> out(n3, fill), se_out(n3, fill), diff(n3, fill), out2(n3, fill), diff2(n3, fill);
          CHECK(run(p, dp, pf, out.data(), se_out.data(), diff.data()) == SPT_OK);
          CHECK(run(p, dp, pf, out2.data(), nullptr, nullptr) == SPT_OK);  // the optional planes left out
          CHECK(std::memcmp(out.data(), out2.data(), n3 * 4) == 0);
          CHECK(run(p, dp, pf, out2.data(), nullptr, diff2.data()) == SPT_OK);
          CHECK(std::memcmp(diff.data(), diff2.data(), n3 * 4) == 0);
          for (size_t k = 0; k < n3; ++k) {
            CHECK(std::isfinite(out[k]) && out[k] <= 1.0f && std::fabs(out[k] - p.rgb_a[k]) < 0.15f);
            CHECK(std::isfinite(se_out[k]) && se_out[k] >= 0.0f);
            CHECK(std::isfinite(diff[k]) && std::fabs(diff[k]) < 0.1f);
            if (it == 0) {
              CHECK(out[k] == 0.5f * (p.rgb_a[k] + p.rgb_b[k]) && diff[k] == 0.5f * (p.rgb_a[k] - p.rgb_b[k]));
              CHECK(se_out[k] == 0.5f * std::sqrt(p.se_a[k] * p.se_a[k] + p.se_b[k] * p.se_b[k]));
            }
          }
          // swapped halves: out and se_out keep their bits, diff is negated
          std::vector<float> outs(n3, fill), ses(n3, fill), diffs(n3, fill);
          CHECK(run(swapped, dp, pf, outs.data(), ses.data(), diffs.data()) == SPT_OK);
          CHECK(std::memcmp(out.data(), outs.data(), n3 * 4) == 0);
          CHECK(std::memcmp(se_out.data(), ses.data(), n3 * 4) == 0);
          for (size_t k = 0; k < n3; ++k) CHECK(diff[k] == -diffs[k]);
          // equal halves: the single filter's image, diff +0
          std::vector<float> oute(n3, fill), diffe(n3, fill), single(n3, fill);
          CHECK(run(equal, dp, pf, oute.data(), nullptr, diffe.data()) == SPT_OK);
          CHECK(spt_denoise_host(equal.rgb_a.data(), equal.se_a.data(), equal.albedo.data(), equal.normal.data(),
                                 equal.depth.data(), equal.w, equal.h, &dp, single.data(), nullptr) == SPT_OK);
          CHECK(std::memcmp(oute.data(), single.data(), n3 * 4) == 0);
          CHECK(all_are(diffe, 0.0f));
          // the summary of this diff plane against a plain loop
          spt_pair_summary sm;
          std::memset(&sm, 0xff, sizeof sm);
          CHECK(spt_denoise_pair_summary_host(diff.data(), p.w, p.h, &sm) == SPT_OK);
          double s3[3] = {0, 0, 0};
          float mx = 0.0f;
          for (size_t k = 0; k < n3; ++k) {
            s3[k % 3] += (double)diff[k] * (double)diff[k];
            mx = std::fmax(mx, std::fabs(diff[k]));
          }
          const double npx = (double)(n3 / 3);
          for (int k = 0; k < 3; ++k) CHECK(sm.rmse[k] == std::sqrt(s3[k] / npx));
          CHECK(sm.rmse_all == std::sqrt(((s3[0] + s3[1]) + s3[2]) / (3.0 * npx)));
          CHECK(sm.diff_max == mx && sm.reserved == 0);
        }
  }
  {  // inputs that are not finite: unspecified values, no fault
    Planes p = make(17, 13);
    p.rgb_a[5] = std::numeric_limits<float>::quiet_NaN();
    p.rgb_b[11] = std::numeric_limits<float>::infinity();
    p.se_a[40] = std::numeric_limits<float>::infinity();
    p.se_b[41] = std::numeric_limits<float>::quiet_NaN();
    p.depth[7] = -std::numeric_limits<float>::infinity();
    p.normal[100] = std::numeric_limits<float>::quiet_NaN();
    p.albedo[200] = -1e30f;
    std::vector<float> out(p.rgb_a.size(), fill), se_out(p.rgb_a.size(), fill), diff(p.rgb_a.size(), fill);
    for (uint32_t pf = 0; pf <= 1; ++pf) CHECK(run(p, def, pf, out.data(), se_out.data(), diff.data()) == SPT_OK);
    spt_pair_summary sm;
    CHECK(spt_denoise_pair_summary_host(diff.data(), 17, 13, &sm) == SPT_OK);
  }
  {  // the refusals: SPT_ERR_INVALID_ARG, a message, the outputs untouched
    const Planes p = make(3, 2);
    const size_t n3 = p.rgb_a.size();
    std::vector<float> out(n3, fill), se_out(n3, fill), diff(n3, fill);
    auto refused = [&](spt_status st) {
      CHECK(st == SPT_ERR_INVALID_ARG);
      CHECK(spt_last_error()[0] != 0);
      CHECK(all_are(out, fill) && all_are(se_out, fill) && all_are(diff, fill));
    };
    const float* in[7] = {p.rgb_a.data(), p.se_a.data(), p.rgb_b.data(), p.se_b.data(),
                          p.albedo.data(), p.normal.data(), p.depth.data()};
    auto call = [&](const float* const a[7], int32_t w, int32_t h, const spt_denoise_params* dp, uint32_t pf,
                    float* o, float* s, float* d) {
      return spt_denoise_pair_host(a[0], a[1], a[2], a[3], a[4], a[5], a[6], w, h, dp, pf, o, s, d);
    };
    for (int k = 0; k < 7; ++k) {
      const float* a[7] = {in[0], in[1], in[2], in[3], in[4], in[5], in[6]};
      a[k] = nullptr;
      refused(call(a, 3, 2, &def, 0, out.data(), se_out.data(), diff.data()));
    }
    refused(call(in, 3, 2, nullptr, 0, out.data(), se_out.data(), diff.data()));
    refused(call(in, 3, 2, &def, 0, nullptr, se_out.data(), diff.data()));
    refused(call(in, 3, 2, &def, 0, out.data(), out.data(), diff.data()));
    refused(call(in, 3, 2, &def, 0, out.data(), se_out.data(), out.data()));
    refused(call(in, 3, 2, &def, 0, out.data(), se_out.data(), se_out.data()));
    for (uint32_t pf : {2u, 3u, 0x80000000u, 0xFFFFFFFFu})
      refused(call(in, 3, 2, &def, pf, out.data(), se_out.data(), diff.data()));
    const int32_t dims[5][2] = {{0, 2}, {3, 0}, {-3, 2}, {3, -2}, {65536, 32768}};
    for (const auto& d : dims) refused(call(in, d[0], d[1], &def, 0, out.data(), se_out.data(), diff.data()));
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    for (int field = 0; field < 4; ++field)
      for (float bad : {0.0f, -1.0f, nan, inf, -inf}) {
        spt_denoise_params dp = def;
        (field == 0 ? dp.sigma_color : field == 1 ? dp.sigma_depth : field == 2 ? dp.sigma_albedo : dp.albedo_floor) = bad;
        refused(run(p, dp, 0, out.data(), se_out.data(), diff.data()));
      }
    for (int32_t it : {-1, 7, INT32_MAX, INT32_MIN}) {
      spt_denoise_params dp = def;
      dp.iterations = it;
      refused(run(p, dp, 0, out.data(), se_out.data(), diff.data()));
      dp = def;
      dp.normal_squarings = it == 7 ? 9 : it;
      refused(run(p, dp, 1, out.data(), se_out.data(), diff.data()));
    }
    for (uint32_t fl : {2u, 3u, 0x80000000u}) {
      spt_denoise_params dp = def;
      dp.flags = fl;  // SPT_DENOISE_PAIR_OWN_WEIGHTS is no bit of params->flags
      refused(run(p, dp, 0, out.data(), se_out.data(), diff.data()));
    }
    spt_denoise_params dp = def;
    dp.reserved = 1;
    refused(run(p, dp, 0, out.data(), se_out.data(), diff.data()));
    // an output that is an input: refused before anything is written (the inputs keep their bits)
    Planes q = make(3, 2);
    const Planes before = q;
    float* planes6[6] = {q.rgb_a.data(), q.se_a.data(), q.rgb_b.data(), q.se_b.data(), q.albedo.data(),
                         q.normal.data()};
    for (float* pl : planes6) {
      CHECK(run(q, def, 0, pl, nullptr, nullptr) == SPT_ERR_INVALID_ARG);
      CHECK(run(q, def, 0, out.data(), pl, nullptr) == SPT_ERR_INVALID_ARG);
      CHECK(run(q, def, 0, out.data(), nullptr, pl) == SPT_ERR_INVALID_ARG);
    }
    CHECK(q.rgb_a == before.rgb_a && q.se_a == before.se_a && q.rgb_b == before.rgb_b && q.se_b == before.se_b &&
          q.albedo == before.albedo && q.normal == before.normal && all_are(out, fill));
    // the summary's refusals leave *out untouched
    spt_pair_summary sm;
    std::memset(&sm, 0x5a, sizeof sm);
    const spt_pair_summary keep = sm;
    CHECK(spt_denoise_pair_summary_host(nullptr, 3, 2, &sm) == SPT_ERR_INVALID_ARG);
    CHECK(spt_denoise_pair_summary_host(diff.data(), 3, 2, nullptr) == SPT_ERR_INVALID_ARG);
    for (const auto& d : dims) CHECK(spt_denoise_pair_summary_host(diff.data(), d[0], d[1], &sm) == SPT_ERR_INVALID_ARG);
    CHECK(std::memcmp(&sm, &keep, sizeof sm) == 0);
  }
  if (g_failed) {
    std::fprintf(stderr, "spt_denoise_pair_check: %d checks failed\n", g_failed);
    return 1;
  }
  std::printf("spt_denoise_pair_check ok\n");
  return 0;
}

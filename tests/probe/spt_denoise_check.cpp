// spt_denoise_check.cpp — TEST INFRASTRUCTURE ONLY: a stand-alone host program over the a-trous
// filter's CPU statement (spt_denoise_host in spt_denoise_host.cpp, with spt_dispatch.cpp for
// spt_last_error), built with -fsanitize=address,undefined by tests/probe/denoise_check.mk and run by
// tests/test_denoise_host.py. No HIP, no device, never loaded into Python. Every buffer is a
// std::vector of exactly the size the statement may touch, so a read or write past a plane is a
// sanitizer report: the 3x2 image at step 32 (iterations = 6) is where an unclipped tap address would
// be caught. Sizes 1x1, 3x2, 5x1, 1x5, 17x13 and 40x56; iterations 0 and 6; se_out left NULL; both
// flag values; every refused argument, with the outputs checked for their fill pattern.
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
  std::vector<float> rgb, se, albedo, normal, depth;
};

uint32_t g_state = 12345u;
float rnd() {  // [0, 1)
  g_state = g_state * 1664525u + 1013904223u;
  return (float)(g_state >> 8) * 0x1p-24f;
}

// Two regions with orthogonal normals, noise on the colour, one miss pixel where there is room.
Planes make(int32_t w, int32_t h) {
  Planes p{w, h, {}, {}, {}, {}, {}};
  const size_t n = (size_t)w * h;
  p.rgb.resize(3 * n);
  p.se.resize(3 * n);
  p.albedo.resize(3 * n);
  p.normal.resize(3 * n);
  p.depth.resize(n);
  for (int32_t y = 0; y < h; ++y)
    for (int32_t x = 0; x < w; ++x) {
      const size_t i = (size_t)y * w + x;
      const bool right = x >= w / 2;
      for (int k = 0; k < 3; ++k) {
        p.albedo[3 * i + k] = right ? 0.2f + 0.3f * k : 0.7f - 0.2f * k;
        p.rgb[3 * i + k] = p.albedo[3 * i + k] * 0.6f + 0.05f * (rnd() - 0.5f);
        p.se[3 * i + k] = 0.02f;
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

spt_status run(const Planes& p, const spt_denoise_params& dp, float* out, float* se_out) {
  return spt_denoise_host(p.rgb.data(), p.se.data(), p.albedo.data(), p.normal.data(), p.depth.data(),
                          p.w, p.h, &dp, out, se_out);
}

bool all_are(const std::vector<float>& v, float fill) {
  for (float x : v)
    if (std::memcmp(&x, &fill, 4) != 0) return false;
  return true;
}

}  // namespace

int main() {
  static_assert(sizeof(spt_denoise_params) == 32, "spt_denoise_params");
  spt_denoise_params def;
  spt_denoise_default_params(&def);
  CHECK(def.iterations == 5 && def.sigma_color == 4.0f && def.sigma_depth == 1.0f);
  CHECK(def.sigma_albedo == 0.1f && def.normal_squarings == 7 && def.albedo_floor == 0.01f);
  CHECK(def.flags == 0 && def.reserved == 0);
  spt_denoise_default_params(nullptr);  // ignored

  const int32_t sizes[6][2] = {{1, 1}, {3, 2}, {5, 1}, {1, 5}, {17, 13}, {40, 56}};
  const float fill = -7.25f;
  for (const auto& s : sizes) {
    const Planes p = make(s[0], s[1]);
    const size_t n3 = p.rgb.size();
    for (uint32_t flags = 0; flags <= 1; ++flags)
      for (int32_t it : {0, 1, 6}) {
        spt_denoise_params dp = def;
        dp.iterations = it;
        dp.flags = flags;
        std::vector<float> out(n3, fill), se_out(n3, fill), out2(n3, fill);
        CHECK(run(p, dp, out.data(), se_out.data()) == SPT_OK);
        CHECK(run(p, dp, out2.data(), nullptr) == SPT_OK);  // the optional plane left out
        CHECK(std::memcmp(out.data(), out2.data(), n3 * 4) == 0);
        if (it == 0) {
          CHECK(std::memcmp(out.data(), p.rgb.data(), n3 * 4) == 0);
          CHECK(std::memcmp(se_out.data(), p.se.data(), n3 * 4) == 0);
        }
        for (size_t k = 0; k < n3; ++k) {
          CHECK(std::isfinite(out[k]) && out[k] <= 1.0f && std::fabs(out[k] - p.rgb[k]) < 0.1f);
          CHECK(std::isfinite(se_out[k]) && se_out[k] >= 0.0f);
        }
      }
  }
  {  // a constant image: every tap carries the centre's colour, so the mean is the colour (a few ulp)
    Planes p = make(17, 13);
    for (size_t i = 0; i < p.depth.size(); ++i)
      for (int k = 0; k < 3; ++k) {
        p.rgb[3 * i + k] = 0.3f + 0.1f * k;
        p.albedo[3 * i + k] = 0.5f;
        p.normal[3 * i + k] = k == 2 ? 1.0f : 0.0f;
      }
    std::vector<float> out(p.rgb.size(), fill), se_out(p.rgb.size(), fill);
    CHECK(run(p, def, out.data(), se_out.data()) == SPT_OK);
    for (size_t k = 0; k < out.size(); ++k) CHECK(std::fabs(out[k] - p.rgb[k]) < 1e-6f);
    for (size_t k = 0; k < out.size(); ++k) CHECK(se_out[k] < 0.02f);
  }
  {  // inputs that are not finite: unspecified values, no fault
    Planes p = make(17, 13);
    p.rgb[5] = std::numeric_limits<float>::quiet_NaN();
    p.se[40] = std::numeric_limits<float>::infinity();
    p.depth[7] = -std::numeric_limits<float>::infinity();
    p.normal[100] = std::numeric_limits<float>::quiet_NaN();
    p.albedo[200] = -1e30f;
    std::vector<float> out(p.rgb.size(), fill), se_out(p.rgb.size(), fill);
    CHECK(run(p, def, out.data(), se_out.data()) == SPT_OK);
  }
  {  // the refusals: SPT_ERR_INVALID_ARG, a message, the outputs untouched
    const Planes p = make(3, 2);
    std::vector<float> out(p.rgb.size(), fill), se_out(p.rgb.size(), fill);
    auto refused = [&](spt_status st) {
      CHECK(st == SPT_ERR_INVALID_ARG);
      CHECK(spt_last_error()[0] != 0);
      CHECK(all_are(out, fill) && all_are(se_out, fill));
    };
    const float* in[5] = {p.rgb.data(), p.se.data(), p.albedo.data(), p.normal.data(), p.depth.data()};
    for (int k = 0; k < 5; ++k) {
      const float* a[5] = {in[0], in[1], in[2], in[3], in[4]};
      a[k] = nullptr;
      refused(spt_denoise_host(a[0], a[1], a[2], a[3], a[4], 3, 2, &def, out.data(), se_out.data()));
    }
    refused(spt_denoise_host(in[0], in[1], in[2], in[3], in[4], 3, 2, nullptr, out.data(), se_out.data()));
    refused(spt_denoise_host(in[0], in[1], in[2], in[3], in[4], 3, 2, &def, nullptr, se_out.data()));
    refused(spt_denoise_host(in[0], in[1], in[2], in[3], in[4], 3, 2, &def, out.data(), out.data()));
    const int32_t dims[5][2] = {{0, 2}, {3, 0}, {-3, 2}, {3, -2}, {65536, 32768}};
    for (const auto& d : dims)
      refused(spt_denoise_host(in[0], in[1], in[2], in[3], in[4], d[0], d[1], &def, out.data(), se_out.data()));
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    for (int field = 0; field < 4; ++field)
      for (float bad : {0.0f, -1.0f, nan, inf, -inf}) {
        spt_denoise_params dp = def;
        (field == 0 ? dp.sigma_color : field == 1 ? dp.sigma_depth : field == 2 ? dp.sigma_albedo : dp.albedo_floor) = bad;
        refused(run(p, dp, out.data(), se_out.data()));
      }
    for (int32_t it : {-1, 7, INT32_MAX, INT32_MIN}) {
      spt_denoise_params dp = def;
      dp.iterations = it;
      refused(run(p, dp, out.data(), se_out.data()));
      dp = def;
      dp.normal_squarings = it == 7 ? 9 : it;
      refused(run(p, dp, out.data(), se_out.data()));
    }
    for (uint32_t fl : {2u, 3u, 0x80000000u}) {
      spt_denoise_params dp = def;
      dp.flags = fl;
      refused(run(p, dp, out.data(), se_out.data()));
    }
    spt_denoise_params dp = def;
    dp.reserved = 1;
    refused(run(p, dp, out.data(), se_out.data()));
    // an output that is an input: refused before anything is written (the inputs keep their bits)
    Planes q = make(3, 2);
    const Planes before = q;
    CHECK(spt_denoise_host(q.rgb.data(), q.se.data(), q.albedo.data(), q.normal.data(), q.depth.data(), 3, 2,
                           &def, q.rgb.data(), nullptr) == SPT_ERR_INVALID_ARG);
    CHECK(spt_denoise_host(q.rgb.data(), q.se.data(), q.albedo.data(), q.normal.data(), q.depth.data(), 3, 2,
                           &def, out.data(), q.normal.data()) == SPT_ERR_INVALID_ARG);
    CHECK(q.rgb == before.rgb && q.normal == before.normal && all_are(out, fill));
  }
  if (g_failed) {
    std::fprintf(stderr, "spt_denoise_check: %d checks failed\n", g_failed);
    return 1;
  }
  std::printf("spt_denoise_check ok\n");
  return 0;
}

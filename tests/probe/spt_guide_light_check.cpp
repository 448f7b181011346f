// spt_guide_light_check.cpp — TEST INFRASTRUCTURE ONLY: a stand-alone host program over the light
// guide's two CPU statements (spt_light_guide_resolve_host and spt_light_shade_host in
// spt_guide_light_host.cpp, with spt_dispatch.cpp for spt_last_error), built with
// -fsanitize=address,undefined by tests/probe/guide_light_check.mk and run by
// tests/test_guide_light_host.py. No HIP, no device, never loaded into Python. Every buffer is a
// std::vector of exactly the size the statement may touch, so a read or write past a plane is a
// sanitizer report. The records are the edges of the header's rule: tested == 0, lit == tested,
// 0 < lit < tested, a weight sum of one sample at the clamp and of spp samples at it; full and partial
// samples_done, n == 0, planes left NULL, a zero-pixel guide and the refused arguments; the shade with
// its floor at both ends of (0, 1], in place, and refused outside.
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

static bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

int main() {
  constexpr int64_t one = (int64_t)1 << 31;
  constexpr int32_t spp = 8;
  const int32_t w = 3, rows = 2;
  std::vector<int64_t> rec = {
      0, 0, 0, 0,              // never tested
      spp, spp, one * spp, 0,  // every sample lit, each at the per-sample clamp: direct = spp
      spp, 3, one / 4 + 1, 0,  // 0 < lit < tested
      3, 0, 0, 0,              // tested, never lit
      1, 1, one, 0,            // one sample of eight
      7, 2, 3, 0,
  };
  CHECK(rec.size() == (size_t)w * rows * 4);
  std::vector<float> v(w * rows), d(w * rows), t(w * rows);
  {  // a full light guide
    const spt_guide_info info{w, rows, spp, spp, 0, 0};
    CHECK(spt_light_guide_resolve_host(rec.data(), &info, v.data(), d.data(), t.data()) == SPT_OK);
    CHECK(same(v[0], 0.0f) && same(d[0], 0.0f) && same(t[0], 0.0f));
    CHECK(same(v[1], 1.0f) && same(d[1], 8.0f) && same(t[1], 1.0f));  // not clamped
    CHECK(same(v[2], 0.375f) && same(d[2], 0.25f) && same(t[2], 1.0f));  // (2^29 + 1 rounds to 2^29)
    CHECK(same(v[3], 0.0f) && same(d[3], 0.0f) && same(t[3], 0.375f));
    CHECK(same(v[4], 1.0f) && same(d[4], 1.0f) && same(t[4], 0.125f));
    CHECK(same(v[5], (float)(2.0 / 7.0)) && same(d[5], 3.0f * 0x1p-31f) && same(t[5], 0.875f));
  }
  {  // a partial one: r = (float)(8.0 / 3.0), one more multiply on direct alone
    const spt_guide_info info{w, rows, spp, 3, 0, 0};
    const float r = (float)(8.0 / 3.0);
    CHECK(spt_light_guide_resolve_host(rec.data(), &info, v.data(), d.data(), t.data()) == SPT_OK);
    CHECK(same(v[2], 0.375f) && same(d[2], 0.25f * r) && same(t[3], 1.0f));
    CHECK(same(d[4], 1.0f * r) && same(t[4], (float)(1.0 / 3.0)));
    // planes left out leave no trace in the others
    std::vector<float> d2(w * rows, -7.0f);
    CHECK(spt_light_guide_resolve_host(rec.data(), &info, nullptr, d2.data(), nullptr) == SPT_OK);
    CHECK(std::memcmp(d2.data(), d.data(), d.size() * 4) == 0);
    std::vector<float> v2(w * rows, -7.0f);
    CHECK(spt_light_guide_resolve_host(rec.data(), &info, v2.data(), nullptr, nullptr) == SPT_OK);
    CHECK(std::memcmp(v2.data(), v.data(), v.size() * 4) == 0);
    CHECK(spt_light_guide_resolve_host(rec.data(), &info, nullptr, nullptr, nullptr) == SPT_OK);
  }
  {  // n == 0: zeros everywhere, whatever the records hold
    const spt_guide_info info{w, rows, spp, 0, 0, 0};
    CHECK(spt_light_guide_resolve_host(rec.data(), &info, v.data(), d.data(), t.data()) == SPT_OK);
    for (int i = 0; i < w * rows; ++i) CHECK(same(v[i], 0.0f) && same(d[i], 0.0f) && same(t[i], 0.0f));
  }
  {  // a zero-pixel light guide (a shard without rows): nothing is read or written
    const spt_guide_info info{w, 0, spp, 5, 0, 0};
    CHECK(spt_light_guide_resolve_host(nullptr, &info, nullptr, nullptr, nullptr) == SPT_OK);
    std::vector<float> none;
    CHECK(spt_light_guide_resolve_host(nullptr, &info, none.data(), none.data(), none.data()) == SPT_OK);
  }
  {  // a 1 x 1 light guide at the largest spp, every sample at the clamp
    const int32_t big = 1 << 24;
    std::vector<int64_t> r1 = {big, big, one * big, 0};
    float v1, d1, t1;
    const spt_guide_info info{1, 1, big, big, 0, 0};
    CHECK(spt_light_guide_resolve_host(r1.data(), &info, &v1, &d1, &t1) == SPT_OK);
    CHECK(same(v1, 1.0f) && same(d1, 0x1p24f) && same(t1, 1.0f));
  }
  {  // refused
    const spt_guide_info over{w, rows, spp, spp + 1, 0, 0}, neg{w, rows, spp, -1, 0, 0};
    const spt_guide_info nospp{w, rows, 0, 0, 0, 0}, ok{w, rows, spp, 1, 0, 0};
    CHECK(spt_light_guide_resolve_host(rec.data(), &over, v.data(), nullptr, nullptr) == SPT_ERR_INVALID_ARG);
    CHECK(spt_light_guide_resolve_host(rec.data(), &neg, v.data(), nullptr, nullptr) == SPT_ERR_INVALID_ARG);
    CHECK(spt_light_guide_resolve_host(rec.data(), &nospp, v.data(), nullptr, nullptr) == SPT_ERR_INVALID_ARG);
    CHECK(spt_light_guide_resolve_host(rec.data(), nullptr, v.data(), nullptr, nullptr) == SPT_ERR_INVALID_ARG);
    CHECK(spt_light_guide_resolve_host(nullptr, &ok, v.data(), nullptr, nullptr) == SPT_ERR_INVALID_ARG);
    CHECK(std::strlen(spt_last_error()) > 0);
  }
  {  // the shade: m = f + (1 - f) * vis, a multiply then an add; out_k = albedo_k * m
    const std::vector<float> vis = {0.0f, 1.0f, 0.375f, (float)(2.0 / 7.0)};
    const std::vector<float> alb = {0.75f, 0.25f, 1.0f, 0.75f, 0.25f, 1.0f, 0.5f, 0.0f, 0.999f, 0.1f, 0.2f, 0.3f};
    std::vector<float> out(alb.size(), -7.0f);
    CHECK(spt_light_shade_host(alb.data(), vis.data(), 4, 0.25f, out.data()) == SPT_OK);
    CHECK(same(out[0], 0.75f * 0.25f) && same(out[2], 0.25f));   // vis 0: the floor
    CHECK(same(out[3], 0.75f) && same(out[5], 1.0f));            // vis 1: 0.25 + 0.75 = 1
    const float m2 = 0.25f + 0.75f * 0.375f;
    CHECK(same(out[6], 0.5f * m2) && same(out[7], 0.0f) && same(out[8], 0.999f * m2));
    volatile float prod = 0.75f * vis[3];
    const float m3 = 0.25f + prod;
    CHECK(same(out[9], 0.1f * m3) && same(out[11], 0.3f * m3));
    // floor 1: the albedo itself; in place
    std::vector<float> io = alb;
    CHECK(spt_light_shade_host(io.data(), vis.data(), 4, 1.0f, io.data()) == SPT_OK);
    CHECK(std::memcmp(io.data(), alb.data(), alb.size() * 4) == 0);
    CHECK(spt_light_shade_host(io.data(), vis.data(), 4, 0.25f, io.data()) == SPT_OK);
    CHECK(std::memcmp(io.data(), out.data(), out.size() * 4) == 0);
    // the smallest floor
    CHECK(spt_light_shade_host(alb.data(), vis.data(), 4, std::numeric_limits<float>::denorm_min(), out.data()) == SPT_OK);
    CHECK(same(out[3], 0.75f));
    // nothing to do, nothing touched
    CHECK(spt_light_shade_host(nullptr, nullptr, 0, 0.25f, nullptr) == SPT_OK);
    // refused: the floor outside (0, 1] or not finite, a negative count, a null plane
    std::vector<float> keep(alb.size(), -7.0f);
    const float bad[] = {0.0f, -0.0f, -0.25f, 1.0000001f, 2.0f, std::numeric_limits<float>::infinity(),
                         -std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN()};
    for (float f : bad) CHECK(spt_light_shade_host(alb.data(), vis.data(), 4, f, keep.data()) == SPT_ERR_INVALID_ARG);
    CHECK(spt_light_shade_host(alb.data(), vis.data(), -1, 0.25f, keep.data()) == SPT_ERR_INVALID_ARG);
    CHECK(spt_light_shade_host(nullptr, vis.data(), 4, 0.25f, keep.data()) == SPT_ERR_INVALID_ARG);
    CHECK(spt_light_shade_host(alb.data(), nullptr, 4, 0.25f, keep.data()) == SPT_ERR_INVALID_ARG);
    CHECK(spt_light_shade_host(alb.data(), vis.data(), 4, 0.25f, nullptr) == SPT_ERR_INVALID_ARG);
    for (float x : keep) CHECK(same(x, -7.0f));
  }
  if (g_failed) {
    std::fprintf(stderr, "spt_guide_light_check: %d checks failed\n", g_failed);
    return 1;
  }
  std::printf("spt_guide_light_check ok\n");
  return 0;
}

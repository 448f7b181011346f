// spt_guide_check.cpp — TEST INFRASTRUCTURE ONLY: a stand-alone host program over the guide's CPU
// resolve (spt_guide_resolve_host in spt_guide_host.cpp, with spt_dispatch.cpp for spt_last_error),
// built with -fsanitize=address,undefined by tests/probe/guide_check.mk and run by
// tests/test_guide_host.py. No HIP, no device, never loaded into Python. Every buffer is a
// std::vector of exactly the size the statement may touch, so a read or write past a plane is a
// sanitizer report. The records are the edges of the header's rule: hits == 0, 0 < hits < n,
// negative normal sums (INT64_MIN's neighbour included), albedo sums at and above the clamp, the
// largest depth; full and partial samples_done, n == 0, planes left NULL, a zero-pixel guide, and
// the refused arguments.
#include <cmath>
#include <cstdint>
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

static bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

int main() {
  static_assert(sizeof(spt_guide_info) == 32, "spt_guide_info");
  CHECK(spt_guide_info_size() == 32);
  constexpr int64_t one = (int64_t)1 << 31;
  constexpr int32_t spp = 8;
  const int32_t w = 3, rows = 2;
  std::vector<int64_t> rec = {
      0, 0, 0, 0, 0, 0, 0, 0,                                                   // never hit
      one, one / 2, one * 3, -one, one / 4, -1, ((int64_t)1 << 36) * spp, spp,  // the clamp; 2^20 deep
      one + 1, 1, 0, one, -(one - 1), 0, 65536 * 3 + 1, 3,                      // 0 < hits < n
      one * spp, 0, 0, INT64_MIN + 1, INT64_MAX, 0, 1, 1,                       // far above the clamp
      0, 0, 0, 0, 0, 0, 0, 0,
      one / 8, one / 8, one / 8, -one / 8, -one / 8, -one / 8, 65536, 1,
  };
  CHECK(rec.size() == (size_t)w * rows * 8);
  std::vector<float> a(3 * w * rows), n(3 * w * rows), d(w * rows), c(w * rows);
  {  // a full guide
    const spt_guide_info info{w, rows, spp, spp, 0, 0};
    CHECK(spt_guide_resolve_host(rec.data(), &info, a.data(), n.data(), d.data(), c.data()) == SPT_OK);
    for (int k = 0; k < 3; ++k) CHECK(same(a[k], 0.0f) && same(n[k], 0.0f));
    CHECK(same(d[0], 0.0f) && same(c[0], 0.0f));
    CHECK(same(a[3], 1.0f) && same(a[4], 0.5f) && same(a[5], 1.0f));  // 2^31 is exactly 1; 3 clamps
    CHECK(same(n[3], -1.0f) && same(n[4], 0.25f) && same(n[5], -0x1p-31f));
    CHECK(same(d[1], 0x1p20f) && same(c[1], 1.0f));
    CHECK(same(a[6], 1.0f));  // (float)(2^31 + 1) * 2^-31 rounds to 1
    CHECK(same(n[6], 1.0f) && same(n[7], -1.0f) && same(n[8], 0.0f));  // (2^31 - 1 rounds to 2^31)
    CHECK(same(d[2], (float)((double)(65536 * 3 + 1) / (3.0 * 65536.0))) && same(c[2], 0.375f));
    CHECK(same(a[9], 1.0f) && same(n[9], -0x1p32f) && same(n[10], 0x1p32f));  // unclamped normals
    CHECK(same(d[3], (float)(1.0 / 65536.0)) && same(c[3], 0.125f));
    CHECK(same(a[15], 0.125f) && same(n[15], -0.125f) && same(d[5], 1.0f));
  }
  {  // a partial guide: two separate multiplies, r = (float)(8.0 / 3.0)
    const spt_guide_info info{w, rows, spp, 3, 0, 0};
    const float r = (float)(8.0 / 3.0);
    CHECK(spt_guide_resolve_host(rec.data(), &info, a.data(), n.data(), d.data(), c.data()) == SPT_OK);
    CHECK(same(a[15], 0.125f * r) && same(n[15], -(0.125f * r)) && same(a[4], 1.0f));
    CHECK(same(n[4], 0.25f * r) && same(c[5], (float)(1.0 / 3.0)) && same(d[5], 1.0f));
    // planes left out leave no trace in the others
    std::vector<float> n2(3 * w * rows, -7.0f);
    CHECK(spt_guide_resolve_host(rec.data(), &info, nullptr, n2.data(), nullptr, nullptr) == SPT_OK);
    CHECK(std::memcmp(n2.data(), n.data(), n.size() * 4) == 0);
    std::vector<float> c2(w * rows, -7.0f);
    CHECK(spt_guide_resolve_host(rec.data(), &info, nullptr, nullptr, nullptr, c2.data()) == SPT_OK);
    CHECK(std::memcmp(c2.data(), c.data(), c.size() * 4) == 0);
  }
  {  // n == 0: zeros everywhere, whatever the records hold
    const spt_guide_info info{w, rows, spp, 0, 0, 0};
    CHECK(spt_guide_resolve_host(rec.data(), &info, a.data(), n.data(), d.data(), c.data()) == SPT_OK);
    for (float v : a) CHECK(same(v, 0.0f));
    for (float v : n) CHECK(same(v, 0.0f));
    for (float v : d) CHECK(same(v, 0.0f));
    for (float v : c) CHECK(same(v, 0.0f));
  }
  {  // a zero-pixel guide (a shard without rows): nothing is read or written
    const spt_guide_info info{w, 0, spp, 5, 0, 0};
    CHECK(spt_guide_resolve_host(nullptr, &info, nullptr, nullptr, nullptr, nullptr) == SPT_OK);
    std::vector<float> none;
    CHECK(spt_guide_resolve_host(nullptr, &info, none.data(), none.data(), none.data(), none.data()) == SPT_OK);
    const spt_guide_info info2{0, 4, spp, 5, 0, 0};
    CHECK(spt_guide_resolve_host(nullptr, &info2, nullptr, nullptr, nullptr, nullptr) == SPT_OK);
  }
  {  // a 1 x 1 guide at the largest spp
    const int32_t big = 1 << 24;
    std::vector<int64_t> r1 = {one, 0, 0, 0, 0, -one, ((int64_t)1 << 36) * big, big};
    std::vector<float> a1(3), n1(3), d1(1), c1(1);
    const spt_guide_info info{1, 1, big, big, 0, 0};
    CHECK(spt_guide_resolve_host(r1.data(), &info, a1.data(), n1.data(), d1.data(), c1.data()) == SPT_OK);
    CHECK(same(a1[0], 1.0f) && same(n1[2], -1.0f) && same(d1[0], 0x1p20f) && same(c1[0], 1.0f));
  }
  {  // refused
    const spt_guide_info over{w, rows, spp, spp + 1, 0, 0}, neg{w, rows, spp, -1, 0, 0};
    const spt_guide_info nospp{w, rows, 0, 0, 0, 0}, ok{w, rows, spp, 1, 0, 0};
    CHECK(spt_guide_resolve_host(rec.data(), &over, a.data(), nullptr, nullptr, nullptr) == SPT_ERR_INVALID_ARG);
    CHECK(spt_guide_resolve_host(rec.data(), &neg, a.data(), nullptr, nullptr, nullptr) == SPT_ERR_INVALID_ARG);
    CHECK(spt_guide_resolve_host(rec.data(), &nospp, a.data(), nullptr, nullptr, nullptr) == SPT_ERR_INVALID_ARG);
    CHECK(spt_guide_resolve_host(rec.data(), nullptr, a.data(), nullptr, nullptr, nullptr) == SPT_ERR_INVALID_ARG);
    CHECK(spt_guide_resolve_host(nullptr, &ok, a.data(), nullptr, nullptr, nullptr) == SPT_ERR_INVALID_ARG);
    CHECK(std::strlen(spt_last_error()) > 0);
  }
  if (g_failed) {
    std::fprintf(stderr, "spt_guide_check: %d checks failed\n", g_failed);
    return 1;
  }
  std::printf("spt_guide_check ok\n");
  return 0;
}

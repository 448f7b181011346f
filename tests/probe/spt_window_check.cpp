// spt_window_check.cpp — TEST INFRASTRUCTURE ONLY: a stand-alone host program over what a film and a
// guide share (spt_window_shape.h, with spt_dispatch.cpp for spt::fail / spt_last_error and
// spt_host.cpp for the shard's rows), built with -fsanitize=address,undefined by
// tests/probe/window_check.mk and run by tests/test_window_shape_host.py. No HIP, no device, never
// loaded into Python.
//   * shape_from_params: the smallest image, a shard without rows, tile_rows 0 read as 8, and every
//     rejection with its exact text, the two pixel caps (2^32 - 1 and 2^31 - 1) at and one above;
//   * shape_accepts, for both nouns: each of the four messages from the smallest change that trips
//     it, and the earlier message when a call trips two checks;
//   * shape_equal.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../small-pathtracer_amd/csrc/spt_window_shape.h"

using namespace spt;

static int g_failed = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s (last error: %s)\n", __FILE__, __LINE__, #cond, \
                   spt_last_error());                                        \
      ++g_failed;                                                            \
    }                                                                        \
  } while (0)

static spt_params params(int32_t w, int32_t h, int32_t spp) {
  spt_params p;
  CHECK(spt_default_params(&p) == SPT_OK);
  p.width = w;
  p.height = h;
  p.spp = spp;
  return p;
}

static bool rejected(spt_status st, const std::string& text) {
  return st == SPT_ERR_INVALID_ARG && text == spt_last_error();
}

constexpr uint64_t kFilmCap = 0xFFFFFFFFull, kGuideCap = 0x7FFFFFFFull;

static void from_params() {
  const char* positive = "width/height/spp must be positive";
  const char* large = "image too large for 32-bit pixel counters";
  const char* shard = "bad shard_index/shard_count/tile_rows";
  for (uint64_t cap : {kFilmCap, kGuideCap}) {
    WindowShape s;
    s.samples_done = 5;
    spt_params p = params(1, 1, 1);
    CHECK(shape_from_params(&p, cap, &s) == SPT_OK);
    CHECK(s.width == 1 && s.height == 1 && s.rows == 1 && s.spp_total == 1 && s.tile_rows == 8);
    CHECK(s.shard_index == 0 && s.shard_count == 1 && s.samples_done == 0);

    p = params(5, 8, 2);  // one row tile, two shards: the second owns no rows
    p.shard_count = 2;
    p.shard_index = 1;
    CHECK(shape_from_params(&p, cap, &s) == SPT_OK);
    CHECK(s.rows == 0 && s.shard_index == 1 && s.shard_count == 2 && s.height == 8);
    p.shard_index = 0;
    CHECK(shape_from_params(&p, cap, &s) == SPT_OK && s.rows == 8);

    p = params(5, 9, 2);
    p.tile_rows = 0;  // read as 8: rows 0-7 are shard 0's, row 8 is shard 1's
    p.shard_count = 2;
    CHECK(shape_from_params(&p, cap, &s) == SPT_OK && s.tile_rows == 8 && s.rows == 8);
    p.tile_rows = 3;
    CHECK(shape_from_params(&p, cap, &s) == SPT_OK && s.tile_rows == 3 && s.rows == 6);

    for (int32_t bad : {0, -1}) {
      p = params(bad, 1, 1);
      CHECK(rejected(shape_from_params(&p, cap, &s), positive));
      p = params(1, bad, 1);
      CHECK(rejected(shape_from_params(&p, cap, &s), positive));
      p = params(1, 1, bad);
      CHECK(rejected(shape_from_params(&p, cap, &s), positive));
    }
    p = params(1, 1, 1);
    p.shard_count = 3;
    p.shard_index = 3;
    CHECK(rejected(shape_from_params(&p, cap, &s), shard));
    p.shard_index = -1;
    CHECK(rejected(shape_from_params(&p, cap, &s), shard));
    p.shard_index = 0;
    p.shard_count = 0;
    CHECK(rejected(shape_from_params(&p, cap, &s), shard));
    p = params(1, 1, 1);
    p.tile_rows = -1;
    CHECK(rejected(shape_from_params(&p, cap, &s), shard));
    // a call tripping two checks gets the earlier message
    p = params(0, 1, 1);
    p.tile_rows = -1;
    CHECK(rejected(shape_from_params(&p, cap, &s), positive));
    p = params(65536, 65536, 1);
    p.tile_rows = -1;
    CHECK(rejected(shape_from_params(&p, cap, &s), large));
  }
  WindowShape s;
  // 2^32 - 1 = 65535 * 65537 is the film's cap; 2^32 is one above
  spt_params p = params(65535, 65537, 1);
  CHECK(shape_from_params(&p, kFilmCap, &s) == SPT_OK && s.width == 65535 && s.rows == 65537);
  CHECK(rejected(shape_from_params(&p, kGuideCap, &s), large));
  p = params(65536, 65536, 1);
  CHECK(rejected(shape_from_params(&p, kFilmCap, &s), large));
  // 2^31 - 1 is prime: one row of that many pixels is the guide's cap; 2^31 = 32768 * 65536 is above
  p = params(0x7FFFFFFF, 1, 1);
  CHECK(shape_from_params(&p, kGuideCap, &s) == SPT_OK && s.width == 0x7FFFFFFF && s.rows == 1);
  p = params(32768, 65536, 1);
  CHECK(rejected(shape_from_params(&p, kGuideCap, &s), large));
  CHECK(shape_from_params(&p, kFilmCap, &s) == SPT_OK);
}

static void accepts(const std::string& noun) {
  const std::string differ = "width/height/spp differ from the " + noun + "'s";
  const std::string shard = "the shard fields differ from the " + noun + "'s";
  const std::string window = "sample window outside [0, spp)";
  const std::string more = "the " + noun + " would hold more than spp samples";
  const char* n = noun.c_str();
  spt_params p0 = params(4, 24, 8);
  p0.tile_rows = 0;
  p0.shard_count = 2;
  p0.shard_index = 1;
  WindowShape s;
  CHECK(shape_from_params(&p0, kGuideCap, &s) == SPT_OK && s.tile_rows == 8 && s.rows == 8);

  CHECK(shape_accepts(s, &p0, 0, 8, n) == SPT_OK);
  CHECK(shape_accepts(s, &p0, 7, 1, n) == SPT_OK);
  spt_params p = p0;
  p.tile_rows = 8;  // 8 against the 0 it was created with: the same tiles
  CHECK(shape_accepts(s, &p, 0, 8, n) == SPT_OK);

  p = p0; p.width += 1;
  CHECK(rejected(shape_accepts(s, &p, 0, 8, n), differ));
  p = p0; p.height += 1;
  CHECK(rejected(shape_accepts(s, &p, 0, 8, n), differ));
  p = p0; p.spp += 1;
  CHECK(rejected(shape_accepts(s, &p, 0, 8, n), differ));

  p = p0; p.tile_rows = 4;
  CHECK(rejected(shape_accepts(s, &p, 0, 8, n), shard));
  p = p0; p.tile_rows = -8;
  CHECK(rejected(shape_accepts(s, &p, 0, 8, n), shard));
  p = p0; p.shard_index = 0;
  CHECK(rejected(shape_accepts(s, &p, 0, 8, n), shard));
  p = p0; p.shard_count = 3;
  CHECK(rejected(shape_accepts(s, &p, 0, 8, n), shard));

  CHECK(rejected(shape_accepts(s, &p0, -1, 1, n), window));
  CHECK(rejected(shape_accepts(s, &p0, 1, 8, n), window));  // base + count = spp + 1
  CHECK(rejected(shape_accepts(s, &p0, 0, 0, n), window));
  CHECK(rejected(shape_accepts(s, &p0, 0x7FFFFFFF, 0x7FFFFFFF, n), window));  // no 32-bit wrap

  s.samples_done = 1;  // the window itself is in range; the plane would hold spp + 1
  CHECK(rejected(shape_accepts(s, &p0, 0, 8, n), more));
  CHECK(shape_accepts(s, &p0, 0, 7, n) == SPT_OK);
  CHECK(shape_accepts(s, &p0, 1, 7, n) == SPT_OK);
  s.samples_done = 8;
  CHECK(rejected(shape_accepts(s, &p0, 0, 1, n), more));

  // a call tripping two checks gets the earlier message
  s.samples_done = 1;
  p = p0; p.width += 1; p.tile_rows = 4;
  CHECK(rejected(shape_accepts(s, &p, -1, 1, n), differ));
  p = p0; p.tile_rows = 4;
  CHECK(rejected(shape_accepts(s, &p, -1, 1, n), shard));
  CHECK(rejected(shape_accepts(s, &p0, 1, 8, n), window));  // outside, and more than spp
}

static void equal() {
  WindowShape a, b;
  spt_params p = params(6, 5, 64), q = params(6, 5, 8);
  CHECK(shape_from_params(&p, kFilmCap, &a) == SPT_OK && shape_from_params(&q, kGuideCap, &b) == SPT_OK);
  b.samples_done = 8;
  CHECK(shape_equal(a, b) && shape_equal(b, a));  // a 64-spp film and its 8-spp guide
  q.width = 5;
  CHECK(shape_from_params(&q, kGuideCap, &b) == SPT_OK && !shape_equal(a, b));
  q = params(6, 6, 8);
  CHECK(shape_from_params(&q, kGuideCap, &b) == SPT_OK && !shape_equal(a, b));
  q = params(6, 10, 64);  // the same pixels by another route: one of two five-row tiles
  q.tile_rows = 5;
  q.shard_count = 2;
  CHECK(shape_from_params(&q, kGuideCap, &b) == SPT_OK && b.rows == 5 && shape_equal(a, b));
}

int main() {
  from_params();
  accepts("film");
  accepts("guide");
  equal();
  if (g_failed) {
    std::fprintf(stderr, "spt_window_check: %d checks failed\n", g_failed);
    return 1;
  }
  std::puts("spt_window_check ok");
  return 0;
}

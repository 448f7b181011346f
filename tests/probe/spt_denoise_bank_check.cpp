// spt_denoise_bank_check.cpp — TEST INFRASTRUCTURE ONLY: a stand-alone host program over the filter bank's
// CPU statement and its summary (spt_denoise_bank_host, spt_denoise_bank_summary_host in
// spt_denoise_host.cpp, with spt_dispatch.cpp for spt_last_error), built with
// -fsanitize=address,undefined by tests/probe/denoise_bank_check.mk and run by
// tests/test_denoise_bank_host.py. No HIP, no device, never loaded into Python. Every buffer is a
// std::vector of exactly the size the statement may touch, so a read or write past a plane is a
// sanitizer report: the small images at the smoothing's step 4 and the filter's step 32 are where an
// unclipped tap address would be caught. Sizes 1x1, 3x2, 5x1, 1x5 and 17x13; 1, 2 and 4 candidates;
// error_iterations 0..3; both pair_flags; mse and choice left NULL; one candidate against the pair
// filter; swapped halves; inputs that are not finite; every refused argument, with the outputs checked
// for their fill pattern.
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

spt_status run(const Planes& p, const spt_denoise_params* c, int32_t n, const spt_bank_params* b, float* out,
               float* mse, uint8_t* choice) {
  return spt_denoise_bank_host(p.rgb_a.data(), p.se_a.data(), p.rgb_b.data(), p.se_b.data(), p.albedo.data(),
                               p.normal.data(), p.depth.data(), p.w, p.h, c, n, b, out, mse, choice);
}

template <class T>
bool all_are(const std::vector<T>& v, T fill) {
  for (const T& x : v)
    if (std::memcmp(&x, &fill, sizeof(T)) != 0) return false;
  return true;
}

}  // namespace

int main() {
  static_assert(sizeof(spt_bank_params) == 16, "spt_bank_params");
  static_assert(sizeof(spt_bank_summary) == 56, "spt_bank_summary");
  spt_denoise_params def;
  spt_denoise_default_params(&def);
  spt_bank_params bdef;
  std::memset(&bdef, 0xff, sizeof bdef);
  spt_denoise_bank_default_params(&bdef);
  spt_denoise_bank_default_params(nullptr);
  CHECK(bdef.error_iterations == 2 && bdef.pair_flags == SPT_DENOISE_PAIR_OWN_WEIGHTS && bdef.reserved[0] == 0 &&
        bdef.reserved[1] == 0);
  // four candidates: iterations 6 (step 32), 3, 0 and 1 with no demodulation
  spt_denoise_params cands[4] = {def, def, def, def};
  cands[0].iterations = 6;
  cands[0].sigma_color = 2.0f;
  cands[1].iterations = 3;
  cands[1].sigma_color = 8.0f;
  cands[2].iterations = 0;
  cands[3].iterations = 1;
  cands[3].flags = SPT_DENOISE_NO_DEMODULATE;
  const int32_t sizes[5][2] = {{1, 1}, {3, 2}, {5, 1}, {1, 5}, {17, 13}};
  const float fill = -7.25f;
  const uint8_t cfill = 0xA5;
  for (const auto& s : sizes) {
    const Planes p = make(s[0], s[1]);
    Planes swapped = p;
    swapped.rgb_a.swap(swapped.rgb_b);
    swapped.se_a.swap(swapped.se_b);
    const size_t n = p.depth.size(), n3 = 3 * n;
    for (uint32_t pf = 0; pf <= 1; ++pf)
      for (int32_t nc : {1, 2, 4})
        for (int32_t ei = 0; ei <= 3; ++ei) {
          spt_bank_params b = bdef;
          b.pair_flags = pf;
          b.error_iterations = ei;
          std::vector<float> out(n3, fill), mse(n, fill), out2(n3, fill), mse2(n, fill);
          std::vector<uint8_t> choice(n, cfill), choice2(n, cfill);
          CHECK(run(p, cands, nc, &b, out.data(), mse.data(), choice.data()) == SPT_OK);
          CHECK(run(p, cands, nc, &b, out2.data(), nullptr, nullptr) == SPT_OK);  // the optional planes left out
          CHECK(std::memcmp(out.data(), out2.data(), n3 * 4) == 0);
          CHECK(run(p, cands, nc, &b, out2.data(), mse2.data(), nullptr) == SPT_OK);
          CHECK(std::memcmp(mse.data(), mse2.data(), n * 4) == 0);
          for (size_t k = 0; k < n3; ++k)
            CHECK(std::isfinite(out[k]) && out[k] <= 1.0f && std::fabs(out[k] - p.rgb_a[k]) < 0.15f);
          for (size_t k = 0; k < n; ++k) CHECK(std::isfinite(mse[k]) && std::fabs(mse[k]) < 0.1f && choice[k] < nc);
          // swapped halves: every output keeps its bits
          CHECK(run(swapped, cands, nc, &b, out2.data(), mse2.data(), choice2.data()) == SPT_OK);
          CHECK(std::memcmp(out.data(), out2.data(), n3 * 4) == 0);
          CHECK(std::memcmp(mse.data(), mse2.data(), n * 4) == 0);
          CHECK(choice == choice2);
          if (nc == 1) {  // one candidate: the pair filter's out, choice 0
            std::vector<float> pair(n3, fill);
            CHECK(spt_denoise_pair_host(p.rgb_a.data(), p.se_a.data(), p.rgb_b.data(), p.se_b.data(),
                                        p.albedo.data(), p.normal.data(), p.depth.data(), p.w, p.h, cands, pf,
                                        pair.data(), nullptr, nullptr) == SPT_OK);
            CHECK(std::memcmp(out.data(), pair.data(), n3 * 4) == 0);
            CHECK(all_are(choice, (uint8_t)0));
          }
          // the summary of these planes against a plain loop
          spt_bank_summary sm;
          std::memset(&sm, 0xff, sizeof sm);
          CHECK(spt_denoise_bank_summary_host(mse.data(), choice.data(), p.w, p.h, &sm) == SPT_OK);
          double sum = 0.0, cnt[4] = {0, 0, 0, 0};
          float mn = mse[0], mx = mse[0];
          for (size_t k = 0; k < n; ++k) {
            sum += (double)mse[k];
            cnt[choice[k]] += 1.0;
            mn = std::fmin(mn, mse[k]);
            mx = std::fmax(mx, mse[k]);
          }
          CHECK(sm.mse_mean == sum / (double)n);
          CHECK(sm.rmse_est == std::sqrt(sm.mse_mean > 0.0 ? sm.mse_mean : 0.0));
          for (int k = 0; k < 4; ++k) CHECK(sm.share[k] == cnt[k] / (double)n);
          CHECK(sm.mse_min == mn && sm.mse_max == mx);
        }
  }
  {  // inputs that are not finite: unspecified values, no fault, choice below n_cands
    Planes p = make(17, 13);
    p.rgb_a[5] = std::numeric_limits<float>::quiet_NaN();
    p.rgb_b[11] = std::numeric_limits<float>::infinity();
    p.se_a[40] = std::numeric_limits<float>::infinity();
    p.se_b[41] = std::numeric_limits<float>::quiet_NaN();
    p.depth[7] = -std::numeric_limits<float>::infinity();
    p.normal[100] = std::numeric_limits<float>::quiet_NaN();
    p.albedo[200] = -1e30f;
    const size_t n = p.depth.size();
    std::vector<float> out(3 * n, fill), mse(n, fill);
    std::vector<uint8_t> choice(n, cfill);
    for (uint32_t pf = 0; pf <= 1; ++pf) {
      spt_bank_params b = bdef;
      b.pair_flags = pf;
      b.error_iterations = 3;
      CHECK(run(p, cands, 4, &b, out.data(), mse.data(), choice.data()) == SPT_OK);
      for (uint8_t c : choice) CHECK(c < 4);
    }
    spt_bank_summary sm;
    CHECK(spt_denoise_bank_summary_host(mse.data(), choice.data(), 17, 13, &sm) == SPT_OK);
    choice[3] = 200;  // a choice that names no candidate counts for no share
    CHECK(spt_denoise_bank_summary_host(mse.data(), choice.data(), 17, 13, &sm) == SPT_OK);
    CHECK(((sm.share[0] + sm.share[1]) + sm.share[2]) + sm.share[3] < 1.0);
  }
  {  // the refusals: SPT_ERR_INVALID_ARG, a message, the outputs untouched
    const Planes p = make(3, 2);
    const size_t n = p.depth.size(), n3 = 3 * n;
    std::vector<float> out(n3, fill), mse(n, fill);
    std::vector<uint8_t> choice(n, cfill);
    auto refused = [&](spt_status st) {
      CHECK(st == SPT_ERR_INVALID_ARG);
      CHECK(spt_last_error()[0] != 0);
      CHECK(all_are(out, fill) && all_are(mse, fill) && all_are(choice, cfill));
    };
    const float* in[7] = {p.rgb_a.data(), p.se_a.data(), p.rgb_b.data(), p.se_b.data(),
                          p.albedo.data(), p.normal.data(), p.depth.data()};
    auto call = [&](const float* const a[7], int32_t w, int32_t h, const spt_denoise_params* c, int32_t nc,
                    const spt_bank_params* b, float* o, float* m, uint8_t* ch) {
      return spt_denoise_bank_host(a[0], a[1], a[2], a[3], a[4], a[5], a[6], w, h, c, nc, b, o, m, ch);
    };
    for (int k = 0; k < 7; ++k) {
      const float* a[7] = {in[0], in[1], in[2], in[3], in[4], in[5], in[6]};
      a[k] = nullptr;
      refused(call(a, 3, 2, cands, 2, &bdef, out.data(), mse.data(), choice.data()));
    }
    refused(call(in, 3, 2, nullptr, 2, &bdef, out.data(), mse.data(), choice.data()));
    refused(call(in, 3, 2, cands, 2, nullptr, out.data(), mse.data(), choice.data()));
    refused(call(in, 3, 2, cands, 2, &bdef, nullptr, mse.data(), choice.data()));
    refused(call(in, 3, 2, cands, 2, &bdef, out.data(), out.data(), choice.data()));
    refused(call(in, 3, 2, cands, 2, &bdef, out.data(), mse.data(), (uint8_t*)out.data()));
    refused(call(in, 3, 2, cands, 2, &bdef, out.data(), mse.data(), (uint8_t*)mse.data()));
    for (int32_t nc : {0, -1, 5, INT32_MAX, INT32_MIN})
      refused(call(in, 3, 2, cands, nc, &bdef, out.data(), mse.data(), choice.data()));
    for (int32_t ei : {-1, 4, INT32_MAX, INT32_MIN}) {
      spt_bank_params b = bdef;
      b.error_iterations = ei;
      refused(run(p, cands, 2, &b, out.data(), mse.data(), choice.data()));
    }
    for (uint32_t pf : {2u, 3u, 0x80000000u, 0xFFFFFFFFu}) {
      spt_bank_params b = bdef;
      b.pair_flags = pf;
      refused(run(p, cands, 2, &b, out.data(), mse.data(), choice.data()));
    }
    for (int r = 0; r < 2; ++r) {
      spt_bank_params b = bdef;
      b.reserved[r] = 1;
      refused(run(p, cands, 2, &b, out.data(), mse.data(), choice.data()));
    }
    const int32_t dims[5][2] = {{0, 2}, {3, 0}, {-3, 2}, {3, -2}, {65536, 32768}};
    for (const auto& d : dims) refused(call(in, d[0], d[1], cands, 2, &bdef, out.data(), mse.data(), choice.data()));
    // a bad candidate in every place of the list
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    for (int place = 0; place < 4; ++place) {
      for (int field = 0; field < 4; ++field)
        for (float bad : {0.0f, -1.0f, nan, inf, -inf}) {
          spt_denoise_params c[4] = {def, def, def, def};
          (field == 0 ? c[place].sigma_color : field == 1 ? c[place].sigma_depth : field == 2 ? c[place].sigma_albedo
                                                                                            : c[place].albedo_floor) = bad;
          refused(run(p, c, 4, &bdef, out.data(), mse.data(), choice.data()));
        }
      for (int32_t it : {-1, 7, INT32_MAX, INT32_MIN}) {
        spt_denoise_params c[4] = {def, def, def, def};
        c[place].iterations = it;
        refused(run(p, c, 4, &bdef, out.data(), mse.data(), choice.data()));
        c[place] = def;
        c[place].normal_squarings = it == 7 ? 9 : it;
        refused(run(p, c, 4, &bdef, out.data(), mse.data(), choice.data()));
      }
      spt_denoise_params c[4] = {def, def, def, def};
      c[place].flags = 2u;
      refused(run(p, c, 4, &bdef, out.data(), mse.data(), choice.data()));
      c[place] = def;
      c[place].reserved = 1;
      refused(run(p, c, 4, &bdef, out.data(), mse.data(), choice.data()));
      if (place > 0) CHECK(run(p, c, place, &bdef, out.data(), mse.data(), choice.data()) == SPT_OK);  // not read
      std::fill(out.begin(), out.end(), fill);
      std::fill(mse.begin(), mse.end(), fill);
      std::fill(choice.begin(), choice.end(), cfill);
    }
    // an output that is an input: refused before anything is written (the inputs keep their bits)
    Planes q = make(3, 2);
    const Planes before = q;
    float* planes6[6] = {q.rgb_a.data(), q.se_a.data(), q.rgb_b.data(), q.se_b.data(), q.albedo.data(),
                         q.normal.data()};
    for (float* pl : planes6) {
      CHECK(run(q, cands, 2, &bdef, pl, nullptr, nullptr) == SPT_ERR_INVALID_ARG);
      CHECK(run(q, cands, 2, &bdef, out.data(), pl, nullptr) == SPT_ERR_INVALID_ARG);
      CHECK(run(q, cands, 2, &bdef, out.data(), nullptr, (uint8_t*)pl) == SPT_ERR_INVALID_ARG);
    }
    CHECK(q.rgb_a == before.rgb_a && q.se_a == before.se_a && q.rgb_b == before.rgb_b && q.se_b == before.se_b &&
          q.albedo == before.albedo && q.normal == before.normal && all_are(out, fill));
    // the summary's refusals leave *out untouched
    spt_bank_summary sm;
    std::memset(&sm, 0x5a, sizeof sm);
    const spt_bank_summary keep = sm;
    CHECK(spt_denoise_bank_summary_host(nullptr, choice.data(), 3, 2, &sm) == SPT_ERR_INVALID_ARG);
    CHECK(spt_denoise_bank_summary_host(mse.data(), nullptr, 3, 2, &sm) == SPT_ERR_INVALID_ARG);
    CHECK(spt_denoise_bank_summary_host(mse.data(), choice.data(), 3, 2, nullptr) == SPT_ERR_INVALID_ARG);
    for (const auto& d : dims)
      CHECK(spt_denoise_bank_summary_host(mse.data(), choice.data(), d[0], d[1], &sm) == SPT_ERR_INVALID_ARG);
    CHECK(std::memcmp(&sm, &keep, sizeof sm) == 0);
  }
  if (g_failed) {
    std::fprintf(stderr, "spt_denoise_bank_check: %d checks failed\n", g_failed);
    return 1;
  }
  std::printf("spt_denoise_bank_check ok\n");
  return 0;
}

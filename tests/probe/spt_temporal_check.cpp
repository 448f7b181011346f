// spt_temporal_check.cpp — TEST INFRASTRUCTURE ONLY: a stand-alone host program over temporal
// accumulation's CPU statement (spt_temporal_accumulate_host in spt_temporal_host.cpp, with
// spt_dispatch.cpp for spt_last_error), built with -fsanitize=address,undefined by
// tests/probe/temporal_check.mk and run by tests/test_temporal_host.py. No HIP, no device, never loaded
// into Python. Every plane is a std::vector of exactly its size, so a tap address that was formed before
// its range check is a sanitizer report. Sizes 1x1, 3x2, 5x1, 1x5, 17x13 and 40x56: a first frame, the
// same camera again, a moved camera, a camera behind the previous one and one far to the side; both flag
// values; the optional planes left NULL; inputs and a previous state that are not finite; every refused
// argument, with the outputs checked for their fill pattern.
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

const float kFill = -7.25f;

uint32_t g_state = 12345u;
float rnd() {  // [0, 1)
  g_state = g_state * 1664525u + 1013904223u;
  return (float)(g_state >> 8) * 0x1p-24f;
}

// A camera at (ox, oy, oz) that looks down -z: image plane at distance 1, 0.8 wide, square pixels.
spt_camera camera(int32_t w, int32_t h, double ox, double oy, double oz) {
  const double a = 0.4, b = 0.4 * h / w;
  spt_camera c;
  const double o[3] = {ox, oy, oz}, e[3] = {-a, -b, -1.0}, hor[3] = {2 * a, 0, 0}, ver[3] = {0, 2 * b, 0};
  for (int k = 0; k < 3; ++k) {
    c.origin[k] = o[k];
    c.lower_left_corner[k] = o[k] + e[k];
    c.horizontal[k] = hor[k];
    c.vertical[k] = ver[k];
  }
  return c;
}

struct Planes {
  int32_t w, h;
  std::vector<float> rgb, se, albedo, normal, depth;
};

// What `cam` sees of the wall z = -100 (|x|, |y| <= 30: the corner pixels miss): the pixel-mean rays.
Planes make(int32_t w, int32_t h, const spt_camera& cam) {
  const size_t n = (size_t)w * h;
  Planes p{w, h, std::vector<float>(3 * n), std::vector<float>(3 * n), std::vector<float>(3 * n),
           std::vector<float>(3 * n), std::vector<float>(n)};
  for (int32_t y = 0; y < h; ++y)
    for (int32_t x = 0; x < w; ++x) {
      const size_t i = (size_t)y * w + x;
      double d[3], len = 0;
      for (int k = 0; k < 3; ++k) {
        d[k] = (cam.lower_left_corner[k] - cam.origin[k]) + cam.horizontal[k] / w * x +
               cam.vertical[k] / h * (h - 1 - y);
        len += d[k] * d[k];
      }
      len = std::sqrt(len);
      const double t = (-100.0 - cam.origin[2]) / (d[2] / len);
      const double X = cam.origin[0] + t * d[0] / len, Y = cam.origin[1] + t * d[1] / len;
      const bool hit = t > 0 && std::fabs(X) <= 30 && std::fabs(Y) <= 30;
      p.depth[i] = hit ? (float)t : 0.0f;
      for (int k = 0; k < 3; ++k) {
        p.albedo[3 * i + k] = hit ? 0.7f - 0.2f * k : 0.0f;
        p.normal[3 * i + k] = hit && k == 2 ? 1.0f : 0.0f;
        p.rgb[3 * i + k] = p.albedo[3 * i + k] * 0.6f + 0.05f * (rnd() - 0.5f);
        p.se[3 * i + k] = 0.02f;
      }
    }
  return p;
}

// A state of exactly its size and the struct that points at it.
struct State {
  std::vector<float> c, v, n, X, N;
  explicit State(size_t npix) : c(3 * npix, kFill), v(3 * npix, kFill), n(npix, kFill), X(3 * npix, kFill), N(3 * npix, kFill) {}
  spt_temporal_state view() { return spt_temporal_state{c.data(), v.data(), n.data(), X.data(), N.data()}; }
  bool untouched() const {
    for (const auto* p : {&c, &v, &n, &X, &N})
      for (float x : *p)
        if (std::memcmp(&x, &kFill, 4) != 0) return false;
    return true;
  }
};

struct Outs {
  std::vector<float> rgb, se, n, hist;
  explicit Outs(size_t npix) : rgb(3 * npix, kFill), se(3 * npix, kFill), n(npix, kFill), hist(3 * npix, kFill) {}
  bool untouched() const {
    for (const auto* p : {&rgb, &se, &n, &hist})
      for (float x : *p)
        if (std::memcmp(&x, &kFill, 4) != 0) return false;
    return true;
  }
};

spt_status run(const Planes& p, const spt_camera& cam, const spt_temporal_params& tp, State* prev,
               const spt_camera* prev_cam, Outs& o, State& next, bool optional = true) {
  spt_temporal_state pv{}, nx = next.view();
  if (prev) pv = prev->view();
  return spt_temporal_accumulate_host(p.rgb.data(), p.se.data(), p.albedo.data(), p.normal.data(), p.depth.data(),
                                      p.w, p.h, &cam, &tp, prev ? &pv : nullptr, prev_cam, o.rgb.data(),
                                      o.se.data(), optional ? o.n.data() : nullptr,
                                      optional ? o.hist.data() : nullptr, &nx);
}

}  // namespace

int main() {
  static_assert(sizeof(spt_temporal_params) == 24, "spt_temporal_params");
  static_assert(sizeof(spt_temporal_state) == 40, "spt_temporal_state");
  spt_temporal_params def;
  spt_temporal_default_params(&def);
  CHECK(def.n_max == 32.0f && def.normal_min == 0.9f && def.plane_tol == 0.01f && def.albedo_floor == 0.01f);
  CHECK(def.flags == 0 && def.reserved == 0);
  spt_temporal_default_params(nullptr);  // ignored
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();

  const int32_t sizes[6][2] = {{1, 1}, {3, 2}, {5, 1}, {1, 5}, {17, 13}, {40, 56}};
  for (const auto& s : sizes) {
    const int32_t w = s[0], h = s[1];
    const size_t n = (size_t)w * h;
    const spt_camera cam0 = camera(w, h, 0, 0, 0), cam1 = camera(w, h, 1.3, -0.7, 0.5);
    const spt_camera behind = camera(w, h, 0, 0, -200), far = camera(w, h, 1000, 0, 0);
    const Planes p0 = make(w, h, cam0), p1 = make(w, h, cam1);
    for (uint32_t flags = 0; flags <= 1; ++flags) {
      spt_temporal_params tp = def;
      tp.flags = flags;
      State s1(n), s2(n), s3(n), s4(n);
      Outs o1(n), o2(n), o3(n), o4(n), o5(n);
      CHECK(run(p0, cam0, tp, nullptr, nullptr, o1, s1) == SPT_OK);  // a first frame
      CHECK(run(p0, cam0, tp, &s1, &cam0, o2, s2) == SPT_OK);       // the same camera
      CHECK(run(p1, cam1, tp, &s2, &cam0, o3, s3) == SPT_OK);       // a moved camera
      for (size_t i = 0; i < n; ++i) {
        const bool hit = p0.depth[i] != 0.0f;
        CHECK(o1.n[i] == (hit ? 1.0f : 0.0f) && s1.n[i] == o1.n[i]);
        CHECK(o2.n[i] == (hit ? 2.0f : 0.0f));
        CHECK(o3.n[i] >= 0.0f && o3.n[i] <= 3.0f);
        for (int k = 0; k < 3; ++k) {
          CHECK(std::isfinite(o3.rgb[3 * i + k]) && o3.rgb[3 * i + k] <= 1.0f);
          CHECK(std::isfinite(o3.se[3 * i + k]) && o3.se[3 * i + k] >= 0.0f);
          CHECK(std::memcmp(&s3.N[3 * i + k], &p1.normal[3 * i + k], 4) == 0);
          if (hit) CHECK(o2.se[3 * i + k] < p0.se[3 * i + k]);
        }
      }
      // the optional planes left out: the same outputs and state
      Outs o3b(n);
      State s3b(n);
      CHECK(run(p1, cam1, tp, &s2, &cam0, o3b, s3b, false) == SPT_OK);
      CHECK(o3b.rgb == o3.rgb && o3b.se == o3.se && s3b.c == s3.c && s3b.v == s3.v && s3b.n == s3.n);
      for (float x : o3b.n) CHECK(x == kFill);
      for (float x : o3b.hist) CHECK(x == kFill);
      // behind the previous camera, and every tap outside its image: history refused everywhere
      for (const spt_camera* pc : {&behind, &far}) {
        CHECK(run(p0, cam0, tp, &s3, pc, o4, s4) == SPT_OK);
        CHECK(o4.rgb == o1.rgb && o4.se == o1.se && o4.n == o1.n && o4.hist == p0.rgb);
      }
      // a previous state and inputs that are not finite: unspecified values, no fault
      State wild = s3;
      Planes q = p0;
      for (size_t i = 0; i < n; ++i) {
        const float bad[6] = {nan, inf, -inf, -1e30f, 3e38f, 0.0f};
        wild.X[3 * i + i % 3] = bad[i % 6];
        wild.N[3 * i + (i + 1) % 3] = bad[(i + 1) % 6];
        wild.n[i] = bad[(i + 2) % 6];
        wild.c[3 * i] = bad[(i + 3) % 6];
        if (i % 2) q.depth[i] = bad[i % 6];
        if (i % 3 == 0) q.normal[3 * i + 2] = bad[(i + 4) % 6];
        if (i % 5 == 0) q.albedo[3 * i + 1] = bad[(i + 5) % 6];
        if (i % 7 == 0) q.rgb[3 * i] = q.se[3 * i + 1] = bad[i % 6];
      }
      CHECK(run(q, cam1, tp, &wild, &cam0, o5, s4) == SPT_OK);
      CHECK(run(q, cam0, tp, &wild, &cam0, o5, s4) == SPT_OK);
      // a camera so far away that the float -> int conversion's range checks are what stands in the way
      const spt_camera huge = camera(w, h, -3e9, 2e9, 0);
      CHECK(run(p0, cam0, tp, &s3, &huge, o5, s4) == SPT_OK);
      CHECK(o5.n == o1.n);
    }
  }
  {  // the refusals: SPT_ERR_INVALID_ARG, a message, the outputs and the next state untouched
    const int32_t w = 3, h = 2;
    const size_t n = 6;
    const spt_camera cam = camera(w, h, 0, 0, 0);
    const Planes p = make(w, h, cam);
    State s1(n);
    Outs first(n);
    CHECK(run(p, cam, def, nullptr, nullptr, first, s1) == SPT_OK);
    Outs o(n);
    State next(n);
    auto refused = [&](spt_status st) {
      CHECK(st == SPT_ERR_INVALID_ARG);
      CHECK(spt_last_error()[0] != 0);
      CHECK(o.untouched() && next.untouched());
    };
    const float* in[5] = {p.rgb.data(), p.se.data(), p.albedo.data(), p.normal.data(), p.depth.data()};
    spt_temporal_state pv = s1.view(), nx = next.view();
    auto call = [&](const float* const* a, int32_t ww, int32_t hh, const spt_camera* c, const spt_temporal_params* tp,
                    const spt_temporal_state* prev, const spt_camera* pc, float* r, float* e, float* nn, float* hi,
                    const spt_temporal_state* nxt) {
      return spt_temporal_accumulate_host(a[0], a[1], a[2], a[3], a[4], ww, hh, c, tp, prev, pc, r, e, nn, hi, nxt);
    };
    for (int k = 0; k < 5; ++k) {  // a null input plane
      const float* a[5] = {in[0], in[1], in[2], in[3], in[4]};
      a[k] = nullptr;
      refused(call(a, w, h, &cam, &def, &pv, &cam, o.rgb.data(), o.se.data(), o.n.data(), o.hist.data(), &nx));
    }
    refused(call(in, w, h, nullptr, &def, &pv, &cam, o.rgb.data(), o.se.data(), o.n.data(), o.hist.data(), &nx));
    refused(call(in, w, h, &cam, nullptr, &pv, &cam, o.rgb.data(), o.se.data(), o.n.data(), o.hist.data(), &nx));
    refused(call(in, w, h, &cam, &def, &pv, &cam, nullptr, o.se.data(), o.n.data(), o.hist.data(), &nx));
    refused(call(in, w, h, &cam, &def, &pv, &cam, o.rgb.data(), nullptr, o.n.data(), o.hist.data(), &nx));
    refused(call(in, w, h, &cam, &def, &pv, &cam, o.rgb.data(), o.se.data(), o.n.data(), o.hist.data(), nullptr));
    refused(call(in, w, h, &cam, &def, &pv, nullptr, o.rgb.data(), o.se.data(), o.n.data(), o.hist.data(), &nx));
    refused(call(in, w, h, &cam, &def, nullptr, &cam, o.rgb.data(), o.se.data(), o.n.data(), o.hist.data(), &nx));
    for (int k = 0; k < 5; ++k) {  // a null plane in the next or in the previous state
      spt_temporal_state bad = nx;
      (k == 0 ? bad.c : k == 1 ? bad.v : k == 2 ? bad.n : k == 3 ? bad.X : bad.N) = nullptr;
      refused(call(in, w, h, &cam, &def, &pv, &cam, o.rgb.data(), o.se.data(), o.n.data(), o.hist.data(), &bad));
      bad = pv;
      (k == 0 ? bad.c : k == 1 ? bad.v : k == 2 ? bad.n : k == 3 ? bad.X : bad.N) = nullptr;
      refused(call(in, w, h, &cam, &def, &bad, &cam, o.rgb.data(), o.se.data(), o.n.data(), o.hist.data(), &nx));
    }
    const int32_t dims[5][2] = {{0, 2}, {3, 0}, {-3, 2}, {3, -2}, {65536, 32768}};
    for (const auto& d : dims)
      refused(call(in, d[0], d[1], &cam, &def, &pv, &cam, o.rgb.data(), o.se.data(), o.n.data(), o.hist.data(), &nx));
    auto with = [&](const spt_temporal_params& tp) {
      refused(call(in, w, h, &cam, &tp, &pv, &cam, o.rgb.data(), o.se.data(), o.n.data(), o.hist.data(), &nx));
    };
    for (int field = 0; field < 4; ++field)
      for (float bad : {nan, inf, -inf, -2.0f, field == 0 ? 0.5f : field == 1 ? 1.5f : field == 2 ? -1e-9f : 0.0f}) {
        spt_temporal_params tp = def;
        (field == 0 ? tp.n_max : field == 1 ? tp.normal_min : field == 2 ? tp.plane_tol : tp.albedo_floor) = bad;
        with(tp);
      }
    for (uint32_t fl : {2u, 3u, 0x80000000u}) {
      spt_temporal_params tp = def;
      tp.flags = fl;
      with(tp);
    }
    spt_temporal_params tp = def;
    tp.reserved = 1;
    with(tp);
    // singular cameras, current and previous: no volume, no width, not finite
    spt_camera flat = cam, thin = cam, wild = cam;
    for (int k = 0; k < 3; ++k) {
      flat.vertical[k] = flat.horizontal[k];
      thin.horizontal[k] = 0.0;
    }
    wild.origin[1] = std::numeric_limits<double>::quiet_NaN();
    for (const spt_camera* c : {&flat, &thin, &wild}) {
      refused(call(in, w, h, c, &def, &pv, &cam, o.rgb.data(), o.se.data(), o.n.data(), o.hist.data(), &nx));
      refused(call(in, w, h, &cam, &def, &pv, c, o.rgb.data(), o.se.data(), o.n.data(), o.hist.data(), &nx));
    }
    // an output that is an input, a plane of the previous state, or another output
    refused(call(in, w, h, &cam, &def, &pv, &cam, o.rgb.data(), o.rgb.data(), o.n.data(), o.hist.data(), &nx));
    refused(call(in, w, h, &cam, &def, &pv, &cam, o.rgb.data(), o.se.data(), o.n.data(), o.rgb.data(), &nx));
    refused(call(in, w, h, &cam, &def, &pv, &cam, o.rgb.data(), o.se.data(), next.n.data(), o.hist.data(), &nx));
    {
      spt_temporal_state twice = nx;
      twice.v = twice.c;
      refused(call(in, w, h, &cam, &def, &pv, &cam, o.rgb.data(), o.se.data(), o.n.data(), o.hist.data(), &twice));
    }
    Planes q = p;
    State keep = s1;
    const float* qin[5] = {q.rgb.data(), q.se.data(), q.albedo.data(), q.normal.data(), q.depth.data()};
    refused(call(qin, w, h, &cam, &def, &pv, &cam, q.rgb.data(), o.se.data(), o.n.data(), o.hist.data(), &nx));
    refused(call(qin, w, h, &cam, &def, &pv, &cam, o.rgb.data(), o.se.data(), q.depth.data(), o.hist.data(), &nx));
    refused(call(in, w, h, &cam, &def, &pv, &cam, o.rgb.data(), o.se.data(), o.n.data(), o.hist.data(), &pv));
    refused(call(in, w, h, &cam, &def, &pv, &cam, s1.c.data(), o.se.data(), o.n.data(), o.hist.data(), &nx));
    CHECK(q.rgb == p.rgb && q.depth == p.depth);
    CHECK(s1.c == keep.c && s1.v == keep.v && s1.n == keep.n && s1.X == keep.X && s1.N == keep.N);
  }
  if (g_failed) {
    std::fprintf(stderr, "spt_temporal_check: %d checks failed\n", g_failed);
    return 1;
  }
  std::printf("spt_temporal_check ok\n");
  return 0;
}

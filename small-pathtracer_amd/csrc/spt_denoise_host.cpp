// spt_denoise_host.cpp — the a-trous filter as a pure host function (include/spt.h, SPT_HAS_DENOISE):
// the CPU statement every GPU denoise test compares the device kernels against, and below it the
// two-half filter and its summary (SPT_HAS_DENOISE_PAIR) and the filter bank (SPT_HAS_DENOISE_BANK). Plain
// C++, no HIP: it is also built into tests/probe/spt_denoise_check, spt_denoise_pair_check and
// spt_denoise_bank_check under the host sanitizers.
#include <cstring>
#include <utility>
#include <vector>

#include "spt_denoise.h"
#include "spt_status.h"

static_assert(sizeof(spt_denoise_params) == 32, "spt_denoise_params layout (the Python mirror's)");

extern "C" void spt_denoise_default_params(spt_denoise_params* p) {
  if (!p) return;
  p->iterations = 5;
  p->sigma_color = 4.0f;
  p->sigma_depth = 1.0f;
  p->sigma_albedo = 0.1f;
  p->normal_squarings = 7;
  p->albedo_floor = 0.01f;
  p->flags = 0;
  p->reserved = 0;
}

namespace {

using namespace spt_denoise_math;

struct HostPlanes {
  const f4 *cv_, *nz_, *av_;
  int32_t w;
  f4 cv(int32_t x, int32_t y) const { return cv_[(size_t)y * w + x]; }
  f4 nz(int32_t x, int32_t y) const { return nz_[(size_t)y * w + x]; }
  f4 av(int32_t x, int32_t y) const { return av_[(size_t)y * w + x]; }
  float v(int32_t x, int32_t y) const { return cv_[(size_t)y * w + x].w; }
};

spt_status fail(const char* msg) { return spt::fail(SPT_ERR_INVALID_ARG, std::string("spt_denoise_host: ") + msg); }

}  // namespace

extern "C" spt_status spt_denoise_host(const float* rgb, const float* se, const float* albedo,
                                       const float* normal, const float* depth, int32_t width,
                                       int32_t height, const spt_denoise_params* params, float* out,
                                       float* se_out) {
  if (!rgb || !se || !albedo || !normal || !depth || !out) return fail("null plane");
  if (const char* e = params_error(params)) return fail(e);
  if (width <= 0 || height <= 0 || (int64_t)width * (int64_t)height > kMaxPixels)
    return fail("width/height must be positive and hold at most 2^31 - 1 pixels");
  for (const float* in : {rgb, se, albedo, normal, depth})
    if (out == in || (se_out && se_out == in)) return fail("an output plane is an input plane");
  if (se_out == out) return fail("out and se_out are one plane");
  const size_t npix = (size_t)width * (size_t)height;
  if (params->iterations == 0) {
    std::memcpy(out, rgb, npix * 3 * sizeof(float));
    if (se_out) std::memcpy(se_out, se, npix * 3 * sizeof(float));
    return SPT_OK;
  }
  const Args A = make_args(params);
  std::vector<f4> cv0(npix), cv1(npix), nz(npix), av(npix);
  std::vector<float> gx(npix), gy(npix);
  for (int32_t y = 0; y < height; ++y)
    for (int32_t x = 0; x < width; ++x) {
      const size_t i = (size_t)y * width + x;
      cv0[i] = prepare(rgb + 3 * i, se + 3 * i, albedo + 3 * i, A);
      nz[i] = {normal[3 * i], normal[3 * i + 1], normal[3 * i + 2], depth[i]};
      av[i] = {albedo[3 * i], albedo[3 * i + 1], albedo[3 * i + 2], 0.0f};
      gx[i] = gradient(x, width, x > 0 ? depth[i - 1] : 0.0f, depth[i], x < width - 1 ? depth[i + 1] : 0.0f);
      gy[i] = gradient(y, height, y > 0 ? depth[i - width] : 0.0f, depth[i],
                       y < height - 1 ? depth[i + width] : 0.0f);
    }
  f4 *cur = cv0.data(), *nxt = cv1.data();
  for (int32_t it = 0; it < params->iterations; ++it) {
    const HostPlanes P{cur, nz.data(), av.data(), width};
    for (int32_t y = 0; y < height; ++y)
      for (int32_t x = 0; x < width; ++x) av[(size_t)y * width + x].w = variance_filter(P, x, y, width, height);
    for (int32_t y = 0; y < height; ++y)
      for (int32_t x = 0; x < width; ++x) {
        const size_t i = (size_t)y * width + x;
        nxt[i] = iterate(P, x, y, width, height, (int32_t)1 << it, gx[i], gy[i], A);
      }
    f4* t = cur;
    cur = nxt;
    nxt = t;
  }
  for (size_t i = 0; i < npix; ++i) finish(cur[i], av[i], A, out + 3 * i, se_out ? se_out + 3 * i : nullptr);
  return SPT_OK;
}

// ---- the two-half filter (SPT_HAS_DENOISE_PAIR) ----
static_assert(sizeof(spt_pair_summary) == 40, "spt_pair_summary layout (the Python mirror's)");

namespace {

struct HostPairPlanes {
  const f4 *ca_, *cb_, *nz_, *av_;
  const float* vtb_;
  int32_t w;
  f4 ca(int32_t x, int32_t y) const { return ca_[(size_t)y * w + x]; }
  f4 cb(int32_t x, int32_t y) const { return cb_[(size_t)y * w + x]; }
  f4 nz(int32_t x, int32_t y) const { return nz_[(size_t)y * w + x]; }
  f4 av(int32_t x, int32_t y) const { return av_[(size_t)y * w + x]; }
  float vtb(int32_t x, int32_t y) const { return vtb_[(size_t)y * w + x]; }
};

spt_status fail_pair(const char* msg) {
  return spt::fail(SPT_ERR_INVALID_ARG, std::string("spt_denoise_pair_host: ") + msg);
}

// The pair filter of validated arguments: out / se_out / diff as spt_denoise_pair_host gives them, or (the
// bank: out NULL) the two halves' finish values o^A and o^B, 3 floats per pixel each.
void pair_filter(const float* rgb_a, const float* se_a, const float* rgb_b, const float* se_b,
                 const float* albedo, const float* normal, const float* depth, int32_t width, int32_t height,
                 const spt_denoise_params* params, uint32_t pair_flags, float* out, float* se_out, float* diff,
                 float* oa, float* ob) {
  const size_t npix = (size_t)width * (size_t)height;
  const auto at = [](float* p, size_t i) { return p ? p + 3 * i : nullptr; };
  if (params->iterations == 0) {
    for (size_t i = 0; i < npix; ++i) {
      if (out)
        finish_pair_zero(rgb_a + 3 * i, se_a + 3 * i, rgb_b + 3 * i, se_b + 3 * i, out + 3 * i, at(se_out, i),
                         at(diff, i));
      else
        for (int k = 0; k < 3; ++k) {
          oa[3 * i + k] = rgb_a[3 * i + k];
          ob[3 * i + k] = rgb_b[3 * i + k];
        }
    }
    return;
  }
  const Args A = make_args(params);
  const bool own = (pair_flags & SPT_DENOISE_PAIR_OWN_WEIGHTS) != 0;
  std::vector<f4> ca0(npix), ca1(npix), cb0(npix), cb1(npix), nz(npix), av(npix);
  std::vector<float> vtb(npix), gx(npix), gy(npix);
  for (int32_t y = 0; y < height; ++y)
    for (int32_t x = 0; x < width; ++x) {
      const size_t i = (size_t)y * width + x;
      ca0[i] = prepare(rgb_a + 3 * i, se_a + 3 * i, albedo + 3 * i, A);
      cb0[i] = prepare(rgb_b + 3 * i, se_b + 3 * i, albedo + 3 * i, A);
      nz[i] = {normal[3 * i], normal[3 * i + 1], normal[3 * i + 2], depth[i]};
      av[i] = {albedo[3 * i], albedo[3 * i + 1], albedo[3 * i + 2], 0.0f};
      gx[i] = gradient(x, width, x > 0 ? depth[i - 1] : 0.0f, depth[i], x < width - 1 ? depth[i + 1] : 0.0f);
      gy[i] = gradient(y, height, y > 0 ? depth[i - width] : 0.0f, depth[i],
                       y < height - 1 ? depth[i + width] : 0.0f);
    }
  f4 *cura = ca0.data(), *nxta = ca1.data(), *curb = cb0.data(), *nxtb = cb1.data();
  for (int32_t it = 0; it < params->iterations; ++it) {
    const HostPlanes PA{cura, nullptr, nullptr, width}, PB{curb, nullptr, nullptr, width};
    for (int32_t y = 0; y < height; ++y)
      for (int32_t x = 0; x < width; ++x) {
        av[(size_t)y * width + x].w = variance_filter(PA, x, y, width, height);
        vtb[(size_t)y * width + x] = variance_filter(PB, x, y, width, height);
      }
    const HostPairPlanes P{cura, curb, nz.data(), av.data(), vtb.data(), width};
    for (int32_t y = 0; y < height; ++y)
      for (int32_t x = 0; x < width; ++x) {
        const size_t i = (size_t)y * width + x;
        iterate_pair(P, x, y, width, height, (int32_t)1 << it, gx[i], gy[i], A, own, &nxta[i], &nxtb[i]);
      }
    std::swap(cura, nxta);
    std::swap(curb, nxtb);
  }
  for (size_t i = 0; i < npix; ++i) {
    if (out)
      finish_pair(cura[i], curb[i], av[i], A, out + 3 * i, at(se_out, i), at(diff, i));
    else
      finish_halves(cura[i], curb[i], av[i], A, oa + 3 * i, ob + 3 * i);
  }
}

}  // namespace

extern "C" spt_status spt_denoise_pair_host(const float* rgb_a, const float* se_a, const float* rgb_b,
                                            const float* se_b, const float* albedo, const float* normal,
                                            const float* depth, int32_t width, int32_t height,
                                            const spt_denoise_params* params, uint32_t pair_flags,
                                            float* out, float* se_out, float* diff) {
  if (!rgb_a || !se_a || !rgb_b || !se_b || !albedo || !normal || !depth || !out) return fail_pair("null plane");
  if (const char* e = params_error(params)) return fail_pair(e);
  if (const char* e = pair_flags_error(pair_flags)) return fail_pair(e);
  if (width <= 0 || height <= 0 || (int64_t)width * (int64_t)height > kMaxPixels)
    return fail_pair("width/height must be positive and hold at most 2^31 - 1 pixels");
  for (const float* o : {(const float*)out, (const float*)se_out, (const float*)diff}) {
    if (!o) continue;
    for (const float* in : {rgb_a, se_a, rgb_b, se_b, albedo, normal, depth})
      if (o == in) return fail_pair("an output plane is an input plane");
  }
  if (se_out == out || diff == out || (se_out && se_out == diff))
    return fail_pair("two output planes are one plane");
  pair_filter(rgb_a, se_a, rgb_b, se_b, albedo, normal, depth, width, height, params, pair_flags, out, se_out,
              diff, nullptr, nullptr);
  return SPT_OK;
}

extern "C" spt_status spt_denoise_pair_summary_host(const float* diff, int32_t width, int32_t height,
                                                    spt_pair_summary* out) {
  if (!diff || !out) return spt::fail(SPT_ERR_INVALID_ARG, "spt_denoise_pair_summary_host: null argument");
  if (width <= 0 || height <= 0 || (int64_t)width * (int64_t)height > kMaxPixels)
    return spt::fail(SPT_ERR_INVALID_ARG,
                     "spt_denoise_pair_summary_host: width/height must be positive and hold at most 2^31 - 1 pixels");
  const size_t npix = (size_t)width * (size_t)height;
  PairPartial t{};
  for (size_t i = 0; i < npix; ++i) pair_partial_add(t, diff + 3 * i);
  pair_summary_finish(t, npix, out);
  return SPT_OK;
}

// ---- the filter bank (SPT_HAS_DENOISE_BANK) ----
static_assert(sizeof(spt_bank_params) == 16, "spt_bank_params layout (the Python mirror's)");
static_assert(sizeof(spt_bank_summary) == 56, "spt_bank_summary layout (the Python mirror's)");

extern "C" void spt_denoise_bank_default_params(spt_bank_params* b) {
  if (!b) return;
  b->error_iterations = 2;
  b->pair_flags = SPT_DENOISE_PAIR_OWN_WEIGHTS;
  b->reserved[0] = b->reserved[1] = 0;
}

namespace {

struct HostBankPlanes {
  const f4 *m_, *nz_, *av_;
  int32_t w;
  f4 m(int32_t x, int32_t y) const { return m_[(size_t)y * w + x]; }
  f4 nz(int32_t x, int32_t y) const { return nz_[(size_t)y * w + x]; }
  f4 av(int32_t x, int32_t y) const { return av_[(size_t)y * w + x]; }
};

spt_status fail_bank(const char* msg) {
  return spt::fail(SPT_ERR_INVALID_ARG, std::string("spt_denoise_bank_host: ") + msg);
}

}  // namespace

extern "C" spt_status spt_denoise_bank_host(const float* rgb_a, const float* se_a, const float* rgb_b,
                                            const float* se_b, const float* albedo, const float* normal,
                                            const float* depth, int32_t width, int32_t height,
                                            const spt_denoise_params* cands, int32_t n_cands,
                                            const spt_bank_params* bank, float* out, float* mse,
                                            uint8_t* choice) {
  if (!rgb_a || !se_a || !rgb_b || !se_b || !albedo || !normal || !depth || !out) return fail_bank("null plane");
  if (const char* e = bank_error(cands, n_cands, bank)) return fail_bank(e);
  if (width <= 0 || height <= 0 || (int64_t)width * (int64_t)height > kMaxPixels)
    return fail_bank("width/height must be positive and hold at most 2^31 - 1 pixels");
  const void* outs[3] = {out, mse, choice};
  for (const void* o : outs) {
    if (!o) continue;
    for (const float* in : {rgb_a, se_a, rgb_b, se_b, albedo, normal, depth})
      if (o == (const void*)in) return fail_bank("an output plane is an input plane");
  }
  if ((const void*)mse == (const void*)out || (const void*)choice == (const void*)out ||
      (mse && (const void*)mse == (const void*)choice))
    return fail_bank("two output planes are one plane");
  const size_t npix = (size_t)width * (size_t)height;
  // 1, 2: every candidate's halves, its out and its error estimate
  std::vector<float> oa(3 * npix), ob(3 * npix), outk((size_t)n_cands * 3 * npix);
  std::vector<f4> m0(npix, f4{0.0f, 0.0f, 0.0f, 0.0f}), m1(npix);
  for (int32_t k = 0; k < n_cands; ++k) {
    pair_filter(rgb_a, se_a, rgb_b, se_b, albedo, normal, depth, width, height, cands + k, bank->pair_flags,
                nullptr, nullptr, nullptr, oa.data(), ob.data());
    for (size_t i = 0; i < npix; ++i) {
      const float m = bank_error_of(oa.data() + 3 * i, ob.data() + 3 * i, rgb_a + 3 * i, se_a + 3 * i,
                                    rgb_b + 3 * i, se_b + 3 * i, outk.data() + (size_t)k * 3 * npix + 3 * i);
      (k == 0 ? m0[i].x : k == 1 ? m0[i].y : k == 2 ? m0[i].z : m0[i].w) = m;
    }
  }
  // 3: the smoothing passes, with the geometric factor of cands[0]
  const Args A = make_args(cands);
  std::vector<f4> nz(npix), av(npix);
  std::vector<float> gx(npix), gy(npix);
  for (int32_t y = 0; y < height; ++y)
    for (int32_t x = 0; x < width; ++x) {
      const size_t i = (size_t)y * width + x;
      nz[i] = {normal[3 * i], normal[3 * i + 1], normal[3 * i + 2], depth[i]};
      av[i] = {albedo[3 * i], albedo[3 * i + 1], albedo[3 * i + 2], 0.0f};
      gx[i] = gradient(x, width, x > 0 ? depth[i - 1] : 0.0f, depth[i], x < width - 1 ? depth[i + 1] : 0.0f);
      gy[i] = gradient(y, height, y > 0 ? depth[i - width] : 0.0f, depth[i],
                       y < height - 1 ? depth[i + width] : 0.0f);
    }
  f4 *cur = m0.data(), *nxt = m1.data();
  for (int32_t it = 0; it < bank->error_iterations; ++it) {
    const HostBankPlanes P{cur, nz.data(), av.data(), width};
    for (int32_t y = 0; y < height; ++y)
      for (int32_t x = 0; x < width; ++x) {
        const size_t i = (size_t)y * width + x;
        nxt[i] = bank_pass<false>(P, x, y, width, height, (int32_t)1 << it, gx[i], gy[i], A, n_cands);
      }
    std::swap(cur, nxt);
  }
  // 4, 5: the choice and the blend
  const HostBankPlanes P{cur, nz.data(), av.data(), width};
  for (int32_t y = 0; y < height; ++y)
    for (int32_t x = 0; x < width; ++x) {
      const size_t i = (size_t)y * width + x;
      const f4 s = bank_pass<true>(P, x, y, width, height, 1, gx[i], gy[i], A, n_cands);
      const float e = bank_blend(s, cur[i], n_cands, outk.data(), 3 * npix, 3 * i, out + 3 * i);
      if (mse) mse[i] = e;
      if (choice) choice[i] = (uint8_t)bank_choice(cur[i], n_cands);
    }
  return SPT_OK;
}

extern "C" spt_status spt_denoise_bank_summary_host(const float* mse, const uint8_t* choice, int32_t width,
                                                    int32_t height, spt_bank_summary* out) {
  if (!mse || !choice || !out) return spt::fail(SPT_ERR_INVALID_ARG, "spt_denoise_bank_summary_host: null argument");
  if (width <= 0 || height <= 0 || (int64_t)width * (int64_t)height > kMaxPixels)
    return spt::fail(SPT_ERR_INVALID_ARG,
                     "spt_denoise_bank_summary_host: width/height must be positive and hold at most 2^31 - 1 pixels");
  const size_t npix = (size_t)width * (size_t)height;
  BankPartial t = bank_partial_zero();
  for (size_t i = 0; i < npix; ++i) bank_partial_add(t, mse[i], choice[i]);
  bank_summary_finish(t, npix, out);
  return SPT_OK;
}

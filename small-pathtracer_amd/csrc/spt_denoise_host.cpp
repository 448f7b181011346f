// spt_denoise_host.cpp — the a-trous filter as a pure host function (include/spt.h, SPT_HAS_DENOISE):
// the CPU statement every GPU denoise test compares the device kernels against, and below it the
// two-half filter and its summary (SPT_HAS_DENOISE_PAIR) and the filter bank (SPT_HAS_DENOISE_BANK). Plain
// C++, no HIP: it is also built into tests/probe/spt_denoise_check, spt_denoise_pair_check and
// spt_denoise_bank_check under the host sanitizers. The three filters share one argument check
// (check_call), one guide pack (HostGuides) and spt_denoise.h's accessor over row-major planes.
#include <cstring>
#include <utility>
#include <vector>

#include "spt_denoise.h"
#include "spt_status.h"

static_assert(sizeof(spt_denoise_params) == 32, "spt_denoise_params layout (the Python mirror's)");
static_assert(sizeof(spt_pair_summary) == 40, "spt_pair_summary layout (the Python mirror's)");
static_assert(sizeof(spt_bank_params) == 16, "spt_bank_params layout (the Python mirror's)");
static_assert(sizeof(spt_bank_summary) == 56, "spt_bank_summary layout (the Python mirror's)");

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

extern "C" void spt_denoise_bank_default_params(spt_bank_params* b) {
  if (!b) return;
  b->error_iterations = 2;
  b->pair_flags = SPT_DENOISE_PAIR_OWN_WEIGHTS;
  b->reserved[0] = b->reserved[1] = 0;
}

namespace {

using namespace spt_denoise_math;
using HostPlanes = Planes<RowMajor>;

spt_status fail(const char* who, const char* msg) {
  return spt::fail(SPT_ERR_INVALID_ARG, std::string(who) + ": " + msg);
}

// What every entry point asks of its arguments, in the order it reports them: the planes there (outs'
// first is the one output that must be; a summary has no output plane), the parameters (perr: what is
// wrong with them, or NULL), the size, no output an input, the outputs distinct.
spt_status check_call(const char* who, const char* perr, int32_t width, int32_t height, PlaneList outs,
                      PlaneList ins) {
  if (!outs.size() && any_null(ins)) return fail(who, "null argument");
  if (any_null(ins) || (outs.size() && !*outs.begin())) return fail(who, "null plane");
  if (perr) return fail(who, perr);
  if (const char* e = size_error(width, height)) return fail(who, e);
  if (const char* e = inputs_error(outs, ins)) return fail(who, e);
  if (const char* e = outputs_error(outs)) return fail(who, e);
  return SPT_OK;
}

// The packed guides and the depth gradient of a whole image.
struct HostGuides {
  std::vector<f4> nz, av;
  std::vector<float> gx, gy;
  HostGuides(const float* normal, const float* depth, const float* albedo, int32_t width, int32_t height)
      : nz((size_t)width * height), av(nz.size()), gx(nz.size()), gy(nz.size()) {
    for (int32_t y = 0; y < height; ++y)
      for (int32_t x = 0; x < width; ++x) {
        const size_t i = (size_t)y * width + x;
        pack_guides(normal, depth, albedo + 3 * i, x, y, width, height, i, &nz[i], &av[i], &gx[i], &gy[i]);
      }
  }
};

// fn(x, y, i) at every pixel, rows first.
template <class Fn>
void for_pixels(int32_t width, int32_t height, const Fn& fn) {
  for (int32_t y = 0; y < height; ++y)
    for (int32_t x = 0; x < width; ++x) fn(x, y, (size_t)y * width + x);
}

}  // namespace

extern "C" spt_status spt_denoise_host(const float* rgb, const float* se, const float* albedo,
                                       const float* normal, const float* depth, int32_t width,
                                       int32_t height, const spt_denoise_params* params, float* out,
                                       float* se_out) {
  SPT_TRY(check_call("spt_denoise_host", params_error(params), width, height, {out, se_out},
                     {rgb, se, albedo, normal, depth}));
  const size_t npix = (size_t)width * (size_t)height;
  if (params->iterations == 0) {
    std::memcpy(out, rgb, npix * 3 * sizeof(float));
    if (se_out) std::memcpy(se_out, se, npix * 3 * sizeof(float));
    return SPT_OK;
  }
  const Args A = make_args(params);
  std::vector<f4> cv0(npix), cv1(npix);
  HostGuides G(normal, depth, albedo, width, height);
  for (size_t i = 0; i < npix; ++i) cv0[i] = prepare(rgb + 3 * i, se + 3 * i, albedo + 3 * i, A);
  f4 *cur = cv0.data(), *nxt = cv1.data();
  for (int32_t it = 0; it < params->iterations; ++it) {
    const HostPlanes P{{width}, G.nz.data(), G.av.data(), cur};
    for_pixels(width, height,
               [&](int32_t x, int32_t y, size_t i) { G.av[i].w = variance_filter(P, x, y, width, height); });
    for_pixels(width, height, [&](int32_t x, int32_t y, size_t i) {
      nxt[i] = iterate(P, x, y, width, height, (int32_t)1 << it, G.gx[i], G.gy[i], A);
    });
    std::swap(cur, nxt);
  }
  for (size_t i = 0; i < npix; ++i) finish(cur[i], G.av[i], A, out + 3 * i, se_out ? se_out + 3 * i : nullptr);
  return SPT_OK;
}

// ---- the two-half filter (SPT_HAS_DENOISE_PAIR) ----
namespace {

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
  std::vector<f4> ca0(npix), ca1(npix), cb0(npix), cb1(npix);
  std::vector<float> vtb(npix);
  HostGuides G(normal, depth, albedo, width, height);
  for (size_t i = 0; i < npix; ++i) {
    ca0[i] = prepare(rgb_a + 3 * i, se_a + 3 * i, albedo + 3 * i, A);
    cb0[i] = prepare(rgb_b + 3 * i, se_b + 3 * i, albedo + 3 * i, A);
  }
  f4 *cura = ca0.data(), *nxta = ca1.data(), *curb = cb0.data(), *nxtb = cb1.data();
  for (int32_t it = 0; it < params->iterations; ++it) {
    const HostPlanes P{{width}, G.nz.data(), G.av.data(), cura, curb, vtb.data()};
    const HostPlanes PB{{width}, nullptr, nullptr, curb};
    for_pixels(width, height, [&](int32_t x, int32_t y, size_t i) {
      G.av[i].w = variance_filter(P, x, y, width, height);
      vtb[i] = variance_filter(PB, x, y, width, height);
    });
    for_pixels(width, height, [&](int32_t x, int32_t y, size_t i) {
      iterate_pair(P, x, y, width, height, (int32_t)1 << it, G.gx[i], G.gy[i], A, own, &nxta[i], &nxtb[i]);
    });
    std::swap(cura, nxta);
    std::swap(curb, nxtb);
  }
  for (size_t i = 0; i < npix; ++i) {
    if (out)
      finish_pair(cura[i], curb[i], G.av[i], A, out + 3 * i, at(se_out, i), at(diff, i));
    else
      finish_halves(cura[i], curb[i], G.av[i], A, oa + 3 * i, ob + 3 * i);
  }
}

}  // namespace

extern "C" spt_status spt_denoise_pair_host(const float* rgb_a, const float* se_a, const float* rgb_b,
                                            const float* se_b, const float* albedo, const float* normal,
                                            const float* depth, int32_t width, int32_t height,
                                            const spt_denoise_params* params, uint32_t pair_flags,
                                            float* out, float* se_out, float* diff) {
  const char* perr = params_error(params);
  SPT_TRY(check_call("spt_denoise_pair_host", perr ? perr : pair_flags_error(pair_flags), width, height,
                     {out, se_out, diff}, {rgb_a, se_a, rgb_b, se_b, albedo, normal, depth}));
  pair_filter(rgb_a, se_a, rgb_b, se_b, albedo, normal, depth, width, height, params, pair_flags, out, se_out,
              diff, nullptr, nullptr);
  return SPT_OK;
}

extern "C" spt_status spt_denoise_pair_summary_host(const float* diff, int32_t width, int32_t height,
                                                    spt_pair_summary* out) {
  SPT_TRY(check_call("spt_denoise_pair_summary_host", nullptr, width, height, {}, {diff, out}));
  const size_t npix = (size_t)width * (size_t)height;
  PairPartial t = pair_partial_zero();
  for (size_t i = 0; i < npix; ++i) pair_partial_add(t, diff + 3 * i);
  pair_summary_finish(t, npix, out);
  return SPT_OK;
}

// ---- the filter bank (SPT_HAS_DENOISE_BANK) ----
extern "C" spt_status spt_denoise_bank_host(const float* rgb_a, const float* se_a, const float* rgb_b,
                                            const float* se_b, const float* albedo, const float* normal,
                                            const float* depth, int32_t width, int32_t height,
                                            const spt_denoise_params* cands, int32_t n_cands,
                                            const spt_bank_params* bank, float* out, float* mse,
                                            uint8_t* choice) {
  SPT_TRY(check_call("spt_denoise_bank_host", bank_error(cands, n_cands, bank), width, height,
                     {out, mse, choice}, {rgb_a, se_a, rgb_b, se_b, albedo, normal, depth}));
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
  const HostGuides G(normal, depth, albedo, width, height);
  f4 *cur = m0.data(), *nxt = m1.data();
  const auto planes = [&] { return HostPlanes{{width}, G.nz.data(), G.av.data(), nullptr, nullptr, nullptr, cur}; };
  for (int32_t it = 0; it < bank->error_iterations; ++it) {
    const HostPlanes P = planes();
    for_pixels(width, height, [&](int32_t x, int32_t y, size_t i) {
      nxt[i] = bank_pass<false>(P, x, y, width, height, (int32_t)1 << it, G.gx[i], G.gy[i], A, n_cands);
    });
    std::swap(cur, nxt);
  }
  // 4, 5: the choice and the blend
  const HostPlanes P = planes();
  for_pixels(width, height, [&](int32_t x, int32_t y, size_t i) {
    const f4 s = bank_pass<true>(P, x, y, width, height, 1, G.gx[i], G.gy[i], A, n_cands);
    const float e = bank_blend(s, cur[i], n_cands, outk.data(), 3 * npix, 3 * i, out + 3 * i);
    if (mse) mse[i] = e;
    if (choice) choice[i] = (uint8_t)bank_choice(cur[i], n_cands);
  });
  return SPT_OK;
}

extern "C" spt_status spt_denoise_bank_summary_host(const float* mse, const uint8_t* choice, int32_t width,
                                                    int32_t height, spt_bank_summary* out) {
  SPT_TRY(check_call("spt_denoise_bank_summary_host", nullptr, width, height, {}, {mse, choice, out}));
  const size_t npix = (size_t)width * (size_t)height;
  BankPartial t = bank_partial_zero();
  for (size_t i = 0; i < npix; ++i) bank_partial_add(t, mse[i], choice[i]);
  bank_summary_finish(t, npix, out);
  return SPT_OK;
}

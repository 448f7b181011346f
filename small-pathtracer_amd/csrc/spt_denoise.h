// spt_denoise.h — the edge-stopping a-trous filter's arithmetic, stated once for the kernels
// (spt_denoise.hip) and for the CPU statement (spt_denoise_host.cpp, plain C++: it runs under the host
// sanitizers). Internal: the public statement is include/spt.h (SPT_HAS_DENOISE, SPT_HAS_DENOISE_PAIR,
// SPT_HAS_DENOISE_BANK). Each piece is stated once for the single, the pair and the bank filter: the
// argument rules (size_error, outputs_error, inputs_error), the guide pack (pack_guides), the plane
// accessor (Planes over the index policies RowMajor and Tile), the tap weights (geom_factors,
// geom_weight, colour_weight, acc_add), the 5 x 5 walk (SPT_FOR_TAPS), the finish (Remod, remodulate)
// and the summaries' partials. The order of every operation is part of the statement: the kernels'
// listings are compared with the previous build's (tools/isa_same.py), not only the bits.
// Needs -ffp-contract=off on both sides. IEEE fp32 + - * /, fmaxf, fminf, fabsf and sqrtf only.
#pragma once
#include <cmath>
#include <cstdint>
#include <initializer_list>

#include "../../include/spt.h"
#include "spt_film_math.h"  // SPT_FILM_FN

namespace spt_denoise_math {

constexpr int32_t kMaxIterations = 6, kMaxSquarings = 8;
constexpr int64_t kMaxPixels = 0x7FFFFFFF;  // the guide's limit: 32-bit pixel counters

// A pixel's packed state: cv = (c_r, c_g, c_b, v), nz = (n_x, n_y, n_z, z), av = (albedo_r, albedo_g,
// albedo_b, vt) with vt the 3x3 binomial filter of the current v (written before every iteration).
struct alignas(16) f4 {  // one 16-byte load on the device
  float x, y, z, w;
};

// The parameters as the filter reads them: the squares taken once on the host.
struct Args {
  float sc2, sa2, sd, floor_;
  int32_t squarings, demodulate;
};

inline Args make_args(const spt_denoise_params* p) {
  Args a;
  a.sc2 = p->sigma_color * p->sigma_color;
  a.sa2 = p->sigma_albedo * p->sigma_albedo;
  a.sd = p->sigma_depth;
  a.floor_ = p->albedo_floor;
  a.squarings = p->normal_squarings;
  a.demodulate = (p->flags & SPT_DENOISE_NO_DEMODULATE) ? 0 : 1;
  return a;
}

// NULL when the parameters are in range, else what is wrong with them.
inline const char* params_error(const spt_denoise_params* p) {
  if (!p) return "null params";
  if (p->iterations < 0 || p->iterations > kMaxIterations) return "iterations outside 0..6";
  if (p->normal_squarings < 0 || p->normal_squarings > kMaxSquarings) return "normal_squarings outside 0..8";
  const float s[4] = {p->sigma_color, p->sigma_depth, p->sigma_albedo, p->albedo_floor};
  for (float v : s)
    if (!(v > 0.0f) || !std::isfinite(v)) return "sigma_color, sigma_depth, sigma_albedo and albedo_floor must be finite and > 0";
  if (p->flags & ~SPT_DENOISE_NO_DEMODULATE) return "unknown flag bits";
  if (p->reserved != 0) return "reserved must be 0";
  return nullptr;
}

// NULL when an image of width x height pixels can be filtered, else what is wrong with it.
inline const char* size_error(int32_t width, int32_t height) {
  return (width <= 0 || height <= 0 || (int64_t)width * (int64_t)height > kMaxPixels)
             ? "width/height must be positive and hold at most 2^31 - 1 pixels"
             : nullptr;
}

// The rules of a call's planes. outs: the outputs, the optional ones NULL when not asked for.
using PlaneList = std::initializer_list<const void*>;

inline bool any_null(PlaneList planes) {
  for (const void* p : planes)
    if (!p) return true;
  return false;
}

// NULL when the outputs asked for are distinct planes.
inline const char* outputs_error(PlaneList outs) {
  for (const void* const* a = outs.begin(); a != outs.end(); ++a)
    for (const void* const* b = a + 1; b != outs.end(); ++b)
      if (*a && *a == *b) return outs.size() == 2 ? "out and se_out are one plane" : "two output planes are one plane";
  return nullptr;
}

// NULL when every input is a plane and none of them is an output.
inline const char* inputs_error(PlaneList outs, PlaneList ins) {
  for (const void* in : ins) {
    if (!in) return "null plane";
    for (const void* o : outs)
      if (in == o) return "an output plane is an input plane";
  }
  return nullptr;
}

SPT_FILM_FN float phi(float x) {
  float t = fmaxf(0.0f, 1.0f - 0.25f * x);
  t = t * t;
  return t * t;
}

SPT_FILM_FN float dot3(float ax, float ay, float az, float bx, float by, float bz) {
  return (ax * bx + ay * by) + az * bz;
}

SPT_FILM_FN float divisor(float albedo, const Args& A) { return A.demodulate ? fmaxf(albedo, A.floor_) : 1.0f; }

// Prepare: the demodulated colour and the variance of one pixel.
SPT_FILM_FN f4 prepare(const float* rgb, const float* se, const float* albedo, const Args& A) {
  const float a0 = divisor(albedo[0], A), a1 = divisor(albedo[1], A), a2 = divisor(albedo[2], A);
  const float e0 = se[0] / a0, e1 = se[1] / a1, e2 = se[2] / a2;
  f4 o;
  o.x = rgb[0] / a0;
  o.y = rgb[1] / a1;
  o.z = rgb[2] / a2;
  o.w = ((e0 * e0 + e1 * e1) + e2 * e2) * (1.0f / 3.0f);
  return o;
}

// The depth gradient along one axis of length n at position i: zm, z0, zp = z(i - 1), z(i), z(i + 1)
// (a value outside the axis is not read by the rule that applies there).
SPT_FILM_FN float gradient(int32_t i, int32_t n, float zm, float z0, float zp) {
  if (n == 1) return 0.0f;
  if (i == 0) return zp - z0;
  if (i == n - 1) return z0 - zm;
  return 0.5f * (zp - zm);
}

// The guide pack of pixel i = y * w + x: (n, z), (albedo, vt = 0) and the depth gradient (gx, gy). normal
// and depth are the planes, albedo the pixel's own three floats.
SPT_FILM_FN void pack_guides(const float* normal, const float* depth, const float* albedo, int32_t x, int32_t y,
                             int32_t w, int32_t h, size_t i, f4* nz, f4* av, float* gx, float* gy) {
  const float z = depth[i];
  *nz = f4{normal[3 * i], normal[3 * i + 1], normal[3 * i + 2], z};
  *av = f4{albedo[0], albedo[1], albedo[2], 0.0f};
  const float zl = x > 0 ? depth[i - 1] : 0.0f, zr = x < w - 1 ? depth[i + 1] : 0.0f;
  const float zu = y > 0 ? depth[i - w] : 0.0f, zd = y < h - 1 ? depth[i + w] : 0.0f;
  *gx = gradient(x, w, zl, z, zr);
  *gy = gradient(y, h, zu, z, zd);
}

SPT_FILM_FN float h5(int k) { return k == 0 ? 0.375f : (k == 1 || k == -1) ? 0.25f : 0.0625f; }

// Where pixel (x, y) lies in a plane: row-major in an image of width w (global memory, the host), or in
// a staged copy KW elements wide whose first element is the image's (x0, y0) (the kernels' LDS tiles).
// own(x, y, i): the same for a caller that holds the pixel's image index i = y * w + x already.
struct RowMajor {
  int32_t w;
  SPT_FILM_FN size_t operator()(int32_t x, int32_t y) const { return (size_t)y * w + x; }
  SPT_FILM_FN size_t own(int32_t, int32_t, size_t i) const { return i; }
};
template <int KW>
struct Tile {
  int32_t x0, y0;
  SPT_FILM_FN int operator()(int32_t x, int32_t y) const { return (y - y0) * KW + (x - x0); }
  SPT_FILM_FN int own(int32_t x, int32_t y, size_t) const { return (*this)(x, y); }
};

// The planes a filter reads, whichever of them its caller supplies: the guides (n, z) and (albedo, vt),
// (c, v) of the single filter or of half A, (c, v) and vt of half B, the bank's four estimates.
template <class Index>
struct Planes {
  Index at;
  const f4 *nz_, *av_, *cv_, *cb_;
  const float* vtb_;
  const f4* m_;
  SPT_FILM_FN f4 nz(int32_t x, int32_t y) const { return nz_[at(x, y)]; }
  SPT_FILM_FN f4 av(int32_t x, int32_t y) const { return av_[at(x, y)]; }
  SPT_FILM_FN f4 av_own(int32_t x, int32_t y, size_t i) const { return av_[at.own(x, y, i)]; }
  SPT_FILM_FN f4 cv(int32_t x, int32_t y) const { return cv_[at(x, y)]; }
  SPT_FILM_FN f4 cb(int32_t x, int32_t y) const { return cb_[at(x, y)]; }
  SPT_FILM_FN float vtb(int32_t x, int32_t y) const { return vtb_[at(x, y)]; }
  SPT_FILM_FN f4 m(int32_t x, int32_t y) const { return m_[at(x, y)]; }
};

// vt: the 3x3 binomial filter of the v of plane cv at spacing 1, taps outside the image skipped.
template <class Plane>
SPT_FILM_FN float variance_filter(const Plane& P, int32_t x, int32_t y, int32_t w, int32_t h) {
  float s = 0.0f, ws = 0.0f;
  for (int dy = -1; dy <= 1; ++dy) {
    const int32_t yy = y + dy;
    if (yy < 0 || yy >= h) continue;
    for (int dx = -1; dx <= 1; ++dx) {
      const int32_t xx = x + dx;
      if (xx < 0 || xx >= w) continue;
      const float k = (float)((2 - (dy < 0 ? -dy : dy)) * (2 - (dx < 0 ? -dx : dx))) * 0.0625f;
      s = s + k * P.cv(xx, yy).w;
      ws = ws + k;
    }
  }
  return s / ws;
}

// The running sums of one pixel's iteration.
struct Acc {
  float c0, c1, c2, v, w;
};

SPT_FILM_FN void acc_add(Acc& a, float w, const f4& cvq) {
  a.w = a.w + w;
  a.c0 = a.c0 + w * cvq.x;
  a.c1 = a.c1 + w * cvq.y;
  a.c2 = a.c2 + w * cvq.z;
  a.v = a.v + (w * w) * cvq.w;
}

constexpr float kCentre = 0.375f * 0.375f;  // the centre tap's weight: h5(0)^2, no edge-stopping factor
SPT_FILM_FN void acc_centre(Acc& a, const f4& cv) { acc_add(a, kCentre, cv); }

// The edge-stopping factors of a tap that is not the centre, no colour in them: the normals', the
// depths' and the albedos'. The tap's offset is (i, j) * step, i the column's, j the row's index in -2..2.
struct Geom {
  float wn, wz, wa;
};

SPT_FILM_FN Geom geom_factors(int i, int j, int32_t step, const f4& nzp, const f4& avp, float gx, float gy,
                              const f4& nzq, const f4& avq, const Args& A) {
  float wn = fmaxf(0.0f, dot3(nzp.x, nzp.y, nzp.z, nzq.x, nzq.y, nzq.z));
  for (int k = 0; k < A.squarings; ++k) wn = wn * wn;
  const float dx = (float)(i * step), dy = (float)(j * step);
  const float wz = phi(fabsf(nzp.w - nzq.w) / ((A.sd * fabsf(gx * dx + gy * dy) + 1e-3f * nzp.w) + 1e-6f));
  const float a0 = avp.x - avq.x, a1 = avp.y - avq.y, a2 = avp.z - avq.z;
  const float wa = phi(dot3(a0, a1, a2, a0, a1, a2) / A.sa2);
  return Geom{wn, wz, wa};
}

// The geometric factor g of the tap: the kernel's weight times the three factors, in this order. Its own
// function because the single filter computes its colour weight between the factors and this product.
SPT_FILM_FN float geom_weight(int i, int j, const Geom& f) { return (((h5(j) * h5(i)) * f.wn) * f.wz) * f.wa; }

// The colour weight of a tap: cp, cq the two ends' (c, v), vtp, vtq their filtered variances.
SPT_FILM_FN float colour_weight(const f4& cp, const f4& cq, float vtp, float vtq, const Args& A) {
  const float d0 = cp.x - cq.x, d1 = cp.y - cq.y, d2 = cp.z - cq.z;
  return phi(dot3(d0, d1, d2, d0, d1, d2) / (A.sc2 * (vtp + vtq) + 1e-10f));
}

// One tap that is not the centre. av.w holds vt.
SPT_FILM_FN void acc_tap(Acc& a, int i, int j, int32_t step, const f4& cvp, const f4& nzp, const f4& avp,
                         float gx, float gy, const f4& cvq, const f4& nzq, const f4& avq, const Args& A) {
  const Geom f = geom_factors(i, j, step, nzp, avp, gx, gy, nzq, avq, A);
  const float wc = colour_weight(cvp, cvq, avp.w, avq.w, A);
  acc_add(a, geom_weight(i, j, f) * wc, cvq);
}

SPT_FILM_FN f4 acc_result(const Acc& a) {
  f4 o;
  o.x = a.c0 / a.w;
  o.y = a.c1 / a.w;
  o.z = a.c2 / a.w;
  o.w = a.v / (a.w * a.w);
  return o;
}

// The 5 x 5 taps of pixel (x, y) at spacing `step` that lie inside the image, rows first: the statement
// that follows runs with int i, j (the column's and the row's index in -2..2) and int32_t qx, qy (the
// tap's pixel). A macro, not a function taking the body: a closure's captures change the order in which
// the compiler meets the body's values, and with it the kernels' schedules.
#define SPT_FOR_TAPS(x, y, w, h, step)                                                        \
  for (int j = -2; j <= 2; ++j)                                                               \
    if (const int64_t yy_ = (int64_t)(y) + (int64_t)j * (step); yy_ >= 0 && yy_ < (h))         \
      for (int i = -2; i <= 2; ++i)                                                           \
        if (const int64_t xx_ = (int64_t)(x) + (int64_t)i * (step); xx_ >= 0 && xx_ < (w))     \
          if (const int32_t qx = (int32_t)xx_, qy = (int32_t)yy_; true)

// One pixel of one iteration. P: Planes with cv, nz, av.
template <class P>
SPT_FILM_FN f4 iterate(const P& pl, int32_t x, int32_t y, int32_t w, int32_t h, int32_t step, float gx,
                       float gy, const Args& A) {
  const f4 cvp = pl.cv(x, y), nzp = pl.nz(x, y), avp = pl.av(x, y);
  Acc a = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  SPT_FOR_TAPS(x, y, w, h, step) {
    if (i == 0 && j == 0)
      acc_centre(a, cvp);
    else
      acc_tap(a, i, j, step, cvp, nzp, avp, gx, gy, pl.cv(qx, qy), pl.nz(qx, qy), pl.av(qx, qy), A);
  }
  return acc_result(a);
}

// The finish of a pixel: its three divisors, taken once; a colour remodulated and clamped to 1; the
// standard error s of a demodulated colour remodulated.
struct Remod {
  float a[3];
};
SPT_FILM_FN Remod remod_of(const f4& av, const Args& A) {
  return Remod{{divisor(av.x, A), divisor(av.y, A), divisor(av.z, A)}};
}
SPT_FILM_FN void remodulate(const f4& c, const Remod& r, float* o) {
  o[0] = fminf(c.x * r.a[0], 1.0f);
  o[1] = fminf(c.y * r.a[1], 1.0f);
  o[2] = fminf(c.z * r.a[2], 1.0f);
}
SPT_FILM_FN void remodulate_error(float s, const Remod& r, float* se_out) {
  se_out[0] = s * r.a[0];
  se_out[1] = s * r.a[1];
  se_out[2] = s * r.a[2];
}

// Finish: remodulate, clamp; the standard error that is left.
SPT_FILM_FN void finish(const f4& cv, const f4& av, const Args& A, float* out, float* se_out) {
  const Remod r = remod_of(av, A);
  remodulate(cv, r, out);
  if (se_out) remodulate_error(sqrtf(cv.w), r, se_out);
}

// ---- the two-half filter (include/spt.h, SPT_HAS_DENOISE_PAIR) ----
// Two runs of the filter above over the halves A and B that share the guides, fused tap by tap: the
// geometric factor g of a tap is computed once, each half has its own colour weight, and a half
// accumulates with the other half's colour weight (cross) or with its own (own). g * w_c is acc_tap's
// product, so equal halves give the single filter's bits.

// NULL when the pair flags are known, else what is wrong with them.
inline const char* pair_flags_error(uint32_t pair_flags) {
  return (pair_flags & ~SPT_DENOISE_PAIR_OWN_WEIGHTS) ? "unknown pair_flags bits" : nullptr;
}

// One tap that is not the centre, for both halves. av.w holds vt of half A; vtb is half B's vt.
SPT_FILM_FN void acc_tap_pair(Acc& a, Acc& b, int i, int j, int32_t step, const f4& cap, const f4& cbp,
                              const f4& nzp, const f4& avp, float vtbp, float gx, float gy, const f4& caq,
                              const f4& cbq, const f4& nzq, const f4& avq, float vtbq, const Args& A,
                              bool own) {
  const float g = geom_weight(i, j, geom_factors(i, j, step, nzp, avp, gx, gy, nzq, avq, A));
  const float wca = colour_weight(cap, caq, avp.w, avq.w, A), wcb = colour_weight(cbp, cbq, vtbp, vtbq, A);
  acc_add(a, g * (own ? wca : wcb), caq);
  acc_add(b, g * (own ? wcb : wca), cbq);
}

// One pixel of one iteration of both halves. P: Planes with cv (half A), cb, nz, av and vtb.
template <class P>
SPT_FILM_FN void iterate_pair(const P& pl, int32_t x, int32_t y, int32_t w, int32_t h, int32_t step, float gx,
                              float gy, const Args& A, bool own, f4* ra, f4* rb) {
  const f4 cap = pl.cv(x, y), cbp = pl.cb(x, y), nzp = pl.nz(x, y), avp = pl.av(x, y);
  const float vtbp = pl.vtb(x, y);
  Acc a = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, b = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  SPT_FOR_TAPS(x, y, w, h, step) {
    if (i == 0 && j == 0) {
      acc_centre(a, cap);
      acc_centre(b, cbp);
    } else {
      acc_tap_pair(a, b, i, j, step, cap, cbp, nzp, avp, vtbp, gx, gy, pl.cv(qx, qy), pl.cb(qx, qy),
                   pl.nz(qx, qy), pl.av(qx, qy), pl.vtb(qx, qy), A, own);
    }
  }
  *ra = acc_result(a);
  *rb = acc_result(b);
}

// The pair's outputs from the two remodulated, clamped halves oa, ob (3 floats each).
SPT_FILM_FN void pair_combine(const float* oa, const float* ob, float* out, float* diff) {
  for (int k = 0; k < 3; ++k) {
    out[k] = 0.5f * (oa[k] + ob[k]);
    if (diff) diff[k] = 0.5f * (oa[k] - ob[k]);
  }
}

// Finish of the pair: each half remodulated and clamped, their mean, half their difference, and the
// propagated standard error of the mean.
SPT_FILM_FN void finish_pair(const f4& ca, const f4& cb, const f4& av, const Args& A, float* out,
                             float* se_out, float* diff) {
  const Remod r = remod_of(av, A);
  float oa[3], ob[3];
  remodulate(ca, r, oa);
  remodulate(cb, r, ob);
  pair_combine(oa, ob, out, diff);
  if (se_out) remodulate_error(0.5f * sqrtf(ca.w + cb.w), r, se_out);
}

// iterations == 0: the halves as given.
SPT_FILM_FN void finish_pair_zero(const float* rgb_a, const float* se_a, const float* rgb_b,
                                  const float* se_b, float* out, float* se_out, float* diff) {
  pair_combine(rgb_a, rgb_b, out, diff);
  if (se_out)
    for (int k = 0; k < 3; ++k) se_out[k] = 0.5f * sqrtf(se_a[k] * se_a[k] + se_b[k] * se_b[k]);
}

// The summary of a diff plane: the sums of (double)diff_k^2 and the largest |diff|.
struct PairPartial {
  double s[3];
  float diff_max;
};

SPT_FILM_FN PairPartial pair_partial_zero() { return PairPartial{}; }

SPT_FILM_FN void pair_partial_merge(PairPartial& a, const PairPartial& b) {
  for (int k = 0; k < 3; ++k) a.s[k] += b.s[k];
  a.diff_max = fmaxf(a.diff_max, b.diff_max);
}

SPT_FILM_FN void pair_partial_add(PairPartial& p, const float* diff) {
  for (int k = 0; k < 3; ++k) {
    const double d = (double)diff[k];
    p.s[k] += d * d;
    p.diff_max = fmaxf(p.diff_max, fabsf(diff[k]));
  }
}

inline void pair_summary_finish(const PairPartial& t, size_t npix, spt_pair_summary* out) {
  const double n = (double)npix;
  for (int k = 0; k < 3; ++k) out->rmse[k] = std::sqrt(t.s[k] / n);
  out->rmse_all = std::sqrt(((t.s[0] + t.s[1]) + t.s[2]) / (3.0 * n));
  out->diff_max = t.diff_max;
  out->reserved = 0;
}

// ---- the filter bank (include/spt.h, SPT_HAS_DENOISE_BANK) ----
// The pair filter at a few parameter sets, a cross-validated error estimate per pixel and candidate,
// smoothed with the geometric factor alone, and the candidates blended by the smoothed choice.

constexpr int32_t kMaxCands = SPT_BANK_MAX_CANDIDATES, kMaxErrorIterations = 3;

// NULL when the candidates and the bank parameters are in range, else what is wrong with them.
inline const char* bank_error(const spt_denoise_params* cands, int32_t n_cands, const spt_bank_params* b) {
  if (!cands) return "null candidates";
  if (n_cands < 1 || n_cands > kMaxCands) return "n_cands outside 1..4";
  for (int32_t k = 0; k < n_cands; ++k)
    if (const char* e = params_error(cands + k)) return e;
  if (!b) return "null bank params";
  if (b->error_iterations < 0 || b->error_iterations > kMaxErrorIterations) return "error_iterations outside 0..3";
  if (const char* e = pair_flags_error(b->pair_flags)) return e;
  if (b->reserved[0] != 0 || b->reserved[1] != 0) return "reserved must be 0";
  return nullptr;
}

// The pair's finish with the halves kept: o^A and o^B as finish_pair takes them.
SPT_FILM_FN void finish_halves(const f4& ca, const f4& cb, const f4& av, const Args& A, float* oa, float* ob) {
  const Remod r = remod_of(av, A);
  remodulate(ca, r, oa);
  remodulate(cb, r, ob);
}

// Step 2: a candidate's out (3 floats) and its cross-validated error m at one pixel.
SPT_FILM_FN float bank_error_of(const float* oa, const float* ob, const float* rgb_a, const float* se_a,
                                const float* rgb_b, const float* se_b, float* out) {
  float m[3];
  for (int c = 0; c < 3; ++c) {
    out[c] = 0.5f * (oa[c] + ob[c]);
    const float d = 0.5f * (oa[c] - ob[c]);
    const float ra = oa[c] - rgb_b[c], rb = ob[c] - rgb_a[c];
    const float e = 0.5f * ((ra * ra - se_b[c] * se_b[c]) + (rb * rb - se_a[c] * se_a[c]));
    m[c] = e - d * d;
  }
  return ((m[0] + m[1]) + m[2]) * (1.0f / 3.0f);
}

// Step 4: the smallest k < n whose estimate is least.
SPT_FILM_FN int bank_choice(const f4& m, int32_t n) {
  int k = 0;
  float best = m.x;
  if (n > 1 && m.y < best) {
    k = 1;
    best = m.y;
  }
  if (n > 2 && m.z < best) {
    k = 2;
    best = m.z;
  }
  if (n > 3 && m.w < best) k = 3;
  return k;
}

// Steps 3 and 5 at one pixel. P: Planes with m, nz, av; m holds the four candidates' estimates (those
// of no candidate are 0 and stay 0). BLEND false: one smoothing pass, the smoothed estimates. BLEND true
// (step 1): the shares s_k of the n candidates among the neighbours' choices.
template <bool BLEND, class P>
SPT_FILM_FN f4 bank_pass(const P& pl, int32_t x, int32_t y, int32_t w, int32_t h, int32_t step, float gx,
                         float gy, const Args& A, int32_t n) {
  const f4 nzp = pl.nz(x, y), avp = pl.av(x, y);
  float W = 0.0f;
  f4 M = {0.0f, 0.0f, 0.0f, 0.0f};
  SPT_FOR_TAPS(x, y, w, h, step) {
    const f4 mq = pl.m(qx, qy);
    const float g =
        (i == 0 && j == 0)
            ? kCentre
            : geom_weight(i, j, geom_factors(i, j, step, nzp, avp, gx, gy, pl.nz(qx, qy), pl.av(qx, qy), A));
    W = W + g;
    if constexpr (BLEND) {
      const int kq = bank_choice(mq, n);
      M.x = M.x + g * (kq == 0 ? 1.0f : 0.0f);
      M.y = M.y + g * (kq == 1 ? 1.0f : 0.0f);
      M.z = M.z + g * (kq == 2 ? 1.0f : 0.0f);
      M.w = M.w + g * (kq == 3 ? 1.0f : 0.0f);
    } else {
      M.x = M.x + g * mq.x;
      M.y = M.y + g * mq.y;
      M.z = M.z + g * mq.z;
      M.w = M.w + g * mq.w;
    }
  }
  return f4{M.x / W, M.y / W, M.z / W, M.w / W};
}

// Step 5's sums at one pixel: s the shares, m the pixel's smoothed estimates, outk the n candidates' out
// planes `stride` floats apart, i3 = 3 * the pixel's index. -> mse.
SPT_FILM_FN float bank_blend(const f4& s, const f4& m, int32_t n, const float* outk, size_t stride, size_t i3,
                             float* out) {
  const float sk[4] = {s.x, s.y, s.z, s.w}, mk[4] = {m.x, m.y, m.z, m.w};
  float o[3] = {0.0f, 0.0f, 0.0f}, mse = 0.0f;
  for (int k = 0; k < 4; ++k) {  // fixed bounds: sk and mk stay in registers
    if (k >= n) break;
    const float* q = outk + (size_t)k * stride + i3;
    o[0] = o[0] + sk[k] * q[0];
    o[1] = o[1] + sk[k] * q[1];
    o[2] = o[2] + sk[k] * q[2];
    mse = mse + sk[k] * mk[k];
  }
  out[0] = fminf(o[0], 1.0f);
  out[1] = fminf(o[1], 1.0f);
  out[2] = fminf(o[2], 1.0f);
  return mse;
}

// The summary of an mse and a choice plane.
struct BankPartial {
  double sum, count[4];
  float mn, mx;
};

SPT_FILM_FN BankPartial bank_partial_zero() {
  BankPartial p;
  p.sum = 0.0;
  for (int k = 0; k < 4; ++k) p.count[k] = 0.0;
  p.mn = INFINITY;
  p.mx = -INFINITY;
  return p;
}

SPT_FILM_FN void bank_partial_add(BankPartial& p, float mse, uint8_t choice) {
  p.sum += (double)mse;
  for (int k = 0; k < 4; ++k) p.count[k] += choice == k ? 1.0 : 0.0;
  p.mn = fminf(p.mn, mse);
  p.mx = fmaxf(p.mx, mse);
}

SPT_FILM_FN void bank_partial_merge(BankPartial& a, const BankPartial& b) {
  a.sum += b.sum;
  for (int k = 0; k < 4; ++k) a.count[k] += b.count[k];
  a.mn = fminf(a.mn, b.mn);
  a.mx = fmaxf(a.mx, b.mx);
}

inline void bank_summary_finish(const BankPartial& t, size_t npix, spt_bank_summary* out) {
  const double n = (double)npix;
  out->mse_mean = t.sum / n;
  out->rmse_est = std::sqrt(out->mse_mean > 0.0 ? out->mse_mean : 0.0);
  for (int k = 0; k < 4; ++k) out->share[k] = t.count[k] / n;
  out->mse_min = t.mn;
  out->mse_max = t.mx;
}

#undef SPT_FOR_TAPS

}  // namespace spt_denoise_math

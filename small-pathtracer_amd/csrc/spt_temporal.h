// spt_temporal.h — temporal accumulation's arithmetic, stated once for the kernel (spt_temporal.hip) and
// for the CPU statement (spt_temporal_host.cpp, plain C++: it runs under the host sanitizers). Internal:
// the public statement is include/spt.h (SPT_HAS_TEMPORAL). Here: the parameter and camera rules, the host
// constants of a call (camera_consts, make_consts: double arithmetic, each value rounded once) and one
// pixel's accumulation (accumulate_pixel) over a previous state that its caller reaches through an
// accessor: the host's 13 row-major planes or the device's packed planes. The order of every operation
// is part of the statement. Needs -ffp-contract=off on both sides. IEEE fp32 + - * /, fmaxf, fminf,
// fabsf, sqrtf, floorf and one float -> int conversion behind float range checks.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/spt.h"
#include "spt_denoise.h"  // f4, dot3, size_error and the plane rules

namespace spt_temporal_math {

using spt_denoise_math::dot3;
using spt_denoise_math::f4;

// NULL when the parameters are in range, else what is wrong with them.
inline const char* params_error(const spt_temporal_params* p) {
  if (!p) return "null params";
  const float s[4] = {p->n_max, p->normal_min, p->plane_tol, p->albedo_floor};
  for (float v : s)
    if (!std::isfinite(v)) return "n_max, normal_min, plane_tol and albedo_floor must be finite";
  if (!(p->n_max >= 1.0f)) return "n_max must be >= 1";
  if (!(p->normal_min >= -1.0f && p->normal_min <= 1.0f)) return "normal_min outside -1..1";
  if (!(p->plane_tol >= 0.0f)) return "plane_tol must be >= 0";
  if (!(p->albedo_floor > 0.0f)) return "albedo_floor must be > 0";
  if (p->flags & ~SPT_TEMPORAL_NO_DEMODULATE) return "unknown flag bits";
  if (p->reserved != 0) return "reserved must be 0";
  return nullptr;
}

// A camera as the pixels read it: o, E = llc - o, Hx = hor / w, Vy = ver / h and M, the inverse of the
// matrix with the columns (Hx, Vy, E), rows in order. Doubles throughout, each value rounded once.
struct CamConsts {
  float o[3], E[3], Hx[3], Vy[3], M[9];
};

// false when the camera is singular (its three vectors span no volume) or not finite.
inline bool camera_consts(const spt_camera* cam, int32_t w, int32_t h, CamConsts* out) {
  double a[3], b[3], c[3];
  for (int k = 0; k < 3; ++k) {
    a[k] = cam->horizontal[k] / (double)w;
    b[k] = cam->vertical[k] / (double)h;
    c[k] = cam->lower_left_corner[k] - cam->origin[k];
  }
  const double bc[3] = {b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0]};
  const double ca[3] = {c[1] * a[2] - c[2] * a[1], c[2] * a[0] - c[0] * a[2], c[0] * a[1] - c[1] * a[0]};
  const double ab[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
  const double det = (a[0] * bc[0] + a[1] * bc[1]) + a[2] * bc[2];
  if (!std::isfinite(det) || !(std::fabs(det) > 0.0)) return false;
  for (int k = 0; k < 3; ++k) {
    out->o[k] = (float)cam->origin[k];
    out->E[k] = (float)c[k];
    out->Hx[k] = (float)a[k];
    out->Vy[k] = (float)b[k];
    out->M[k] = (float)(bc[k] / det);
    out->M[3 + k] = (float)(ca[k] / det);
    out->M[6 + k] = (float)(ab[k] / det);
  }
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(out->o[k]) || !std::isfinite(out->E[k]) || !std::isfinite(out->Hx[k]) ||
        !std::isfinite(out->Vy[k]))
      return false;
  for (float m : out->M)
    if (!std::isfinite(m)) return false;
  return true;
}

// The same-camera rule's test: the twelve doubles equal.
inline bool same_camera(const spt_camera* a, const spt_camera* b) {
  for (int k = 0; k < 3; ++k)
    if (a->origin[k] != b->origin[k] || a->lower_left_corner[k] != b->lower_left_corner[k] ||
        a->horizontal[k] != b->horizontal[k] || a->vertical[k] != b->vertical[k])
      return false;
  return true;
}

// What one call's pixels read: the current camera, the previous one (po, M), the parameters, and what
// the host decided once: whether there is a history and whether the same-camera rule applies.
struct Consts {
  float o[3], E[3], Hx[3], Vy[3];
  float po[3], M[9];
  float n_max, normal_min, plane_tol, floor_;
  int32_t demodulate, has_prev, same;
};

inline Consts make_consts(const CamConsts& cur, const CamConsts* prev, bool same, const spt_temporal_params* p) {
  Consts K;
  for (int k = 0; k < 3; ++k) {
    K.o[k] = cur.o[k];
    K.E[k] = cur.E[k];
    K.Hx[k] = cur.Hx[k];
    K.Vy[k] = cur.Vy[k];
    K.po[k] = prev ? prev->o[k] : 0.0f;
  }
  for (int k = 0; k < 9; ++k) K.M[k] = prev ? prev->M[k] : 0.0f;
  K.n_max = p->n_max;
  K.normal_min = p->normal_min;
  K.plane_tol = p->plane_tol;
  K.floor_ = p->albedo_floor;
  K.demodulate = (p->flags & SPT_TEMPORAL_NO_DEMODULATE) ? 0 : 1;
  K.has_prev = prev ? 1 : 0;
  K.same = (prev && same) ? 1 : 0;
  return K;
}

// A tap of the previous state in two parts: what the validity tests read, and what a valid tap adds.
struct TapGeom {
  float N[3], n, X[3];
};
struct TapColour {
  float c[3], v[3];
};

// The previous state as the host holds it: 13 row-major planes (c, v, n, X, N of spt_temporal_state).
struct HostPrev {
  const float *c, *v, *n, *X, *N;
  TapGeom geom(size_t i) const {
    return TapGeom{{N[3 * i], N[3 * i + 1], N[3 * i + 2]}, n[i], {X[3 * i], X[3 * i + 1], X[3 * i + 2]}};
  }
  TapColour colour(size_t i) const {
    return TapColour{{c[3 * i], c[3 * i + 1], c[3 * i + 2]}, {v[3 * i], v[3 * i + 1], v[3 * i + 2]}};
  }
};

// One pixel's results: the outputs and the new state (its normal is the input normal).
struct Pixel {
  float rgb_out[3], se_out[3], hist[3];
  float c[3], v[3], n, X[3];
};

// Steps 1-7 of spt.h for pixel (x, y). rgb, se, albedo, normal: the pixel's own three floats; z its depth.
template <class Prev>
SPT_FILM_FN Pixel accumulate_pixel(const float* rgb, const float* se, const float* albedo, const float* normal,
                                   float z, int32_t x, int32_t y, int32_t w, int32_t h, const Consts& K,
                                   const Prev& prev) {
  Pixel P;
  // 1: the current estimate
  float a[3], c[3], var[3];
  for (int k = 0; k < 3; ++k) {
    a[k] = K.demodulate ? fmaxf(albedo[k], K.floor_) : 1.0f;
    c[k] = rgb[k] / a[k];
    const float e = se[k] / a[k];
    var[k] = e * e;
  }
  // 2: the world point
  const float px = (float)x, py = (float)(h - 1 - y);
  float D[3];
  for (int k = 0; k < 3; ++k) D[k] = (K.E[k] + K.Hx[k] * px) + K.Vy[k] * py;
  const float len = sqrtf((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]);
  for (int k = 0; k < 3; ++k) P.X[k] = K.o[k] + (D[k] / len) * z;
  const bool miss = z == 0.0f;
  bool ok = K.has_prev && !miss;
  // 3: the previous pixel (the same-camera rule: the pixel itself, no resampling)
  int32_t x0 = x, y0 = y;
  float tx = 0.0f, ty = 0.0f;
  if (ok && !K.same) {
    const float q0 = P.X[0] - K.po[0], q1 = P.X[1] - K.po[1], q2 = P.X[2] - K.po[2];
    const float A = (K.M[0] * q0 + K.M[1] * q1) + K.M[2] * q2;
    const float B = (K.M[3] * q0 + K.M[4] * q1) + K.M[5] * q2;
    const float C = (K.M[6] * q0 + K.M[7] * q1) + K.M[8] * q2;
    ok = C > 0.0f;
    if (ok) {
      const float fx = A / C, fy = (float)(h - 1) - B / C;
      ok = fx >= -1.0f && fx < (float)w && fy >= -1.0f && fy < (float)h;
      if (ok) {
        const float flx = floorf(fx), fly = floorf(fy);
        x0 = (int32_t)flx;
        y0 = (int32_t)fly;
        tx = fx - flx;
        ty = fy - fly;
      }
    }
  }
  // 4: the taps
  float W = 0.0f, Ch[3] = {0.0f, 0.0f, 0.0f}, Vh[3] = {0.0f, 0.0f, 0.0f}, Nh = 0.0f;
  if (ok) {
    for (int j = 0; j < 2; ++j)
      for (int i = 0; i < 2; ++i) {
        if (K.same && (i | j)) continue;
        const int32_t xx = x0 + i, yy = y0 + j;
        if (xx < 0 || xx >= w || yy < 0 || yy >= h) continue;
        const float b = K.same ? 1.0f : (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
        const size_t qi = (size_t)yy * (size_t)w + (size_t)xx;
        const TapGeom g = prev.geom(qi);
        if (!(g.n > 0.0f)) continue;
        if (!(dot3(normal[0], normal[1], normal[2], g.N[0], g.N[1], g.N[2]) >= K.normal_min)) continue;
        const float off = dot3(normal[0], normal[1], normal[2], g.X[0] - P.X[0], g.X[1] - P.X[1], g.X[2] - P.X[2]);
        if (!(fabsf(off) <= K.plane_tol * z)) continue;
        const TapColour t = prev.colour(qi);
        W = W + b;
        for (int k = 0; k < 3; ++k) {
          Ch[k] = Ch[k] + b * t.c[k];
          Vh[k] = Vh[k] + b * t.v[k];
        }
        Nh = Nh + b * g.n;
      }
    ok = W >= 0.25f;
  }
  // 6: the blend
  if (ok) {
    const float n1 = fminf(Nh / W + 1.0f, K.n_max);
    const float alpha = 1.0f / n1, beta = 1.0f - alpha;
    for (int k = 0; k < 3; ++k) {
      const float ch = Ch[k] / W, vh = Vh[k] / W;
      P.c[k] = beta * ch + alpha * c[k];
      P.v[k] = (beta * beta) * vh + (alpha * alpha) * var[k];
      P.hist[k] = ch * a[k];
    }
    P.n = n1;
  } else {
    for (int k = 0; k < 3; ++k) {
      P.c[k] = c[k];
      P.v[k] = var[k];
      P.hist[k] = rgb[k];
    }
    P.n = miss ? 0.0f : 1.0f;
  }
  // 7: the outputs
  for (int k = 0; k < 3; ++k) {
    P.rgb_out[k] = fminf(P.c[k] * a[k], 1.0f);
    P.se_out[k] = sqrtf(P.v[k]) * a[k];
  }
  return P;
}

}  // namespace spt_temporal_math

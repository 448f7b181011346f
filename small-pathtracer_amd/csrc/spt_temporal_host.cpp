// spt_temporal_host.cpp — temporal accumulation as a pure host function (include/spt.h, SPT_HAS_TEMPORAL):
// the CPU statement every GPU temporal test compares the kernel against. Plain C++, no HIP: it is also
// built into tests/probe/spt_temporal_check under the host sanitizers. The arithmetic is spt_temporal.h's.
#include "spt_temporal.h"
#include "spt_status.h"

static_assert(sizeof(spt_temporal_params) == 24, "spt_temporal_params layout (the Python mirror's)");
static_assert(sizeof(spt_temporal_state) == 40, "spt_temporal_state layout (the Python mirror's)");
static_assert(sizeof(spt_temporal_info) == 24, "spt_temporal_info layout (the Python mirror's)");

extern "C" void spt_temporal_default_params(spt_temporal_params* p) {
  if (!p) return;
  p->n_max = 32.0f;
  p->normal_min = 0.9f;
  p->plane_tol = 0.01f;
  p->albedo_floor = 0.01f;
  p->flags = 0;
  p->reserved = 0;
}

namespace {

using namespace spt_temporal_math;
using namespace spt_denoise_math;  // the plane rules

spt_status fail(const char* msg) {
  return spt::fail(SPT_ERR_INVALID_ARG, std::string("spt_temporal_accumulate_host: ") + msg);
}

}  // namespace

extern "C" spt_status spt_temporal_accumulate_host(const float* rgb, const float* se, const float* albedo,
                                                   const float* normal, const float* depth, int32_t width,
                                                   int32_t height, const spt_camera* cam,
                                                   const spt_temporal_params* params,
                                                   const spt_temporal_state* prev, const spt_camera* prev_cam,
                                                   float* rgb_out, float* se_out, float* n_out, float* hist,
                                                   const spt_temporal_state* next) {
  if (!cam || !next) return fail("null argument");
  if (any_null({rgb, se, albedo, normal, depth, rgb_out, se_out, next->c, next->v, next->n, next->X, next->N}))
    return fail("null plane");
  if ((prev == nullptr) != (prev_cam == nullptr)) return fail("a previous state needs its camera and a camera its state");
  if (prev && any_null({prev->c, prev->v, prev->n, prev->X, prev->N})) return fail("null plane");
  if (const char* e = spt_temporal_math::params_error(params)) return fail(e);
  if (const char* e = size_error(width, height)) return fail(e);
  const PlaneList outs = {rgb_out, se_out, n_out, hist, next->c, next->v, next->n, next->X, next->N};
  if (const char* e = inputs_error(outs, {rgb, se, albedo, normal, depth})) return fail(e);
  if (prev)
    if (const char* e = inputs_error(outs, {prev->c, prev->v, prev->n, prev->X, prev->N})) return fail(e);
  if (outputs_error(outs)) return fail("two output planes are one plane");
  CamConsts cur, old;
  if (!camera_consts(cam, width, height, &cur)) return fail("the camera is singular or not finite");
  if (prev_cam && !camera_consts(prev_cam, width, height, &old))
    return fail("the previous camera is singular or not finite");
  const Consts K = make_consts(cur, prev ? &old : nullptr, prev && same_camera(cam, prev_cam), params);
  const HostPrev P = prev ? HostPrev{prev->c, prev->v, prev->n, prev->X, prev->N}
                          : HostPrev{nullptr, nullptr, nullptr, nullptr, nullptr};
  for (int32_t y = 0; y < height; ++y)
    for (int32_t x = 0; x < width; ++x) {
      const size_t i = (size_t)y * width + x;
      const Pixel r = accumulate_pixel(rgb + 3 * i, se + 3 * i, albedo + 3 * i, normal + 3 * i, depth[i], x, y,
                                       width, height, K, P);
      for (int k = 0; k < 3; ++k) {
        rgb_out[3 * i + k] = r.rgb_out[k];
        se_out[3 * i + k] = r.se_out[k];
        if (hist) hist[3 * i + k] = r.hist[k];
        next->c[3 * i + k] = r.c[k];
        next->v[3 * i + k] = r.v[k];
        next->X[3 * i + k] = r.X[k];
        next->N[3 * i + k] = normal[3 * i + k];
      }
      if (n_out) n_out[i] = r.n;
      next->n[i] = r.n;
    }
  return SPT_OK;
}

// spt_guide_light.h — what the light guide (spt_guide_light.hip), its CPU statements
// (spt_guide_light_host.cpp, plain C++: it runs under the host sanitizers) and the context's launch
// (spt_context.cpp) share. Internal: the public statement is include/spt.h (SPT_HAS_GUIDE_LIGHT).
// Needs -ffp-contract=off on both sides.
#pragma once
#include "spt_film_math.h"
#include "spt_window_shape.h"

struct spt_light_guide : spt::WindowShape {
  long long* rec = nullptr;  // [rows * width][4], device
  size_t npix = 0;
  int32_t lanes_per_pixel = 0;  // K of the last launch
  uint32_t flags = 0;           // 0 or SPT_GUIDE_THROUGH_SPECULAR: where every pass takes its vertex
};

// spt_context.cpp: one light-guide launch over the sample window [s_base, s_base + s_count) into the
// records rec_dev (int64[rows * w][4], the shard's compact rows), through the context's scene upload, as
// spt_guide_window (spt_guide.h) does for a guide. flags: the light guide's.
spt_status spt_light_guide_window(spt_context* c, const spt_prim* prims, int32_t n_prims,
                                  const spt_camera* cam, const spt_params* p, int32_t s_base,
                                  int32_t s_count, long long* rec_dev, int32_t* lanes_out, int force_k,
                                  uint32_t flags, void* stream);
int spt_context_device(const spt_context* c);

namespace spt_light_math {

constexpr int kSlots = 4;  // tested 0, lit 1, weight 2 (1.31 sums), reserved 3

// The resolve of one record (spt.h). r and full are spt_film_math::resolve_factor(spp_total, n);
// n == 0 gives zeros.
SPT_FILM_FN void resolve_record(const long long* S, int64_t n, float r, int full, float* visibility,
                                float* direct, float* tested_share) {
  if (n <= 0) {
    *visibility = *direct = *tested_share = 0.0f;
    return;
  }
  const long long tested = S[0];
  *visibility = tested ? (float)((double)S[1] / (double)tested) : 0.0f;
  *tested_share = (float)((double)tested / (double)n);
  float f = (float)(unsigned long long)S[2] * 0x1p-31f;
  if (!full) f = f * r;
  *direct = f;
}

// The shading factor of the consumer (spt_light_shade_*): a multiply, then an add.
SPT_FILM_FN float shade_factor(float shade_floor, float visibility) {
  const float a = (1.0f - shade_floor) * visibility;
  return shade_floor + a;
}

inline bool shade_floor_ok(float f) { return f > 0.0f && f <= 1.0f; }  // (false for a NaN)

}  // namespace spt_light_math

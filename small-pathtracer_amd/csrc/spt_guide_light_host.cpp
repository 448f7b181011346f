// spt_guide_light_host.cpp — the light guide's resolve and the shade of an albedo plane as pure host
// functions (include/spt.h, SPT_HAS_GUIDE_LIGHT): the CPU statements the GPU tests compare the device
// kernels against. Plain C++, no HIP: it is also built into tests/probe/spt_guide_light_check under the
// host sanitizers.
#include "spt_guide_light.h"

extern "C" spt_status spt_light_guide_resolve_host(const int64_t* records, const spt_guide_info* info,
                                                   float* visibility, float* direct, float* tested) {
  if (!info || info->width < 0 || info->rows < 0 || info->spp_total < 1 || info->samples_done < 0 ||
      info->samples_done > info->spp_total)
    return spt::fail(SPT_ERR_INVALID_ARG, "spt_light_guide_resolve_host: bad info");
  const size_t npix = (size_t)info->rows * (size_t)info->width;
  if (npix != 0 && !records)
    return spt::fail(SPT_ERR_INVALID_ARG, "spt_light_guide_resolve_host: null records");
  int full = 0;
  const float r = spt_film_math::resolve_factor(info->spp_total, info->samples_done, &full);
  for (size_t i = 0; i < npix; ++i) {
    long long S[spt_light_math::kSlots];
    for (int k = 0; k < spt_light_math::kSlots; ++k) S[k] = (long long)records[spt_light_math::kSlots * i + k];
    float v, d, ts;
    spt_light_math::resolve_record(S, info->samples_done, r, full, &v, &d, &ts);
    if (visibility) visibility[i] = v;
    if (direct) direct[i] = d;
    if (tested) tested[i] = ts;
  }
  return SPT_OK;
}

extern "C" spt_status spt_light_shade_host(const float* albedo, const float* visibility, int64_t n_pixels,
                                           float shade_floor, float* out) {
  if (n_pixels < 0) return spt::fail(SPT_ERR_INVALID_ARG, "spt_light_shade: bad n_pixels");
  if (!spt_light_math::shade_floor_ok(shade_floor))
    return spt::fail(SPT_ERR_INVALID_ARG, "spt_light_shade: shade_floor must be in (0, 1]");
  if (n_pixels == 0) return SPT_OK;
  if (!albedo || !visibility || !out) return spt::fail(SPT_ERR_INVALID_ARG, "spt_light_shade: null plane");
  for (int64_t i = 0; i < n_pixels; ++i) {
    const float m = spt_light_math::shade_factor(shade_floor, visibility[i]);
    for (int k = 0; k < 3; ++k) out[3 * i + k] = albedo[3 * i + k] * m;  // (out may be albedo)
  }
  return SPT_OK;
}

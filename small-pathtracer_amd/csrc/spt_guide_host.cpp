// spt_guide_host.cpp — the guide's resolve as a pure host function (include/spt.h, SPT_HAS_GUIDE):
// the CPU statement every GPU guide test compares the device kernel against. Plain C++, no HIP: it
// is also built into tests/probe/spt_guide_check under the host sanitizers.
#include "spt_guide.h"

static_assert(sizeof(spt_guide_info) == 32, "spt_guide_info layout (the Python mirror's)");

extern "C" int32_t spt_guide_info_size(void) { return (int32_t)sizeof(spt_guide_info); }

extern "C" spt_status spt_guide_resolve_host(const int64_t* records, const spt_guide_info* info,
                                             float* albedo, float* normal, float* depth,
                                             float* coverage) {
  if (!info || info->width < 0 || info->rows < 0 || info->spp_total < 1 || info->samples_done < 0 ||
      info->samples_done > info->spp_total)
    return spt::fail(SPT_ERR_INVALID_ARG, "spt_guide_resolve_host: bad info");
  const size_t npix = (size_t)info->rows * (size_t)info->width;
  if (npix != 0 && !records) return spt::fail(SPT_ERR_INVALID_ARG, "spt_guide_resolve_host: null records");
  int full = 0;
  const float r = spt_film_math::resolve_factor(info->spp_total, info->samples_done, &full);
  for (size_t i = 0; i < npix; ++i) {
    long long S[spt_guide_math::kSlots];
    for (int k = 0; k < spt_guide_math::kSlots; ++k) S[k] = (long long)records[8 * i + k];
    float a[3], n[3], d, c;
    spt_guide_math::resolve_record(S, info->samples_done, r, full, a, n, &d, &c);
    for (int k = 0; k < 3; ++k) {
      if (albedo) albedo[3 * i + k] = a[k];
      if (normal) normal[3 * i + k] = n[k];
    }
    if (depth) depth[i] = d;
    if (coverage) coverage[i] = c;
  }
  return SPT_OK;
}

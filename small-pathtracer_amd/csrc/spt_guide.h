// spt_guide.h — what the guide (spt_guide.hip), its CPU statement (spt_guide_host.cpp, plain C++: it
// runs under the host sanitizers) and the context's guide launch (spt_context.cpp) share. Internal:
// the public statement is include/spt.h (SPT_HAS_GUIDE). Needs -ffp-contract=off on both sides.
#pragma once
#include "spt_film_math.h"
#include "spt_window_shape.h"

struct spt_guide : spt::WindowShape {
  long long* rec = nullptr;  // [rows * width][8], device
  size_t npix = 0;
  int32_t lanes_per_pixel = 0;  // K of the last launch
  uint32_t flags = 0;           // SPT_GUIDE_*: the kind of record every pass adds (set at creation)
};

// spt_context.cpp: one guide launch over the sample window [s_base, s_base + s_count) into the
// records rec_dev (int64[rows * w][8], the shard's compact rows), through the context's scene upload.
// *lanes_out = the lanes per pixel it ran with; force_k > 0 overrides the host's choice (a
// measurement's knob, not the ABI's). A shard without rows launches nothing. flags: the guide's
// (SPT_GUIDE_THROUGH_SPECULAR picks the chain instantiation of the kernel).
spt_status spt_guide_window(spt_context* c, const spt_prim* prims, int32_t n_prims,
                            const spt_camera* cam, const spt_params* p, int32_t s_base,
                            int32_t s_count, long long* rec_dev, int32_t* lanes_out, int force_k,
                            uint32_t flags, void* stream);
int spt_context_device(const spt_context* c);

namespace spt_guide_math {

constexpr int kSlots = 8;  // albedo 0-2, normal 3-5, depth 6, hits 7

// The resolve of one record (spt.h): out = albedo[3], normal[3], depth, coverage. r and full are
// spt_film_math::resolve_factor(spp_total, n); n == 0 gives zeros.
SPT_FILM_FN void resolve_record(const long long* S, int64_t n, float r, int full, float* albedo,
                                float* normal, float* depth, float* coverage) {
  if (n <= 0) {
    for (int k = 0; k < 3; ++k) albedo[k] = normal[k] = 0.0f;
    *depth = 0.0f;
    *coverage = 0.0f;
    return;
  }
  for (int k = 0; k < 3; ++k) {
    albedo[k] = spt_film_math::film_resolve1((unsigned long long)S[k], r, full);
    const long long v = S[3 + k];
    const unsigned long long mag = v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v;
    float f = (float)mag * 0x1p-31f;
    if (!full) f = f * r;
    normal[k] = v < 0 ? -f : f;
  }
  const long long hits = S[7];
  *depth = hits ? (float)((double)S[6] / ((double)hits * 65536.0)) : 0.0f;
  *coverage = (float)((double)hits / (double)n);
}

}  // namespace spt_guide_math

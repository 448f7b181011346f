// spt_window_shape.h — what a film (spt_film.h) and a guide (spt_guide.h) both are: a device plane
// over one shard's rows of a width x height image that takes sample windows of an spp_total-sample
// render. Internal and HIP-free (tests/probe/spt_window_check.cpp runs it under the host sanitizers).
#pragma once
#include "spt_status.h"

namespace spt {

struct WindowShape {
  int device = 0;
  int32_t width = 0, height = 0, rows = 0, spp_total = 0;
  // the shard the plane was created for (a pass must bring the same one); tile_rows is never 0 here
  int32_t tile_rows = 0, shard_index = 0, shard_count = 1;
  int64_t samples_done = 0;
};

// The create-time checks; *s = the empty plane of p's shard (s->device is the caller's to set).
inline spt_status shape_from_params(const spt_params* p, uint64_t max_pixels, WindowShape* s) {
  if (p->width <= 0 || p->height <= 0 || p->spp <= 0)
    return fail(SPT_ERR_INVALID_ARG, "width/height/spp must be positive");
  if ((uint64_t)p->width * (uint64_t)p->height > max_pixels)
    return fail(SPT_ERR_INVALID_ARG, "image too large for 32-bit pixel counters");
  if (p->shard_count < 1 || p->shard_index < 0 || p->shard_index >= p->shard_count || p->tile_rows < 0)
    return fail(SPT_ERR_INVALID_ARG, "bad shard_index/shard_count/tile_rows");
  s->width = p->width;
  s->height = p->height;
  s->rows = spt_shard_row_count(p);
  s->spp_total = p->spp;
  s->tile_rows = tile_rows_of(p);
  s->shard_index = p->shard_index;
  s->shard_count = p->shard_count;
  s->samples_done = 0;
  return SPT_OK;
}

// May the plane take the window [base, base + count) of a render with params p? noun: "film", "guide".
inline spt_status shape_accepts(const WindowShape& s, const spt_params* p, int32_t base, int32_t count,
                                const char* noun) {
  if (p->width != s.width || p->height != s.height || p->spp != s.spp_total)
    return fail(SPT_ERR_INVALID_ARG, std::string("width/height/spp differ from the ") + noun + "'s");
  if (p->tile_rows < 0 || tile_rows_of(p) != s.tile_rows || p->shard_index != s.shard_index ||
      p->shard_count != s.shard_count)
    return fail(SPT_ERR_INVALID_ARG, std::string("the shard fields differ from the ") + noun + "'s");
  if (base < 0 || count < 1 || (int64_t)base + count > s.spp_total)
    return fail(SPT_ERR_INVALID_ARG, "sample window outside [0, spp)");
  if (s.samples_done + count > s.spp_total)
    return fail(SPT_ERR_INVALID_ARG, std::string("the ") + noun + " would hold more than spp samples");
  return SPT_OK;
}

// Two planes over the same pixels. The sample counts and the shard fields may differ: a film and the
// guide it is denoised with are rendered with different spp.
inline bool shape_equal(const WindowShape& a, const WindowShape& b) {
  return a.width == b.width && a.rows == b.rows;
}

}  // namespace spt

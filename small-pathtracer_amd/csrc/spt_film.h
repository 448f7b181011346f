// spt_film.h — what spt_context.cpp (the render launch) and spt_film.hip (the film) share. Internal:
// the public statement is include/spt.h.
#pragma once
#include "spt_window_shape.h"

// The resumable integer film: the 1.31 fixed-point sums of the samples rendered so far, in image
// pixel order (the row layout of rgb_dev: a shard's film holds its compact rows).
struct spt_film : spt::WindowShape {
  unsigned long long* sums = nullptr;  // [rows * width][3], device
  size_t n = 0;                        // elements (3 * rows * width)
  spt_context* last_ctx = nullptr;     // the context of the last pass (it takes a guarded pass back)
  // the noise film (spt_film_noise_enable): every pass is one batch of `batch` samples
  int32_t batch = 0;                   // 0: a plain film
  int64_t batches_done = 0;
  unsigned long long* m2 = nullptr;    // [rows * width * 3][2]: (lo, hi) of the sum of P^2, device
  void* partials = nullptr;            // the summary's per-block partials and its result, device
  unsigned n_partials = 0;             // blocks of the summary's first stage
  // the adaptive film (spt_film_adaptive_enable): per-pixel batch counts and the active list. The
  // front is batches_done; samples_done stays front * batch.
  bool adaptive = false;
  bool any_retired = false;            // false: every pixel is active, passes take the unlisted path
  uint32_t* cnt = nullptr;             // [rows * width]: low 31 bits batches held, bit 31 retired
  // While nothing has retired every count is the front, so the unlisted passes do not touch the
  // plane; cnt_front is the front it was last written for (-1: never) and whoever reads the plane
  // brings it up first (sync_counts).
  int64_t cnt_front = -1;
  uint32_t* list = nullptr;            // [n_active] active pixels ascending (valid once any_retired)
  uint32_t* scan = nullptr;            // the compaction's per-block counts, then the total
  void* table = nullptr;               // NoiseArgs[b_max + 1] (spt_film_math.h), device
  int32_t b_max = 0;                   // spp_total / batch
  int64_t n_active = 0, samples_total = 0;
  int64_t last_pass_samples = 0;       // what the last pass added to samples_total (rollback)
  // the pooled error's scratch (spt.h SPT_HAS_FILM_POOL), allocated at the first pooled call:
  // planes u[3][npix] and h[3][npix] of doubles, then hn[npix] of uint32 (the row sums' counts)
  double* pool = nullptr;
};

// spt_context.cpp: one render launch over a sample window (film == nullptr: the one-shot finalize).
// list_dev != nullptr: the launch runs over the n_list local pixels of that ascending list (an
// adaptive film's pass); every size of the launch then comes from n_list.
spt_status spt_render_window(spt_context* c, const spt_prim* prims, int32_t n_prims,
                             const spt_camera* cam, const spt_params* p, int32_t s_base,
                             int32_t s_count, float* rgb_dev, spt_film* film, void* stream,
                             const uint32_t* list_dev = nullptr, uint32_t n_list = 0);
void spt_context_forget_film(spt_context* c, const spt_film* film);

// What the film takes from a render launch: the stolen-range sums, the unit slots and their layout,
// the statistics words (word 0: the runaway guard).
struct spt_film_launch {
  const unsigned long long* accum;
  const unsigned long long* slots;
  uint32_t npix, n_chunks, scr_k, scr_q;
  const unsigned long long* stats;
};

// spt_film.hip: enqueue the accumulate pass behind a render launch of `c` and count its s_count
// samples into the film. Once a pixel of an adaptive film has retired the launch is over the film's
// active list (npix = its length): virtual pixel v adds into pixel list[v], and that pixel's count
// goes up by one.
spt_status spt_film_accumulate(spt_film* film, spt_context* c, const spt_film_launch& launch,
                               float* rgb_dev, int32_t s_count, void* stream);
// The pass of `c` hit the runaway guard and added nothing: samples_done goes back by s_count.
void spt_film_rollback(spt_film* film, const spt_context* c, int32_t s_count);
void spt_film_forget_context(spt_film* film, const spt_context* c);

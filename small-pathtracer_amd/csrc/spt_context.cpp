// spt_context.cpp — the render path's HIP runtime calls: contexts (create / reserve / destroy), one
// launch over a sample window (spt_render_window), the statistics, and the one-shot drop-in
// (spt_render). What to launch and how it is sized is decided in spt_dispatch.cpp; the kernels and
// their launchers are spt_kernel.hip (the render) and spt_guide.hip (the guide), through spt_launch.h.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>

#include "../../include/spt.h"
#include "../../include/spt_flops.h"
#include "spt_diag.h"
#include "spt_film.h"
#include "spt_guide.h"
#include "spt_guide_light.h"
#include "spt_launch.h"

using namespace spt;

struct spt_context {
  int device = 0;
  int n_cu = 0, blocks_per_cu = 0;      // generic kernel
  int bpc[KV_COUNT] = {};               // resident blocks per CU of each variant
  DevPrim* prims = nullptr;
  SceneGeo* geo = nullptr;
  unsigned long long* accum = nullptr;
  size_t accum_cap = 0;  // elements
  unsigned long long* slots = nullptr;  // [n_units][3] unit slots, grown on demand
  size_t slots_cap = 0;                 // elements
  uint32_t* queue = nullptr;
  unsigned long long* stats = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // the launch's statistics words, copied to pinned host memory on the launch's stream after the
  // finalize (ev2 marks the copy): spt_context_stats() waits for that launch only, never for work
  // queued behind it on the stream
  unsigned long long* h_stats = nullptr;
  hipEvent_t ev2 = nullptr;
  bool pending = false;
  bool launched = false;  // a render has been enqueued (spt_context_stats has events to read)
  int n_prims = 0;
  // Pinned staging for the async scene upload; reused only after the previous upload completed.
  DevPrim* h_prims = nullptr;
  SceneGeo* h_geo = nullptr;
  KParams* d_kp = nullptr;   // kernel parameters in device memory (read via s_load)
  KParams* h_kp = nullptr;   // pinned staging
  uint64_t samples = 0;      // pixel-samples of the last render (exact, not counted in-kernel)
  bool nee_by_identity = false;  // the last kernel derives nee_events from vertices - samples
  int last_kv = -1;          // variant of the last launch (-1: none yet, or a shard without rows)
  double scene_flop = 0;     // FLOP-model cost of one ray against the scene
  spt_film* last_film = nullptr;  // the film of the last launch (nullptr: a plain render)
  int32_t last_film_count = 0;    // ... and the samples that pass added to its samples_done
  // A guide pass (spt_guide_window) goes through the same scene upload and staging but is no render:
  // it has its own upload event, and leaves everything above alone (stats, last_kv, the film).
  hipEvent_t ev_guide = nullptr;
  bool guide_pending = false;     // the staging may still be read by a guide pass's upload
  int guide_bpc[4] = {0, 0, 0, 0};  // resident blocks per CU of the guide kernels ([chain * 2 + wide]); 0: not asked yet
  int light_bpc[4] = {0, 0, 0, 0};  // ... and of the light-guide kernels
};

// ---- spt_status.h's two helpers that call HIP
spt_status spt::open_device(int32_t device, bool say_why) {
  int count = 0;
  const hipError_t ce = hipGetDeviceCount(&count);
  if (ce != hipSuccess || count == 0)
    return fail(SPT_ERR_NO_DEVICE,
                say_why ? std::string("no HIP device (") + hipGetErrorString(ce) + ")" : "no HIP device");
  if (device < 0 || device >= count) return fail(SPT_ERR_INVALID_ARG, "bad device ordinal");
  SPT_HIP(hipSetDevice(device));
  return SPT_OK;
}

spt_status spt::copy_and_wait(int device, void* dst, const void* src, size_t bytes, int kind,
                              void* stream) {
  SPT_HIP(hipSetDevice(device));
  SPT_HIP(hipMemcpyAsync(dst, src, bytes, (hipMemcpyKind)kind, (hipStream_t)stream));
  SPT_HIP(hipStreamSynchronize((hipStream_t)stream));
  return SPT_OK;
}

// Variant of the calling thread's last spt_render() launch (the one-shot call owns its context).
static thread_local int g_dropin_kv = -1;

extern "C" const char* spt_context_kernel(spt_context* c) {
  const int kv = c ? c->last_kv : g_dropin_kv;
  return spt_kernel_name(kv);
}

extern "C" spt_status spt_context_create(int32_t device, spt_context** out) {
  if (!out) return fail(SPT_ERR_INVALID_ARG, "null out");
  SPT_TRY(open_device(device));
  hipDeviceProp_t prop;
  SPT_HIP(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(SPT_ERR_NO_DEVICE, std::string("built for gfx950, device is ") + prop.gcnArchName);
  spt_context* c = new spt_context();
  c->device = device;
  c->n_cu = prop.multiProcessorCount;
  for (int v = 0; v < KV_COUNT; ++v) {
    const int bpc = render_kernel_occupancy(v);
    c->bpc[v] = bpc > 0 ? bpc : 4;
  }
  c->blocks_per_cu = c->bpc[KV_GENERIC];

  hipError_t e = hipMalloc(&c->prims, sizeof(DevPrim) * kMaxPrims);
  if (e == hipSuccess) e = hipMalloc(&c->geo, sizeof(SceneGeo));
  if (e == hipSuccess) e = hipHostMalloc(&c->h_prims, sizeof(DevPrim) * kMaxPrims, hipHostMallocDefault);
  if (e == hipSuccess) e = hipHostMalloc(&c->h_geo, sizeof(SceneGeo), hipHostMallocDefault);
  if (e == hipSuccess) e = hipMalloc(&c->d_kp, sizeof(KParams));
  if (e == hipSuccess) e = hipHostMalloc(&c->h_kp, sizeof(KParams), hipHostMallocDefault);

  if (e == hipSuccess) e = hipMalloc(&c->queue, sizeof(uint32_t) * 64);
  if (e == hipSuccess) e = hipMalloc(&c->stats, sizeof(unsigned long long) * kStatWords);
  if (e == hipSuccess) e = hipEventCreate(&c->ev0);
  if (e == hipSuccess) e = hipEventCreate(&c->ev1);
  if (e == hipSuccess) e = hipEventCreate(&c->ev2);
  if (e == hipSuccess) e = hipHostMalloc(&c->h_stats, sizeof(unsigned long long) * kStatWords, hipHostMallocDefault);
  if (e == hipSuccess) std::memset(c->h_stats, 0, sizeof(unsigned long long) * kStatWords);  // stats before any launch: zeros
  if (e != hipSuccess) {
    spt_context_destroy(c);
    return fail(SPT_ERR_OOM, std::string("context alloc: ") + hipGetErrorString(e));
  }
  *out = c;
  return SPT_OK;
}

extern "C" spt_status spt_context_destroy(spt_context* c) {
  if (!c) return SPT_OK;
  (void)hipSetDevice(c->device);
  if (c->prims) (void)hipFree(c->prims);
  if (c->geo) (void)hipFree(c->geo);
  if (c->h_prims) (void)hipHostFree(c->h_prims);
  if (c->h_geo) (void)hipHostFree(c->h_geo);
  if (c->d_kp) (void)hipFree(c->d_kp);
  if (c->h_kp) (void)hipHostFree(c->h_kp);

  if (c->accum) (void)hipFree(c->accum);
  if (c->slots) (void)hipFree(c->slots);
  if (c->queue) (void)hipFree(c->queue);
  if (c->stats) (void)hipFree(c->stats);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->ev2) (void)hipEventDestroy(c->ev2);
  if (c->ev_guide) (void)hipEventDestroy(c->ev_guide);
  if (c->h_stats) (void)hipHostFree(c->h_stats);
  if (c->last_film) spt_film_forget_context(c->last_film, c);
  delete c;
  return SPT_OK;
}

extern "C" spt_status spt_context_reserve(spt_context* c, int32_t n_prims, const spt_params* p) {
  if (!c || !p) return fail(SPT_ERR_INVALID_ARG, "null argument");
  (void)n_prims;
  const size_t need = 3ull * (size_t)spt_shard_row_count(p) * (size_t)p->width;
  if (need > c->accum_cap) {
    SPT_HIP(hipSetDevice(c->device));
    if (c->accum) SPT_HIP(hipFree(c->accum));
    c->accum = nullptr;
    c->accum_cap = 0;
    SPT_HIP(hipMalloc(&c->accum, need * sizeof(unsigned long long)));
    c->accum_cap = need;
  }
  return SPT_OK;
}

// The film of the context's last launch and that film's last context name each other and nobody
// else, so whichever is destroyed first can tell the other (spt_film_forget_context).
static void set_last_film(spt_context* c, spt_film* film, int32_t count) {
  if (c->last_film && c->last_film != film) spt_film_forget_context(c->last_film, c);
  c->last_film = film;
  c->last_film_count = count;
}

// ---- The scene staging both windows go through. A window call runs in three steps: every host-side
// rejection (validate, the window check, stage_scene, select_variant, the list check, plan_launch);
// then the allocations; then the stream operations. A call that returns an error from the first step
// has queued nothing and allocated nothing.

// Wait until nobody reads the pinned staging, then state the scene in it and in *K: the primitives and
// their grouping, the fields of KParams that do not depend on the launch's sizes.
static spt_status stage_scene(spt_context* c, const spt_prim* prims, int32_t n_prims, const spt_params* p,
                              int32_t s_base, int32_t s_count, KParams* K, int* light_pos) {
  if (c->pending) SPT_HIP(hipEventSynchronize(c->ev0));  // staging still read by a prior upload
  if (c->guide_pending) SPT_HIP(hipEventSynchronize(c->ev_guide));  // ... or by a guide pass's
  c->guide_pending = false;
  to_dev(prims, n_prims, c->h_prims);
  build_geo(prims, n_prims, c->h_geo, p->light_id, light_pos);
  K->prims = c->prims;
  K->geo = c->geo;
  K->n_prims = n_prims;
  K->width = p->width; K->height = p->height; K->spp = p->spp;
  K->s_base = (uint32_t)s_base; K->s_count = (uint32_t)s_count; K->s_lim = (uint32_t)(s_base + s_count);
  K->seed = p->seed;
  // Ray-direction contract (oracle c_unit_dirs): unit directions iff a sphere or a REFR primitive
  K->unit_dirs = 0;
  for (int i = 0; i < n_prims; ++i)
    if (prims[i].kind == SPT_SPHERE || prims[i].refl == SPT_REFR) K->unit_dirs = 1;
  return SPT_OK;
}

// The staged scene, then (behind whatever the caller enqueues in between) the kernel parameters and
// the event that says the staging has been read. The caller sets pending / guide_pending.
static spt_status upload_scene(spt_context* c, int32_t n_prims, hipStream_t stream) {
  SPT_HIP(hipMemcpyAsync(c->prims, c->h_prims, sizeof(DevPrim) * n_prims, hipMemcpyHostToDevice,
                         stream));
  SPT_HIP(hipMemcpyAsync(c->geo, c->h_geo, sizeof(SceneGeo), hipMemcpyHostToDevice, stream));
  return SPT_OK;
}

static spt_status upload_params(spt_context* c, const KParams& K, hipEvent_t event, hipStream_t stream) {
  *c->h_kp = K;
  SPT_HIP(hipMemcpyAsync(c->d_kp, c->h_kp, sizeof(KParams), hipMemcpyHostToDevice, stream));
  SPT_HIP(hipEventRecord(event, stream));
  return SPT_OK;
}

// One launch over the sample window [s_base, s_base + s_count) of the p->spp-sample image. With
// film == nullptr the window's sums become the clamped floats of rgb_dev (finalize_slots_kernel:
// the one-shot render, window [0, spp)); with a film they are added to it (spt_film.hip) and
// rgb_dev, if given, receives the film resolved after the pass. Every size of the launch comes
// from s_count; the fixed-point scale stays 2^31 / p->spp, so the windows' integers sum to the
// one-shot's.
spt_status spt_render_window(spt_context* c, const spt_prim* prims, int32_t n_prims,
                             const spt_camera* cam, const spt_params* p, int32_t s_base,
                             int32_t s_count, float* rgb_dev, spt_film* film, void* stream_v,
                             const uint32_t* list_dev, uint32_t n_list) {
  if (!c || (!rgb_dev && !film)) return fail(SPT_ERR_INVALID_ARG, "null context/output");
  if (list_dev && (!film || n_list == 0))
    return fail(SPT_ERR_INVALID_ARG, "a pixel list needs a film and at least one pixel");
  SPT_TRY(validate(prims, n_prims, cam, p));
  if (s_base < 0 || s_count < 1 || (int64_t)s_base + s_count > p->spp)
    return fail(SPT_ERR_INVALID_ARG, "sample window outside [0, spp)");
  if (film && film->device != c->device)
    return fail(SPT_ERR_INVALID_ARG, "the film and the context are on different devices");
  SPT_HIP(hipSetDevice(c->device));
  hipStream_t stream = (hipStream_t)stream_v;

  KParams K{};
  int light_pos = -1;
  SPT_TRY(stage_scene(c, prims, n_prims, p, s_base, s_count, &K, &light_pos));
  K.nee_prob = p->nee_prob; K.rr_depth = p->rr_depth; K.max_depth = p->max_depth;
  K.light_id = p->light_id;
  K.lx0 = p->light_x0; K.ldx = p->light_dx; K.lz0 = p->light_z0; K.ldz = p->light_dz;
  K.ly = p->light_y; K.larea = p->light_area; K.light_mode = p->light_mode;
  const int rows = spt_shard_row_count(p);
  if (rows == 0) {  // a shard that owns no rows (more shards than row tiles): nothing to render
    c->samples = 0;
    c->nee_by_identity = false;
    c->last_kv = -1;
    set_last_film(c, nullptr, 0);
    c->scene_flop = 0;
    SPT_HIP(hipMemsetAsync(c->stats, 0, sizeof(unsigned long long) * kStatWords, stream));
    SPT_HIP(hipEventRecord(c->ev0, stream));
    SPT_HIP(hipEventRecord(c->ev1, stream));
    SPT_HIP(hipMemcpyAsync(c->h_stats, c->stats, sizeof(unsigned long long) * kStatWords,
                           hipMemcpyDeviceToHost, stream));
    SPT_HIP(hipEventRecord(c->ev2, stream));
    c->pending = true;
    c->launched = true;
    return SPT_OK;
  }
  // the kernel variant, with the fp32 camera, the early-resolve clauses and the leak-end rule it
  // runs under; then the launch's sizes (both spt_dispatch.cpp)
  const int kv = select_variant(prims, n_prims, cam, p, *c->h_geo, light_pos, &K);
  LaunchPlan plan;
  // over a pixel list the launch's local pixels are the virtual indices [0, n_list)
  if (list_dev && (uint64_t)n_list > (uint64_t)rows * (uint64_t)p->width)
    return fail(SPT_ERR_INVALID_ARG, "the pixel list is longer than the shard");
  K.pix_list = list_dev;
  SPT_TRY(plan_launch(c->n_cu, c->bpc[kv], kv, p, s_count, list_dev ? (int)n_list : rows * p->width, &K,
                      &plan));
  // nothing below rejects the call: the allocations, then the stream
  SPT_TRY(spt_context_reserve(c, n_prims, p));
  const size_t n_units = K.n_units;
  K.accum = c->accum;
  if (3ull * n_units > c->slots_cap) {  // one owner store per unit (24 B): C3 208 MB, C4/C5 ~400 MB
    if (c->slots) SPT_HIP(hipFree(c->slots));
    c->slots = nullptr;
    c->slots_cap = 0;
    SPT_HIP(hipMalloc(&c->slots, 3ull * n_units * sizeof(unsigned long long)));
    c->slots_cap = 3ull * n_units;
  }
  K.slots = c->slots;
  K.queue = c->queue;
  K.stats = c->stats;
  K.light_kind = light_pos >= 0 ? prims[p->light_id].kind : 0;
  K.light_pos = light_pos;
  K.scatter_uniform = (p->flags & SPT_FLAG_UNIFORM_SCATTER) ? 1 : 0;
  K.nee_c = (float)((double)p->light_area / 3.14159265358979323846);
  c->n_prims = n_prims;
  c->samples = (uint64_t)K.n_local_pix * (uint64_t)s_count;
  c->scene_flop = 0;
  for (int i = 0; i < n_prims; ++i)
    c->scene_flop += prims[i].kind == SPT_SPHERE ? SPT_FLOP_SPHERE : SPT_FLOP_RECT;

  SPT_TRY(upload_scene(c, n_prims, stream));
  SPT_HIP(hipMemsetAsync(c->accum, 0, sizeof(unsigned long long) * 3 * (size_t)K.n_local_pix,
                         stream));
  SPT_HIP(hipMemsetAsync(c->queue, 0, sizeof(uint32_t), stream));
  SPT_HIP(hipMemsetAsync(c->stats, 0, sizeof(unsigned long long) * kStatWords, stream));
#ifdef SPT_WAVE_TIMES
  SPT_HIP(hipMemsetAsync(c->stats + 14, 0xFF, sizeof(unsigned long long), stream));
#endif
  c->nee_by_identity = kKernelInfo[kv].nee_by_identity;
  SPT_TRY(upload_params(c, K, c->ev0, stream));
  launch_render_kernel(kv, plan.grid, c->d_kp, stream, list_dev != nullptr);
  SPT_HIP(hipGetLastError());
  SPT_HIP(hipEventRecord(c->ev1, stream));
  const uint32_t np = (uint32_t)K.n_local_pix;
  if (film) {  // add the window's sums to the film (and resolve it into rgb_dev, if given)
    const spt_film_launch launch{c->accum, c->slots, np, plan.n_chunks, K.scr_k, K.scr_q, c->stats};
    SPT_TRY(spt_film_accumulate(film, c, launch, rgb_dev, s_count, stream));
  } else {
    launch_finalize_slots(c->accum, c->slots, rgb_dev, np, plan.n_chunks, K.scr_k, K.scr_q, c->stats,
                          stream);
    SPT_HIP(hipGetLastError());
  }
  set_last_film(c, film, film ? s_count : 0);
  SPT_HIP(hipMemcpyAsync(c->h_stats, c->stats, sizeof(unsigned long long) * kStatWords,
                         hipMemcpyDeviceToHost, stream));
  SPT_HIP(hipEventRecord(c->ev2, stream));
  c->pending = true;
  c->launched = true;
  c->last_kv = kv;
  return SPT_OK;
}

// One guide launch over the sample window (spt_guide.h): the context's scene upload and staging, the
// guide kernel, the records of `rec_dev` (int64[rows * w][8]) updated in place. The context's render
// state -- statistics, last kernel, last film, the events spt_context_stats reads -- is not touched.
// force_k > 0 (a measurement's override, never the ABI's): that many lanes per pixel.
// light: the light guide's launch (spt_guide_light.h) -- the same pass with the light-guide kernel, the
// records int64[rows * w][4] and the light's parameters as a render sets them.
static spt_status guide_window(spt_context* c, const spt_prim* prims, int32_t n_prims,
                               const spt_camera* cam, const spt_params* p, int32_t s_base,
                               int32_t s_count, long long* rec_dev, int32_t* lanes_out, int force_k,
                               uint32_t flags, bool light, void* stream_v) {
  if (!c || !rec_dev) return fail(SPT_ERR_INVALID_ARG, "null context/guide");
  SPT_TRY(validate(prims, n_prims, cam, p));
  if (s_base < 0 || s_count < 1 || (int64_t)s_base + s_count > p->spp)
    return fail(SPT_ERR_INVALID_ARG, "sample window outside [0, spp)");
  const int rows = spt_shard_row_count(p);
  if (rows == 0) return SPT_OK;
  SPT_HIP(hipSetDevice(c->device));
  hipStream_t stream = (hipStream_t)stream_v;

  KParams K{};
  int light_pos = -1;
  SPT_TRY(stage_scene(c, prims, n_prims, p, s_base, s_count, &K, &light_pos));
  const bool wide = c->h_geo->n_sph_wide > 0;
  const bool chain = (flags & SPT_GUIDE_THROUGH_SPECULAR) != 0;
  int& guide_bpc = (light ? c->light_bpc : c->guide_bpc)[(chain ? 2 : 0) + (wide ? 1 : 0)];  // of the instantiation launched
  if (guide_bpc == 0) {
    const int bpc = light ? light_guide_kernel_occupancy(wide, chain) : guide_kernel_occupancy(wide, chain);
    guide_bpc = bpc > 0 ? bpc : 4;
  }
  // the fp32 camera and the launch's terms (shard, magic divisors, fixed-point scale, camera chain)
  // as a render of the scene's run-time kernel would set them; the unit and queue sizes are unused
  (void)select_variant(prims, n_prims, cam, p, *c->h_geo, light_pos, &K);
  LaunchPlan plan;
  spt_params q = *p;
  q.chunk = s_count;  // one unit per pixel: never "too many work units"
  SPT_TRY(plan_launch(c->n_cu, guide_bpc, wide ? KV_WIDE : KV_GENERIC, &q, s_count, rows * p->width, &K,
                      &plan));
  int k = force_k > 0 ? force_k : guide_lanes_per_pixel(c->n_cu, guide_bpc, K.n_local_pix, s_count);
  uint32_t ksh = 0;
  while ((1 << (ksh + 1)) <= k && ksh < 6) ++ksh;
  k = 1 << ksh;
  const uint64_t lanes = (uint64_t)K.n_local_pix << ksh;
  const uint64_t grid = (lanes + kBlock - 1) / kBlock;
  if (grid >= 0x7FFFFFFFull) return fail(SPT_ERR_INVALID_ARG, "the guide launch is too large");
  // nothing below rejects the call
  if (!c->ev_guide) SPT_HIP(hipEventCreate(&c->ev_guide));
  if (light) {
    K.light_rec = rec_dev;
    K.light_kshift = ksh;
    K.light_id = p->light_id;
    K.lx0 = p->light_x0; K.ldx = p->light_dx; K.lz0 = p->light_z0; K.ldz = p->light_dz;
    K.ly = p->light_y; K.larea = p->light_area;
    K.nee_c = (float)((double)p->light_area / 3.14159265358979323846);
  } else {
    K.guide_rec = rec_dev;
    K.guide_kshift = ksh;
  }
  SPT_TRY(upload_scene(c, n_prims, stream));
  SPT_TRY(upload_params(c, K, c->ev_guide, stream));
  c->guide_pending = true;
  if (light) launch_light_guide_kernel(wide, chain, (int)grid, c->d_kp, stream);
  else launch_guide_kernel(wide, chain, (int)grid, c->d_kp, stream);
  SPT_HIP(hipGetLastError());
  if (lanes_out) *lanes_out = k;
  return SPT_OK;
}

spt_status spt_guide_window(spt_context* c, const spt_prim* prims, int32_t n_prims,
                            const spt_camera* cam, const spt_params* p, int32_t s_base,
                            int32_t s_count, long long* rec_dev, int32_t* lanes_out, int force_k,
                            uint32_t flags, void* stream) {
  return guide_window(c, prims, n_prims, cam, p, s_base, s_count, rec_dev, lanes_out, force_k, flags, false,
                      stream);
}

spt_status spt_light_guide_window(spt_context* c, const spt_prim* prims, int32_t n_prims,
                                  const spt_camera* cam, const spt_params* p, int32_t s_base,
                                  int32_t s_count, long long* rec_dev, int32_t* lanes_out, int force_k,
                                  uint32_t flags, void* stream) {
  return guide_window(c, prims, n_prims, cam, p, s_base, s_count, rec_dev, lanes_out, force_k, flags, true,
                      stream);
}

int spt_context_device(const spt_context* c) { return c ? c->device : -1; }

extern "C" spt_status spt_render_async(spt_context* c, const spt_prim* prims, int32_t n_prims,
                                       const spt_camera* cam, const spt_params* p, float* rgb_dev,
                                       void* stream) {
  if (!c || !rgb_dev) return fail(SPT_ERR_INVALID_ARG, "null context/output");
  if (!p) return fail(SPT_ERR_INVALID_ARG, "null argument");
  return spt_render_window(c, prims, n_prims, cam, p, 0, p->spp, rgb_dev, nullptr, stream);
}

// A film whose last pass this context rendered is going away (spt_film_destroy).
void spt_context_forget_film(spt_context* c, const spt_film* film) {
  if (c && c->last_film == film) c->last_film = nullptr;
}

extern "C" spt_status spt_context_stats(spt_context* c, spt_stats* out) {
  if (!c || !out) return fail(SPT_ERR_INVALID_ARG, "null argument");
  if (!c->launched) return fail(SPT_ERR_INVALID_ARG, "no render has been enqueued on this context");
  SPT_HIP(hipSetDevice(c->device));
  SPT_HIP(hipEventSynchronize(c->ev2));
  const unsigned long long* h = c->h_stats;
#ifdef SPT_WAVE_TIMES
  std::fprintf(stderr, "SPT_WAVE_TIMES sum=%llu sumsq=%llu first=%llu last=%llu iters=%llu maxiters=%llu "
               "sumstart16=%llu sumend16=%llu smid=%llu\n",
               h[12], h[13], h[14], h[15], h[16], h[17], h[18], h[19], h[20]);
  if (const char* path = std::getenv("SPT_WAVE_DUMP")) {  // diagnostic build only
    if (FILE* f = std::fopen(path, "wb")) {
      std::fwrite(h + 32, sizeof(unsigned long long), 3 * 32768, f);
      std::fclose(f);
    }
  }
#endif
#ifdef SPT_REGION_STATS
  {
    static const char* names[10] = {"iteration", "unit_retire", "refill", "camera", "path_isect",
                                    "diff_shading", "shadow_test", "nee_light_hit", "cosine",
                                    "path_end"};
    std::fprintf(stderr, "SPT_REGION_STATS");
    for (int r = 0; r < 10; ++r)
      std::fprintf(stderr, " %s=%llu/%llu", names[r], h[kStatRegion + 2 * r],
                   h[kStatRegion + 1 + 2 * r]);
    std::fprintf(stderr, "\n");
  }
#endif
  if (h[0] != 0) {
    c->pending = false;
    // a film pass that hit the guard added nothing (spt_film.hip): take its samples back
    if (c->last_film) spt_film_rollback(c->last_film, c, c->last_film_count);
    set_last_film(c, nullptr, 0);
    return fail(SPT_ERR_HIP, "render kernel hit its iteration cap in " + std::to_string(h[0]) +
                                 " waves (a path did not terminate); the image is incomplete");
  }
  float ms = 0.0f;
  SPT_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  std::memset(out, 0, sizeof *out);
  out->samples = c->samples; out->path_rays = h[1]; out->shadow_rays = h[2]; out->vertices = h[3];
  out->nee_events = h[4]; out->nee_light_hits = h[5]; out->cosine_samples = h[6];
  out->misses = h[7];
  out->shadow_traced = h[kStatShadowTraced];
  out->sphere_vertices = h[kStatSphereVertices];
  out->shadow_proven = h[kStatShadowProven];
  if (c->nee_by_identity) {  // HEAD NEE kernels: one NEE event per non-terminal vertex
    out->nee_events = out->vertices - out->samples;
    out->shadow_rays = out->nee_events;
  }
  // FLOP model (include/spt_flops.h): scene cost per ray from the primitive mix. `flop` charges
  // a full scene test for every shadow ray of the reference (:466); `flop_executed` only for the
  // shadow rays the kernel traced (the others are rejected exactly by the light pre-test or
  // resolved by early_nee_proven()).
  const double scene = c->scene_flop;
  const double common = (double)out->samples * SPT_FLOP_SAMPLE +
                        (double)out->path_rays * scene + (double)out->vertices * SPT_FLOP_VERTEX +
                        (double)out->sphere_vertices * SPT_FLOP_SPHERE_NORMAL +
                        (double)(out->vertices - out->samples) * SPT_FLOP_COMBINE +
                        (double)out->cosine_samples * SPT_FLOP_COSINE +
                        (double)out->nee_events * SPT_FLOP_NEE +
                        (double)out->nee_light_hits * SPT_FLOP_NEE_HIT;
  out->flop = common + (double)out->shadow_rays * scene;
  out->flop_executed = common + (double)(out->shadow_traced - out->shadow_proven) * scene;
  out->kernel_ms = ms;
  c->pending = false;
  return SPT_OK;
}

// The one-shot drop-in (spt_render) keeps one context and one device output buffer per device for
// the life of the process (or until spt_shutdown), so a caller that renders repeatedly -- the
// reference's main() replaced by smallpt_amd, or a Python loop over spt.render -- pays context
// creation, the unit-slot allocation (~200 MB at C3) and the cold first launch once, not per call.
// Calls on one device are serialised by that device's mutex; different devices run concurrently.
namespace {
constexpr int kMaxDropInDevices = 64;
struct DropIn {
  std::mutex mu;
  spt_context* ctx = nullptr;
  float* out = nullptr;  // device output, grown on demand
  size_t out_cap = 0;    // floats
};
DropIn g_dropin[kMaxDropInDevices];
}  // namespace

extern "C" spt_status spt_render(const spt_prim* prims, int32_t n_prims, const spt_camera* cam,
                                 const spt_params* p, float* rgb_out, spt_stats* stats) {
  if (!rgb_out) return fail(SPT_ERR_INVALID_ARG, "null rgb_out");
  SPT_TRY(validate(prims, n_prims, cam, p));
  if (p->device < 0 || p->device >= kMaxDropInDevices) return fail(SPT_ERR_INVALID_ARG, "bad device ordinal");
  const size_t n = 3ull * (size_t)spt_shard_row_count(p) * (size_t)p->width;
  g_dropin_kv = -1;
  if (n == 0) {  // this shard owns no rows: nothing to render, no context or device memory
    if (stats) std::memset(stats, 0, sizeof *stats);
    return SPT_OK;
  }
  DropIn& D = g_dropin[p->device];
  std::lock_guard<std::mutex> lock(D.mu);
  if (!D.ctx) SPT_TRY(spt_context_create(p->device, &D.ctx));  // (leaves D.ctx null when it fails)
  SPT_HIP(hipSetDevice(p->device));
  if (n > D.out_cap) {
    if (D.out) SPT_HIP(hipFree(D.out));
    D.out = nullptr;
    D.out_cap = 0;
    SPT_HIP(hipMalloc(&D.out, n * sizeof(float)));
    D.out_cap = n;
  }
  SPT_TRY(spt_render_async(D.ctx, prims, n_prims, cam, p, D.out, nullptr));
  g_dropin_kv = D.ctx->last_kv;
  spt_stats tmp;
  SPT_TRY(spt_context_stats(D.ctx, stats ? stats : &tmp));
  SPT_HIP(hipMemcpy(rgb_out, D.out, n * sizeof(float), hipMemcpyDeviceToHost));
  return SPT_OK;
}

extern "C" spt_status spt_shutdown(void) {
  for (DropIn& D : g_dropin) {
    std::lock_guard<std::mutex> lock(D.mu);
    if (D.ctx) {
      const int dev = D.ctx->device;
      spt_context_destroy(D.ctx);
      D.ctx = nullptr;
      if (D.out) {
        (void)hipSetDevice(dev);
        (void)hipFree(D.out);
      }
    }
    D.out = nullptr;
    D.out_cap = 0;
  }
  return SPT_OK;
}

extern "C" int32_t spt_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}


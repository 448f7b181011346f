// spt_temporal.hip — temporal accumulation on the device (include/spt.h, SPT_HAS_TEMPORAL): the
// accumulator object that owns the two copies of the state and the film path's planes, the kernel and the
// spt_temporal_* / spt_film_temporal_accumulate calls. The arithmetic is spt_temporal.h's, shared with the
// CPU statement (spt_temporal_host.cpp): the kernel only decides which lane takes which pixel and how the
// state is packed. A pixel's state is three 16-byte words, (N, n), (X, v_0), (c, v_1), and one float, v_2:
// a tap's validity tests read the first two words, a valid tap the rest.
#include <hip/hip_runtime.h>

#include <vector>

#include "spt_film.h"
#include "spt_guide.h"
#include "spt_status.h"
#include "spt_temporal.h"

using namespace spt_temporal_math;
using spt::fail;
using spt_denoise_math::inputs_error;
using spt_denoise_math::outputs_error;
using spt_denoise_math::PlaneList;
using spt_denoise_math::size_error;

namespace {

// One copy of the state, packed.
struct Packed {
  f4 *p0 = nullptr, *p1 = nullptr, *p2 = nullptr;  // (N, n), (X, v_0), (c, v_1)
  float* v2 = nullptr;
};

}  // namespace

struct spt_temporal {
  int device = 0;
  int32_t width = 0, height = 0;
  size_t npix = 0;
  void* base = nullptr;  // the one allocation everything below is carved from
  Packed st[2];          // the ping-pong copies: st[cur] holds the last frame's state
  // the film path's planes (spt_film_temporal_accumulate): rgb, se, albedo, normal (3 floats each), depth (1)
  float *rgb = nullptr, *se = nullptr, *albedo = nullptr, *normal = nullptr, *depth = nullptr;
  int cur = 0;
  int64_t frames = 0;  // since the last reset
  spt_camera cam;      // of the last frame, and its constants
  CamConsts cam_consts;
};

namespace {

// The accumulation's tiling: 64 x 4 pixels, 256 lanes; a wave covers 64 consecutive x.
constexpr int kTileX = 64, kTileY = 4, kBlock = kTileX * kTileY;
constexpr size_t kMaxTiles = 0xFFFFFFFFull / kBlock;

size_t tiles_of(int32_t w, int32_t h) {
  return (((size_t)w + kTileX - 1) / kTileX) * (((size_t)h + kTileY - 1) / kTileY);
}

// The previous state as the device holds it.
struct DevPrev {
  const f4 *p0, *p1, *p2;
  const float* v2;
  __device__ __forceinline__ TapGeom geom(size_t i) const {
    const f4 a = p0[i], b = p1[i];
    return TapGeom{{a.x, a.y, a.z}, a.w, {b.x, b.y, b.z}};
  }
  __device__ __forceinline__ TapColour colour(size_t i) const {
    const f4 b = p1[i], c = p2[i];
    return TapColour{{c.x, c.y, c.z}, {b.w, c.w, v2[i]}};
  }
};

// One lane per pixel: five planes and the previous state in, the outputs and the next state out. Blocks
// are a 1-D grid over the tiles, rows of tiles first. No tap address is formed before accumulate_pixel's
// range checks; a lane outside the image leaves at once.
__global__ void __launch_bounds__(kBlock)
temporal_accumulate_kernel(const float* __restrict__ rgb, const float* __restrict__ se,
                           const float* __restrict__ albedo, const float* __restrict__ normal,
                           const float* __restrict__ depth, int32_t w, int32_t h, Consts K, DevPrev prev,
                           f4* __restrict__ o0, f4* __restrict__ o1, f4* __restrict__ o2, float* __restrict__ ov2,
                           float* __restrict__ rgb_out, float* __restrict__ se_out, float* __restrict__ n_out,
                           float* __restrict__ hist) {
  const uint32_t tiles_x = ((uint32_t)w + kTileX - 1) / kTileX;
  const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int32_t x = (int32_t)(tx * kTileX + (threadIdx.x & (kTileX - 1)));
  const int32_t y = (int32_t)(ty * kTileY + threadIdx.x / kTileX);
  if (x >= w || y >= h) return;
  const size_t i = (size_t)y * w + x;
  const float c[3] = {rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]};
  const float e[3] = {se[3 * i], se[3 * i + 1], se[3 * i + 2]};
  const float a[3] = {albedo[3 * i], albedo[3 * i + 1], albedo[3 * i + 2]};
  const float n[3] = {normal[3 * i], normal[3 * i + 1], normal[3 * i + 2]};
  const Pixel r = accumulate_pixel(c, e, a, n, depth[i], x, y, w, h, K, prev);
  o0[i] = f4{n[0], n[1], n[2], r.n};
  o1[i] = f4{r.X[0], r.X[1], r.X[2], r.v[0]};
  o2[i] = f4{r.c[0], r.c[1], r.c[2], r.v[1]};
  ov2[i] = r.v[2];
  for (int k = 0; k < 3; ++k) {
    rgb_out[3 * i + k] = r.rgb_out[k];
    se_out[3 * i + k] = r.se_out[k];
  }
  if (n_out) n_out[i] = r.n;
  if (hist)
    for (int k = 0; k < 3; ++k) hist[3 * i + k] = r.hist[k];
}

spt_status bad(const char* who, const char* msg) {
  return fail(SPT_ERR_INVALID_ARG, std::string(who) + ": " + msg);
}

// What both accumulate calls ask of their arguments, in order. ins: the input planes the caller gave
// (none on the film path, whose inputs are the accumulator's own planes).
spt_status check_call(const spt_temporal* tp, const char* who, const spt_camera* cam,
                      const spt_temporal_params* params, PlaneList outs, PlaneList ins, CamConsts* cur) {
  if (!tp) return fail(SPT_ERR_INVALID_ARG, "null accumulator");
  if (!cam) return bad(who, "null camera");
  if (const char* e = params_error(params)) return bad(who, e);
  if (!outs.begin()[0] || !outs.begin()[1]) return bad(who, "null output plane");
  if (const char* e = inputs_error(outs, ins)) return bad(who, e);
  if (outputs_error(outs)) return bad(who, "two output planes are one plane");
  if (!camera_consts(cam, tp->width, tp->height, cur)) return bad(who, "the camera is singular or not finite");
  return SPT_OK;
}

// Enqueue one frame of validated arguments and, once it is queued, make it the history.
spt_status run(spt_temporal* tp, const float* rgb, const float* se, const float* albedo, const float* normal,
               const float* depth, const spt_camera* cam, const CamConsts& cur, const spt_temporal_params* params,
               float* rgb_out, float* se_out, float* n_out, float* hist, hipStream_t stream) {
  SPT_HIP(hipSetDevice(tp->device));
  const bool has = tp->frames > 0;
  const Consts K = make_consts(cur, has ? &tp->cam_consts : nullptr, has && same_camera(cam, &tp->cam), params);
  const Packed& in = tp->st[tp->cur];
  const Packed& out = tp->st[tp->cur ^ 1];
  hipLaunchKernelGGL(temporal_accumulate_kernel, dim3((unsigned)tiles_of(tp->width, tp->height)), dim3(kBlock), 0,
                     stream, rgb, se, albedo, normal, depth, tp->width, tp->height, K,
                     DevPrev{in.p0, in.p1, in.p2, in.v2}, out.p0, out.p1, out.p2, out.v2, rgb_out, se_out, n_out,
                     hist);
  SPT_HIP(hipGetLastError());
  tp->cur ^= 1;
  tp->frames += 1;
  tp->cam = *cam;
  tp->cam_consts = cur;
  return SPT_OK;
}

}  // namespace

extern "C" spt_status spt_temporal_create(int32_t device, int32_t width, int32_t height, spt_temporal** out) {
  if (!out) return fail(SPT_ERR_INVALID_ARG, "null argument");
  if (const char* e = size_error(width, height)) return bad("temporal", e);
  if (tiles_of(width, height) > kMaxTiles)
    return bad("temporal", "the image is too narrow or too flat for one launch (spt.h)");
  SPT_TRY(spt::open_device(device));
  spt_temporal* tp = new spt_temporal();
  tp->device = device;
  tp->width = width;
  tp->height = height;
  tp->npix = (size_t)width * (size_t)height;
  // two copies of 3 words and a float, 13 floats of film planes, float planes padded to 16 bytes
  const size_t n = tp->npix, n4 = (n + 3) & ~(size_t)3;
  const size_t bytes = 2 * (3 * n * sizeof(f4) + n4 * sizeof(float)) + 13 * n4 * sizeof(float);
  void* b = nullptr;
  const hipError_t e = hipMalloc(&b, bytes);
  if (e != hipSuccess) {
    delete tp;
    return fail(SPT_ERR_OOM, std::string("temporal alloc: ") + hipGetErrorString(e));
  }
  tp->base = b;
  char* p = (char*)b;
  const auto take = [&p](size_t size) {
    char* r = p;
    p += size;
    return r;
  };
  for (Packed& s : tp->st) {
    s.p0 = (f4*)take(n * sizeof(f4));
    s.p1 = (f4*)take(n * sizeof(f4));
    s.p2 = (f4*)take(n * sizeof(f4));
  }
  for (Packed& s : tp->st) s.v2 = (float*)take(n4 * sizeof(float));
  tp->rgb = (float*)take(3 * n4 * sizeof(float));
  tp->se = (float*)take(3 * n4 * sizeof(float));
  tp->albedo = (float*)take(3 * n4 * sizeof(float));
  tp->normal = (float*)take(3 * n4 * sizeof(float));
  tp->depth = (float*)take(n4 * sizeof(float));
  *out = tp;
  return SPT_OK;
}

extern "C" spt_status spt_temporal_destroy(spt_temporal* tp) {
  if (!tp) return SPT_OK;
  if (tp->base) {
    (void)hipSetDevice(tp->device);
    (void)hipFree(tp->base);
  }
  delete tp;
  return SPT_OK;
}

extern "C" spt_status spt_temporal_reset(spt_temporal* tp) {
  if (!tp) return fail(SPT_ERR_INVALID_ARG, "null accumulator");
  tp->frames = 0;
  return SPT_OK;
}

extern "C" spt_status spt_temporal_info_get(const spt_temporal* tp, spt_temporal_info* out) {
  if (!tp || !out) return fail(SPT_ERR_INVALID_ARG, "null argument");
  out->frames = tp->frames;
  out->width = tp->width;
  out->height = tp->height;
  out->has_history = tp->frames > 0 ? 1 : 0;
  out->reserved = 0;
  return SPT_OK;
}

extern "C" spt_status spt_temporal_accumulate_async(spt_temporal* tp, const float* rgb_dev, const float* se_dev,
                                                    const float* albedo_dev, const float* normal_dev,
                                                    const float* depth_dev, const spt_camera* cam,
                                                    const spt_temporal_params* params, float* rgb_out_dev,
                                                    float* se_out_dev, float* n_out_dev, float* hist_dev,
                                                    void* stream) {
  CamConsts cur;
  SPT_TRY(check_call(tp, "temporal_accumulate", cam, params, {rgb_out_dev, se_out_dev, n_out_dev, hist_dev},
                     {rgb_dev, se_dev, albedo_dev, normal_dev, depth_dev}, &cur));
  return run(tp, rgb_dev, se_dev, albedo_dev, normal_dev, depth_dev, cam, cur, params, rgb_out_dev, se_out_dev,
             n_out_dev, hist_dev, (hipStream_t)stream);
}

extern "C" spt_status spt_film_temporal_accumulate(const spt_film* film, const spt_guide* guide, spt_temporal* tp,
                                                   const spt_camera* cam, const spt_temporal_params* params,
                                                   float* rgb_out_dev, float* se_out_dev, float* n_out_dev,
                                                   float* hist_dev, float* albedo_out_dev, float* normal_out_dev,
                                                   float* depth_out_dev, void* stream) {
  const char* who = "film_temporal_accumulate";
  if (!film || !guide) return bad(who, "null film or guide");
  CamConsts cur;
  SPT_TRY(check_call(tp, who, cam, params,
                     {rgb_out_dev, se_out_dev, n_out_dev, hist_dev, albedo_out_dev, normal_out_dev, depth_out_dev}, {},
                     &cur));
  if (!film->batch) return bad(who, "not a noise film");
  if (film->batches_done < 2) return bad(who, "the error needs at least two batches");
  if (guide->samples_done == 0) return bad(who, "the guide holds no sample");
  if (guide->flags & SPT_GUIDE_THROUGH_SPECULAR)
    return bad(who, "a chain guide's depth is an optical length, not a position");
  if (film->shard_count > 1) return bad(who, "a shard's rows are not image neighbours");
  if (film->width != tp->width || film->rows != tp->height || !spt::shape_equal(*film, *guide))
    return bad(who, "the film's or the guide's size differs from the accumulator's");
  if (film->device != tp->device) return bad(who, "the film and the accumulator are on different devices");
  float* al = albedo_out_dev ? albedo_out_dev : tp->albedo;
  float* no = normal_out_dev ? normal_out_dev : tp->normal;
  float* de = depth_out_dev ? depth_out_dev : tp->depth;
  SPT_TRY(spt_film_resolve(film, tp->rgb, stream));
  SPT_TRY(spt_film_noise_map(film, tp->se, stream));
  SPT_TRY(spt_guide_resolve(guide, al, no, de, nullptr, stream));
  return run(tp, tp->rgb, tp->se, al, no, de, cam, cur, params, rgb_out_dev, se_out_dev, n_out_dev, hist_dev,
             (hipStream_t)stream);
}

extern "C" spt_status spt_temporal_state_download(spt_temporal* tp, const spt_temporal_state* out,
                                                  spt_camera* cam_out, void* stream) {
  if (!tp || !out) return fail(SPT_ERR_INVALID_ARG, "null argument");
  if (!out->c || !out->v || !out->n || !out->X || !out->N) return bad("temporal_state_download", "null plane");
  if (tp->frames == 0) return bad("temporal_state_download", "no history (no frame since the last reset)");
  const size_t n = tp->npix;
  std::vector<f4> w0(n), w1(n), w2(n);
  const Packed& s = tp->st[tp->cur];
  SPT_TRY(spt::copy_and_wait(tp->device, w0.data(), s.p0, n * sizeof(f4), hipMemcpyDeviceToHost, stream));
  SPT_TRY(spt::copy_and_wait(tp->device, w1.data(), s.p1, n * sizeof(f4), hipMemcpyDeviceToHost, stream));
  SPT_TRY(spt::copy_and_wait(tp->device, w2.data(), s.p2, n * sizeof(f4), hipMemcpyDeviceToHost, stream));
  std::vector<float> v2(n);
  SPT_TRY(spt::copy_and_wait(tp->device, v2.data(), s.v2, n * sizeof(float), hipMemcpyDeviceToHost, stream));
  for (size_t i = 0; i < n; ++i) {
    out->N[3 * i] = w0[i].x;
    out->N[3 * i + 1] = w0[i].y;
    out->N[3 * i + 2] = w0[i].z;
    out->n[i] = w0[i].w;
    out->X[3 * i] = w1[i].x;
    out->X[3 * i + 1] = w1[i].y;
    out->X[3 * i + 2] = w1[i].z;
    out->c[3 * i] = w2[i].x;
    out->c[3 * i + 1] = w2[i].y;
    out->c[3 * i + 2] = w2[i].z;
    out->v[3 * i] = w1[i].w;
    out->v[3 * i + 1] = w2[i].w;
    out->v[3 * i + 2] = v2[i];
  }
  if (cam_out) *cam_out = tp->cam;
  return SPT_OK;
}

/*
 * spt.h — C ABI of the MI355X-native smallpt sampling loop (small-pathtracer_amd).
 *
 * Drop-in boundary for the reference's per-pixel sampling loop
 *   /root/reference/src/smallpt.cpp:528-542  (main: row/col/sample loops, r += radiance()/spp, c[i] = clamp(r))
 * whose per-sample kernel is radiance() at :419-496 (live path tracer :444-480).
 * The reference has no plugin/operator/FFI API; its de-facto inputs are globals and locals:
 *   scene  Hitable *rect[NUMBER_OBJ]         :287-311   -> spt_prim[] (tagged flat records)
 *   camera Camera cam(LOOKFROM, ...)         :262-279, :521 -> spt_camera
 *   w, h, samps                              :507-508   -> spt_params.width/height/spp
 *   srand(time) / Xi={0,0,y^3}               :503, :530 -> spt_params.seed (counter-based Philox stream)
 * and its output is Vec *c (w*h RGB, clamped to [0,1], row-major, y=0 = top row) :510, :538,
 * consumed by the PPM writer :548-551 -> rgb_out (float, same layout/clamping).
 *
 * Conventions: extern "C", plain pointers and sizes, no exceptions cross the ABI, every entry
 * point returns an spt_status. Buffers are caller-owned. One spt_context per HIP device; calls on
 * different contexts may run concurrently, calls on one context must be serialised by the caller.
 */
#ifndef SPT_H_
#define SPT_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPT_ABI_VERSION 6 /* 2: spt_stats gained shadow_traced, sphere_vertices, flop_executed;
                             3: shadow_proven; 4: spt_gather_plan, spt_deinterleave_source,
                             spt_gather_staging_floats, spt_shutdown; 5: SPT_FLAG_REFERENCE_LEAKS;
                             6: spt_kernel_count, spt_kernel_name, spt_select_kernel,
                             spt_context_kernel. Added since, with no change to an existing struct or
                             entry point (so the version stays): SPT_HAS_FILM, the spt_film_* calls;
                             SPT_HAS_FILM_NOISE, the spt_film_noise_* calls; SPT_HAS_FILM_ADAPTIVE,
                             the spt_film_adaptive_* calls; SPT_HAS_FILM_POOL, spt_film_noise_pool_map,
                             spt_film_adaptive_select_pooled and their *_host statements;
                             SPT_HAS_GUIDE, the spt_guide_* calls; SPT_HAS_DENOISE, the
                             spt_denoise_* and spt_denoiser_* calls and spt_film_denoise;
                             SPT_HAS_GUIDE_CHAIN, spt_guide_create_ex (spt_guide_info's last field,
                             always 0 until then, now reads the guide's flags); SPT_HAS_DENOISE_PAIR,
                             the spt_denoise_pair_* calls and spt_film_pair_denoise;
                             SPT_HAS_DENOISE_BANK, the spt_denoise_bank_* calls and
                             spt_film_pair_denoise_bank; SPT_HAS_GUIDE_LIGHT, the spt_light_guide_*
                             and spt_light_shade_* calls; SPT_HAS_TEMPORAL, the spt_temporal_* calls
                             and spt_film_temporal_accumulate */
#define SPT_HAS_FILM 1    /* progressive rendering: sample windows into a resumable integer film */
#define SPT_HAS_FILM_NOISE 1 /* the film's second moment: error map, RMSE estimate (below) */
#define SPT_HAS_FILM_ADAPTIVE 1 /* per-pixel batch counts, passes over the pixels still noisy (below) */
#define SPT_HAS_FILM_POOL 1 /* the error pooled over a pixel's neighbourhood: map and selection (below) */
#define SPT_HAS_GUIDE 1 /* guide planes: first-hit albedo, normal, depth and coverage (below) */
#define SPT_HAS_GUIDE_CHAIN 1 /* guides that follow the specular chain: spt_guide_create_ex (below) */
#define SPT_GUIDE_THROUGH_SPECULAR 1u /* spt_guide_create_ex flag: records of the first DIFF surface */
#define SPT_GUIDE_MAX_CHAIN 8 /* segments of a chain at most, the camera ray included */
#define SPT_HAS_GUIDE_LIGHT 1 /* light guides: per-pixel light visibility and direct irradiance (below) */
#define SPT_HAS_DENOISE 1 /* the edge-stopping a-trous filter over a film and its guides (below) */
#define SPT_HAS_DENOISE_PAIR 1 /* two independent halves, cross-weighted, and a measured error (below) */
#define SPT_HAS_DENOISE_BANK 1 /* a few pair filters, the one of least cross-validated error per pixel (below) */
#define SPT_HAS_TEMPORAL 1 /* temporal accumulation: the last frame reprojected through the guides (below) */

typedef enum spt_status {
  SPT_OK = 0,
  SPT_ERR_INVALID_ARG = 1, /* bad sizes, null pointers, unsupported scene/params */
  SPT_ERR_HIP = 2,         /* a HIP runtime call failed (spt_last_error() has the text) */
  SPT_ERR_NO_DEVICE = 3,   /* no usable gfx950 device */
  SPT_ERR_OOM = 4,         /* device allocation failed */
  SPT_ERR_UNSUPPORTED = 5, /* reserved: feature not implemented (not returned today) */
  SPT_ERR_RCCL = 6         /* an RCCL call of the multi-GPU gather failed (spt_last_error()) */
} spt_status;

/* Primitive kinds: the reference's Hitable subclasses (:92-254). */
typedef enum spt_kind {
  SPT_RECT_XY = 0, /* Rectangle_xy(x1,x2,y1,y2,z, e,c,refl)  :137-178, plane z=k  */
  SPT_RECT_XZ = 1, /* Rectangle_xz(x1,x2,z1,z2,y, e,c,refl)  :92-135,  plane y=k  */
  SPT_RECT_YZ = 2, /* Rectangle_yz(y1,y2,z1,z2,x, e,c,refl)  :180-221, plane x=k  */
  SPT_SPHERE = 3   /* Sphere(rad, p, e, c, refl)             :223-254             */
} spt_kind;

/* Refl_t :72-74. Only DIFF is live in the reference (:457); SPEC/REFR are commented out (:481-495). */
typedef enum spt_refl { SPT_DIFF = 0, SPT_SPEC = 1, SPT_REFR = 2 } spt_refl;

/* One scene primitive. geom[] holds the constructor arguments in the reference's order:
 *   RECT_XY: {x1, x2, y1, y2, z}   RECT_XZ: {x1, x2, z1, z2, y}   RECT_YZ: {y1, y2, z1, z2, x}
 *   SPHERE : {rad, px, py, pz, 0}
 * e = emission, c = colour (Vec e, c in the reference). Doubles mirror the reference constructors;
 * the device path rounds them to fp32 once per render. */
typedef struct spt_prim {
  int32_t kind;  /* spt_kind */
  int32_t refl;  /* spt_refl */
  double geom[5];
  double e[3];
  double c[3];
} spt_prim;

/* Camera :256-285 — the four vectors its constructor computes (:267-274). Build with
 * spt_camera_init() for the reference's constructor semantics (float vfov/aspect, tanf). */
typedef struct spt_camera {
  double origin[3];
  double lower_left_corner[3];
  double horizontal[3];
  double vertical[3];
} spt_camera;

/* Light-sample arithmetic of light_sampling() :363-369:  x = 32 + rand()*36/double(RAND_MAX).
 * With glibc (RAND_MAX = 2^31-1) rand()*36 overflows int32 and wraps, so the reference as built
 * on Linux samples x in [31,33], z in [62,64] (measured). GLIBC_WRAP reproduces that arithmetic
 * on a 31-bit draw; UNIFORM is the intended [x0, x0+dx] x [z0, z0+dz] (MinGW RAND_MAX=32767). */
typedef enum spt_light_mode { SPT_LIGHT_GLIBC_WRAP = 0, SPT_LIGHT_UNIFORM = 1 } spt_light_mode;

typedef struct spt_params {
  int32_t width, height, spp; /* :507-508 */
  uint32_t seed;              /* Philox4x32-7 counter word 3 (the key is the fixed SPT_PHILOX_KEY) */
  float nee_prob;             /* Q of :464 (`q < Q`): 1 = HEAD explicit light sampling, 0 = cosine only */
  int32_t rr_depth;           /* Russian roulette starts when ++depth > rr_depth  (:448, HEAD = 5) */
  int32_t max_depth;          /* 0 = unbounded (reference); >0 = path ends at this vertex depth */
  int32_t light_id;           /* primitive index treated as "the light" by NEE (:467, HEAD = 6) */
  float light_x0, light_dx;   /* light sample rect x0 + [0,dx] (:365)   HEAD 32, 36 */
  float light_z0, light_dz;   /* light sample rect z0 + [0,dz] (:366)   HEAD 63, 36 */
  float light_y;              /* sample plane y (:367)                  HEAD 81.6   */
  float light_area;           /* PDF area constant (:471)               HEAD 1296   */
  int32_t light_mode;         /* spt_light_mode */
  /* Row sharding (multi-GPU): tiles of tile_rows image rows, tile t rendered by shard t % shard_count.
   * The output of a shard holds only its rows, compacted in increasing row order (spt_shard_rows). */
  int32_t tile_rows;          /* 0 -> 8 */
  int32_t shard_index, shard_count;
  int32_t chunk;              /* samples per work unit (0 = auto). Never changes results. */
  int32_t device;             /* HIP device ordinal for spt_render() */
  uint32_t flags;             /* SPT_FLAG_* below; other bits must be 0 */
} spt_params;

/* random_scattering() draws from the reference's commented-out UNIFORM hemisphere code (:351-360:
 * dir = u cos(r1) sqrt(r2(2-r2)) + v sin(r1) sqrt(r2(2-r2)) + w (1-r2)) instead of the live
 * cosine-weighted code (:340-347); the estimator weight stays 1, as in the reference. */
#define SPT_FLAG_UNIFORM_SCATTER 1u
/* Leaked paths (a path ray that misses every primitive, :371-377) go on from the miss vertex --
 * the origin, with prim 0's material -- exactly as the reference's do. Without this flag the
 * contract's leak-end rule applies wherever the host can prove it (contract v6: the
 * scene has a closed room, the origin lies outside it, prim 0 does not emit and every emitter lies
 * inside): such a path ends at its first miss, which skips the reference's post-leak vertices (~4 %
 * of them in the HEAD scene) and changes the image's mean by ~8 ppm. */
#define SPT_FLAG_REFERENCE_LEAKS 4u
/* Kernel specialisation cap, flags bits 8-9 (A/B comparisons and tests; never changes a result:
 * every kernel computes the same contract bit for bit). AUTO (0) runs the most specialised kernel
 * the host can prove applicable to the scene and params; the others stop at that level. */
#define SPT_FLAG_KERNEL_LEVEL_MASK 0x300u
#define SPT_FLAG_KERNEL_LEVEL(l) (((uint32_t)(l) & 3u) << 8)
enum { SPT_KERNEL_LEVEL_AUTO = 0, SPT_KERNEL_LEVEL_GENERIC = 1, SPT_KERNEL_LEVEL_CORNELL = 2,
       SPT_KERNEL_LEVEL_CONST = 3 };

/* The counter RNG: Philox4x32 with SPT_PHILOX_ROUNDS rounds (7: the Random123 paper's smallest
 * Crush-resistant count for Philox4x32; its library default is 10), a fixed key (so the key
 * schedule is compile-time) and the counter ctr = (pixel = y*w + x, sample, vertex | stream << 31,
 * seed). */
#define SPT_PHILOX_ROUNDS 7
#define SPT_PHILOX_KEY0 0x53505430u /* "SPT0" */
#define SPT_PHILOX_KEY1 0x53505431u /* "SPT1" */

/* Per-render path statistics (counted in-kernel, summed once per wave). */
typedef struct spt_stats {
  uint64_t samples;        /* pixel-samples finished = camera rays */
  uint64_t path_rays;      /* rays traced through the scene for path vertices (incl. camera rays) */
  uint64_t shadow_rays;    /* NEE shadow rays of the reference: one per NEE event (:466). The kernel
                              traces only `shadow_traced` of them (below); the others cannot reach
                              the light and are rejected exactly by the light's own test */
  uint64_t vertices;       /* path vertices shaded (incl. terminal ones) */
  uint64_t nee_events;     /* NEE light samples taken (:465) */
  uint64_t nee_light_hits; /* ... whose shadow ray hit light_id (:470-472) */
  uint64_t cosine_samples; /* cosine-weighted scatter directions drawn (:337-347) */
  uint64_t misses;         /* path rays that hit nothing (reference: x = origin, id = 0, :373-374) */
  uint64_t shadow_traced;  /* NEE shadow rays that pass the light pre-test: the kernel resolves each
                              of them as the nearest-hit test of :466-467 -- by tracing it, or ... */
  uint64_t sphere_vertices;/* vertices on a sphere (Sphere::normal :246-253) */
  uint64_t shadow_proven;  /* ... of shadow_traced, those the HEAD NEE kernel proved to reach the
                              light without a trace (exact: the trace's result is implied by the
                              geometry; 0 in the other kernels) */
  double flop;             /* algorithmic FLOPs of the reference's work (model in spt_flops.h): every
                              shadow ray of :466 charged as a full scene test */
  double flop_executed;    /* the same model with only the traced shadow rays charged
                              (shadow_traced - shadow_proven) */
  double kernel_ms;        /* device time of the render kernel (HIP events) */
} spt_stats;

/* ---- host helpers mirroring the reference's host-side API ---- */
spt_status spt_default_params(spt_params* p); /* HEAD: w=h=512, spp=16, Q=1, rr 5, light 6, ... */
spt_status spt_camera_init(spt_camera* cam, const double lookfrom[3], const double lookat[3],
                           const double vup[3], float vfov_deg, float aspect); /* :262-275 */
/* rect[] :287-311 (17 primitives). *n_out = 17; fails if cap < 17. */
spt_status spt_scene_cornell(spt_prim* out, int32_t cap, int32_t* n_out);
/* The build-defined 32-sphere scene of config 5: room rects 0-6 of :288-294 + 32 DIFF spheres. */
spt_status spt_scene_spheres32(spt_prim* out, int32_t cap, int32_t* n_out);
/* The room and light of :288-294 plus smallpt's mirror (SPEC) and glass (REFR) balls at the places
 * of the spheres commented out at :296-297; shading = the commented-out code :481-495. 9 prims. */
spt_status spt_scene_cornell_specular(spt_prim* out, int32_t cap, int32_t* n_out);
/* The classic smallpt sphere box of the reference's older revision (the constants mined from the
 * shipped src/a.exe; its renders are the repository's image*.ppm): walls are
 * spheres of radius 1e5 (left x = 1e5+1 green, right x = -1e5+99 red, back, front (black), floor,
 * ceiling y = -1e5+81.6), two matte white (DIFF, .999) balls of radius 16.5 at (27,16.5,47) /
 * (73,16.5,78), and the light, a sphere of radius 600 at (50, 681.33, 81.6) with emission 12
 * (prim 8). 9 prims. Spheres of radius >= SPT_WIDE_SPHERE_RADIUS are intersected in fp64: an fp32
 * quadratic cannot hold a 1e5 wall to the scene's scale, and for the radius-600 light, whose cap
 * dips only 0.27 below the ceiling, r^2 - |q|^2 has an fp32 rounding step of ~0.03 (measured:
 * concentric rings and a washed-out ceiling around the cap). NEE (nee_prob > 0) samples the light
 * RECTANGLE of spt_params, which this scene does not have: render it with nee_prob = 0. */
spt_status spt_scene_smallpt_classic(spt_prim* out, int32_t cap, int32_t* n_out);
/* The same box with smallpt's original materials: the left ball a mirror (SPEC), the right one
 * glass (REFR; shading = the commented-out code :481-495). 9 prims. */
spt_status spt_scene_smallpt_mirror_glass(spt_prim* out, int32_t cap, int32_t* n_out);
#define SPT_WIDE_SPHERE_RADIUS 100.0 /* larger than the scenes' rooms (~100 units across) */
/* Rows rendered by this shard (params tile_rows/shard_index/shard_count), ascending. Returns count. */
int32_t spt_shard_rows(const spt_params* p, int32_t* rows_out, int32_t cap);

/* ---- rendering ---- */
/* One-shot drop-in for :528-542. rgb_out: caller-owned HOST buffer of shard_rows*w*3 floats
 * (linear, clamped to [0,1] per channel after the spp average, :538). stats may be NULL.
 * The library keeps one render context and device output buffer per device (params.device) between
 * calls, so repeated calls pay no context creation, allocation or cold launch; calls on one device
 * are serialised, calls on different devices may run concurrently. Thread-safe. */
spt_status spt_render(const spt_prim* prims, int32_t n_prims, const spt_camera* cam,
                      const spt_params* p, float* rgb_out, spt_stats* stats);
/* Releases spt_render's cached per-device contexts and buffers (the next spt_render re-creates
 * them). Call before unloading the library if its device memory must be returned earlier than
 * process exit. */
spt_status spt_shutdown(void);

typedef struct spt_context spt_context;
spt_status spt_context_create(int32_t device, spt_context** out);
spt_status spt_context_destroy(spt_context* ctx);
/* Enqueue a render on `stream` (a hipStream_t, NULL = default stream). rgb_dev: DEVICE buffer of
 * shard_rows*w*3 floats. No allocation once the context is large enough (spt_context_reserve) and
 * no host synchronisation, except that a second call before spt_context_stats() first waits for
 * the previous call's scene upload (the pinned staging buffers are reused). prims, cam and p are
 * consumed before the call returns: the caller may change or free them at once. A context's frames
 * share its device buffers, so its calls must be serialised by the caller and enqueued on one stream
 * (or ordered by the caller, e.g. by an event recorded after one call that the next call's stream
 * waits for); frames of different contexts need no ordering. */
spt_status spt_context_reserve(spt_context* ctx, int32_t n_prims, const spt_params* p);
spt_status spt_render_async(spt_context* ctx, const spt_prim* prims, int32_t n_prims,
                            const spt_camera* cam, const spt_params* p, float* rgb_dev,
                            void* stream);
/* Synchronises the context's last render and returns its stats (SPT_ERR_INVALID_ARG before the
 * context's first render).
 * A render that hit the kernel's runaway-iteration guard returns SPT_ERR_HIP here and leaves its
 * rgb_dev all NaN (never a partial image). */
spt_status spt_context_stats(spt_context* ctx, spt_stats* out);

/* ---- which kernel runs ----
 * A render launches one of spt_kernel_count() variants of the render kernel, all of which compute
 * the same contract bit for bit; the host picks the most specialised one it can prove applicable
 * to the scene, the camera and the params (capped by SPT_FLAG_KERNEL_LEVEL). These calls make that
 * choice observable; none of them changes a render. */
int32_t spt_kernel_count(void);
/* "generic", "cornell", "const", "const_nee", ..., "uplight_cos_cam"; NULL for an id out of range. */
const char* spt_kernel_name(int32_t id);
typedef struct spt_kernel_choice {
  int32_t kernel;        /* variant id in [0, spt_kernel_count()) */
  int32_t leak_end;      /* 1 = leaked paths end at their first miss (contract v6's leak-end rule),
                            0 = they go on as the reference's (SPT_FLAG_REFERENCE_LEAKS, or a scene
                            the rule cannot be proven for) */
  int32_t early_resolve; /* 1 = the variant resolves some NEE shadow rays without a trace
                            (spt_stats.shadow_proven): the literal HEAD NEE kernels always, the sphere
                            NEE kernels when the scene allows a threshold, the kernels with uploaded
                            boxes when the room, the light and the boxes are within their clauses'
                            margins; 0 = every shadow ray is traced */
} spt_kernel_choice;
/* The variant spt_render / spt_render_async would launch for these arguments. A pure host function:
 * no device, no context; the same argument validation as a render. */
spt_status spt_select_kernel(const spt_prim* prims, int32_t n_prims, const spt_camera* cam,
                             const spt_params* p, spt_kernel_choice* out);
/* Name of the variant of the context's last launch; NULL before any launch and after a render of a
 * shard without rows. ctx == NULL: the calling thread's last spt_render() (which owns its context). */
const char* spt_context_kernel(spt_context* ctx);

/* ---- progressive rendering: sample windows and the resumable integer film (SPT_HAS_FILM) ----
 * A render draws the sample indices [0, spp) of every pixel, converts each sample to 1.31 fixed point
 * with the one scale 2^31 / spp and sums in uint64. A film keeps those sums on the device between
 * launches: uint64[rows * w][3] in image pixel order (rows = the shard's compact rows, the row layout
 * of rgb_dev). A pass renders the window [sample_base, sample_base + sample_count) of the SAME
 * spp-sample image (the counter RNG is keyed by the absolute sample index, the scale stays
 * 2^31 / spp) and adds it. Once every index of [0, spp) has been added exactly once, the film's sums
 * are the one-shot render's, and its resolved image equals spt_render's bit for bit -- whatever the
 * split, the order of the windows, the contexts, processes or GPUs that rendered them.
 * Keeping the windows disjoint is the caller's duty: a film only counts samples (samples_done), it
 * does not record which indices it holds, so that films filled elsewhere can be merged. Calls on one
 * film must be serialised by the caller and enqueued on one stream (or ordered by the caller). */
typedef struct spt_film spt_film;
typedef struct spt_film_info {
  int32_t width, rows, spp_total; /* rows = the shard's row count (the image's height unsharded) */
  int64_t samples_done;           /* samples per pixel added so far, 0 .. spp_total */
} spt_film_info;
/* A zeroed film on `device` for renders with p's width, height, spp (= spp_total) and shard fields. */
spt_status spt_film_create(int32_t device, const spt_params* p, spt_film** out);
spt_status spt_film_destroy(spt_film* film);
spt_status spt_film_info_get(const spt_film* film, spt_film_info* out);
spt_status spt_film_clear(spt_film* film, void* stream); /* sums and samples_done back to 0 */
/* Enqueue the render of the window on `stream` and its add into the film. p's width, height, spp
 * and shard fields must equal the film's, the window must lie in [0, spp) with sample_count >= 1, and
 * samples_done + sample_count must not exceed spp: SPT_ERR_INVALID_ARG otherwise, and a rejected call
 * queues nothing and leaves the film untouched. rgb_dev_or_null: if given (DEVICE, rows*w*3 floats),
 * the same pass also writes the film resolved after the add (what spt_film_resolve would give).
 * ctx and film must be on one device. spt_context_stats(ctx) afterwards reports this pass alone
 * (samples = pixels * sample_count; the integer fields of the passes sum to the one-shot's). A pass
 * that hit the runaway-iteration guard adds nothing: the film's sums are unchanged, a given rgb_dev is
 * all NaN, and spt_context_stats returns SPT_ERR_HIP and takes the pass out of samples_done. A shard
 * without rows renders nothing (its film has no sums) and only counts the samples. */
spt_status spt_film_render_async(spt_context* ctx, spt_film* film, const spt_prim* prims,
                                 int32_t n_prims, const spt_camera* cam, const spt_params* p,
                                 int32_t sample_base, int32_t sample_count, float* rgb_dev_or_null,
                                 void* stream);
/* Film -> float image (DEVICE, rows*w*3). A full film (samples_done == spp_total):
 * min((float)sum * 2^-31, 1), the one-shot render's image. A partial one (a preview):
 * min(((float)sum * 2^-31) * r, 1) with r = (float)((double)spp_total / samples_done), two separate
 * multiplies. samples_done == 0: zeros. */
spt_status spt_film_resolve(const spt_film* film, float* rgb_dev, void* stream);
/* dst += src, dst.samples_done += src.samples_done: films of equal width, rows and spp_total on one
 * device (a film from another process or GPU arrives through spt_film_upload). Rejected, with
 * dst untouched, when they differ or the sum of their samples_done exceeds spp_total. */
spt_status spt_film_merge(spt_film* dst, const spt_film* src, void* stream);
/* The sums to and from HOST memory (rows*w*3 uint64, pixel order): a checkpoint. Both wait for their
 * copy on `stream`, so the host buffer is complete (download) or free again (upload) on return. */
spt_status spt_film_download(const spt_film* film, uint64_t* host_sums, void* stream);
spt_status spt_film_upload(spt_film* film, const uint64_t* host_sums, int64_t samples_done,
                           void* stream);
/* The resolve as a pure host function (no device): the CPU statement of spt_film_resolve, for
 * checkpoints and tests. Uses info's width, rows, spp_total and samples_done. */
spt_status spt_film_resolve_host(const uint64_t* sums, const spt_film_info* info, float* rgb_out);

/* ---- the noise-aware film: batch moments, error map, RMSE estimate (SPT_HAS_FILM_NOISE) ----
 * A noise film takes its samples in B = spp_total / batch passes of exactly `batch` samples each.
 * Beside the sums S it keeps the moment plane M2: uint64[rows * w * 3][2], element e the 128-bit
 * integer (lo, hi) = the sum over the passes of P^2, P = the pass's 1.31 window sum of that pixel and
 * channel (what the pass adds to S). Exact integers: P <= batch * 2^31, so B * M2 <= spp^2 * 2^62
 * < 2^128; like the sums, M2 does not depend on the order of the passes, the contexts or the GPUs.
 * From the two the standard error of every resolved value follows (the passes are independent
 * estimates of the same pixel: the counter RNG is keyed by the absolute sample index):
 *   D  = B * M2 - S^2                (128-bit, >= 0 by Cauchy-Schwarz), d = (double)hi * 2^64 + (double)lo
 *   se = (float)(sqrt(d) * k),       k = spp_total / (batch * 2^31 * B * sqrt(B - 1)) in double
 *   se = 0 where the channel's resolved value (spt_film_resolve's rule) is the clamp 1.0f
 * with B = batches_done >= 2; se estimates the standard error of the resolved (preview or full) value.
 * The clamp rule makes the figures those of the clamped image, the project's metric: an edge pixel
 * of the light has a large unclamped error and a clamped error of 0. */
typedef struct spt_film_noise_info {
  int32_t enabled, batch; /* enabled = 0: a plain film (batch and batches_done 0) */
  int64_t batches_done;
} spt_film_noise_info;
typedef struct spt_noise_summary {
  double rmse[3];       /* per channel: sqrt(mean over ALL pixels of d * k^2), clamped channels 0 */
  double rmse_all;      /* the same over the three channels together */
  float se_max;         /* the largest se of the map */
  uint64_t clamped;     /* channels whose resolved value is the clamp (se = 0 by rule) */
  int64_t batches_done; /* B */
} spt_noise_summary;
/* Allocates and zeroes M2. Only on an empty film (samples_done == 0), with batch >= 1,
 * spp_total % batch == 0 and spp_total / batch >= 2: SPT_ERR_INVALID_ARG otherwise, film untouched.
 * From then on spt_film_render_async accepts only windows with sample_count == batch and
 * sample_base % batch == 0 (rejected otherwise: nothing queued, film untouched); the accumulate pass
 * also does M2 += P^2. A pass that hit the runaway guard adds nothing to M2 either and its batch is
 * taken back with its samples. spt_film_clear also zeroes M2 and the batch count. spt_film_merge
 * wants both films plain (as above) or both noise films of equal batch (dst.M2 += src.M2 with carry,
 * the batch counts add); a mixed pair or unequal batches are rejected with dst untouched.
 * spt_film_upload on a noise film requires samples_done % batch == 0. */
spt_status spt_film_noise_enable(spt_film* film, int32_t batch);
spt_status spt_film_noise_info_get(const spt_film* film, spt_film_noise_info* out);
/* M2 to and from HOST memory (rows*w*3 pairs (lo, hi) of uint64, pixel order); both wait for their
 * copy. upload: 0 <= batches_done <= spp_total / batch. Keeping spt_film_upload's samples_done and
 * this batches_done consistent (samples_done == batches_done * batch) is the caller's duty, as
 * keeping windows disjoint is. Rejected on a plain film. */
spt_status spt_film_noise_download(const spt_film* film, uint64_t* host_m2, void* stream);
spt_status spt_film_noise_upload(spt_film* film, const uint64_t* host_m2, int64_t batches_done,
                                 void* stream);
/* The error map: se of every value of the film, rows*w*3 floats (DEVICE), enqueued on `stream`.
 * Rejected on a plain film and while batches_done < 2. */
spt_status spt_film_noise_map(const spt_film* film, float* se_dev, void* stream);
/* The image figures. Waits on `stream`. A two-stage reduction in a fixed order (per-block partials,
 * then one block; no floating-point atomics): the same film gives the same bits every time. */
spt_status spt_film_noise_summary(spt_film* film, spt_noise_summary* out, void* stream);
/* Both as pure host functions (no device): sums and m2 as downloaded, info and noise from the
 * *_info_get calls (width, rows, spp_total, samples_done; batch, batches_done). */
spt_status spt_film_noise_map_host(const uint64_t* sums, const uint64_t* m2,
                                   const spt_film_info* info, const spt_film_noise_info* noise,
                                   float* se_out);
spt_status spt_film_noise_summary_host(const uint64_t* sums, const uint64_t* m2,
                                       const spt_film_info* info, const spt_film_noise_info* noise,
                                       spt_noise_summary* out);

/* ---- adaptive sampling: per-pixel batch counts and passes over a pixel list (SPT_HAS_FILM_ADAPTIVE) ----
 * An adaptive film is a noise film whose pixels may stop taking batches. It keeps one more plane,
 * cnt: uint32[rows * w], low 31 bits = the batches that pixel holds, bit 31 = retired. The film's
 * front is batches_done. A pixel is either active (cnt == front) or retired (bit 31 set, batches <=
 * front), and a retired pixel never returns; so pixel p always holds exactly the samples
 * [0, batches(p) * batch) of the spp_total-sample image, and its sums and moments are those of a
 * uniform noise film after batches(p) batches, bit for bit (samples are keyed by the global pixel
 * index and the absolute sample index and summed in integers, whichever launch rendered them).
 * Every per-pixel figure takes the pixel's own B = batches(p) through one table, computed once on the
 * host in double and read by the kernels and the host statements alike:
 *   r(B) = (float)((double)spp_total / (B * batch)), full iff B * batch == spp_total (the resolve)
 *   k(B) = spp_total / (batch * 2^31 * B * sqrt(B - 1)), k2(B) = k(B)^2 (the error; 0 for B < 2) */
typedef struct spt_film_adaptive_info {
  int32_t enabled, reserved;
  int64_t front;         /* batches_done */
  int64_t n_active;      /* pixels the next pass would render */
  int64_t samples_total; /* pixel-samples spent: the sum over the passes of n_active * batch */
} spt_film_adaptive_info;
/* Only on an empty noise film with spp_total / batch <= 4096: SPT_ERR_INVALID_ARG otherwise, film
 * untouched. Allocates and zeroes cnt, the list and the scan scratch, uploads the table. From then on
 * spt_film_render_async accepts only the next window (sample_base == front * batch, sample_count ==
 * batch) and renders the active pixels: while nothing has retired through the ordinary launch (a
 * noise film's pass, the counts implied), afterwards through a launch over the active list whose
 * accumulate scatters (virtual pixel v -> g = list[v]: S[g] += P, M2[g] += P^2, cnt[g] += 1). With
 * rgb_dev the adaptive resolve is enqueued behind the add. spt_context_stats then reports
 * samples = n_active * batch. Rejected, nothing queued, film untouched: an out-of-order window, and a
 * pass with no active pixel. A pass that hit the runaway guard adds nothing, increments no count and
 * spt_context_stats restores the front. spt_film_info_get reports samples_done = front * batch.
 * spt_film_resolve, spt_film_noise_map and spt_film_noise_summary use every pixel's own B (the summary
 * stays the mean over ALL pixels, batches_done = the front). spt_film_clear resets counts and list.
 * spt_film_merge with an adaptive film on either side is rejected with dst untouched; spt_film_upload
 * and spt_film_noise_upload keep their meaning (sums, moments) and spt_film_adaptive_upload sets the
 * front, so a checkpoint uploads all three with the counts last. */
spt_status spt_film_adaptive_enable(spt_film* film);
spt_status spt_film_adaptive_info_get(const spt_film* film, spt_film_adaptive_info* out);
/* Retire pixels; the rest is the next pass's list. Requires front >= 2. A pixel stays active iff it is
 * active, and keep is NULL or keep[p] != 0 (DEVICE, rows*w bytes), and se_threshold < 0 or some channel
 * has d * k2(B) > se_threshold^2 (d of the error map: 0 for a clamped channel; the square taken once on
 * the host in double; no square root, so host and device run the same IEEE operations). The pixels
 * that leave get bit 31. The new list is ascending, built by a deterministic compaction (per-block
 * counts from wave ballots, one scan, a scatter by lane rank: no atomic decides an order). Waits on
 * `stream` and returns the count. Rejected: a NaN threshold, a plain or non-adaptive film, front < 2. */
spt_status spt_film_adaptive_select(spt_film* film, double se_threshold, const uint8_t* keep_dev_or_null,
                                    int64_t* n_active, void* stream);
/* The counts plane to and from HOST memory (rows*w uint32); both wait for their copy. An upload
 * rebuilds the list and the front: the active pixels must share one count (the front; with none active
 * the front is the largest count) and no count may exceed spp_total / batch. */
spt_status spt_film_adaptive_download(const spt_film* film, uint32_t* host_counts, void* stream);
spt_status spt_film_adaptive_upload(spt_film* film, const uint32_t* host_counts, void* stream);
/* The per-pixel forms as pure host functions (no device): sums, m2 and counts as downloaded; info's
 * width, rows, spp_total; noise's batch (and batches_done = the front, which the summary reports). */
spt_status spt_film_adaptive_resolve_host(const uint64_t* sums, const uint32_t* counts,
                                          const spt_film_info* info, const spt_film_noise_info* noise,
                                          float* rgb_out);
spt_status spt_film_adaptive_noise_map_host(const uint64_t* sums, const uint64_t* m2,
                                            const uint32_t* counts, const spt_film_info* info,
                                            const spt_film_noise_info* noise, float* se_out);
spt_status spt_film_adaptive_noise_summary_host(const uint64_t* sums, const uint64_t* m2,
                                                const uint32_t* counts, const spt_film_info* info,
                                                const spt_film_noise_info* noise,
                                                spt_noise_summary* out);
/* spt_film_adaptive_select on the host: counts_out (rows*w) = the new plane, list_out (rows*w
 * capacity) = the new active list ascending, *n_active its length. keep: HOST bytes or NULL. */
spt_status spt_film_adaptive_select_host(const uint64_t* sums, const uint64_t* m2,
                                         const uint32_t* counts, const spt_film_info* info,
                                         const spt_film_noise_info* noise, double se_threshold,
                                         const uint8_t* keep_or_null, uint32_t* counts_out,
                                         uint32_t* list_out, int64_t* n_active);

/* ---- the pooled error: a pixel's neighbourhood decides, not its own estimate (SPT_HAS_FILM_POOL) ----
 * A pixel's own estimate after B batches has B - 1 degrees of freedom; a selection on it retires the
 * pixels whose estimate is low by luck. These calls pool the per-batch variance over a window of
 * (2 radius + 1)^2 pixels. For pixel q with B_q = cnt[q] & 0x7FFFFFFF (a uniform noise film:
 * batches_done) and channel c
 *   u(q,c) = (d(q,c) * k2(B_q)) * (double)B_q      d of the error map (0 for a clamped channel)
 * the estimated variance of a ONE-batch estimate in resolved units, comparable between pixels at
 * different counts. A pixel with B_q < 2 has u = 0 and is not counted (uploaded counts only).
 * The window of pixel (y, x): columns max(0, x - R) .. min(w - 1, x + R); rows y - R .. y + R clipped
 * to the film's rows and, with band_rows > 0, to the pixel's band [b, b + band_rows), b = y - y %
 * band_rows: no window crosses a row that is a multiple of band_rows. The device passes band_rows = 0
 * for an unsharded film and the effective tile_rows for a film with shard_count > 1 (a shard's compact
 * rows are image neighbours only inside one tile). The sums, in this order and no other (both sides
 * are built without contraction, so host and device run the same IEEE double operations):
 *   h(y,x,c) = 0.0 + u(y,x0,c) + ... + u(y,x1,c)    columns ascending
 *   g(y,x,c) = 0.0 + h(y0,x,c) + ... + h(y1,x,c)    rows ascending
 *   n(y,x)   = the window's pixels with B_q >= 2
 *   SPT_POOL_EXCLUDE_CENTER: g = g - u(y,x,c), one subtraction per channel, and n = n - 1 if B_p >= 2;
 *   the decision about a pixel then does not depend on that pixel's own samples.
 * The pooled error map: se_pool(p,c) = (float)sqrt(g / ((double)n * (double)B_p)), 0 where n == 0 or
 * B_p < 2. The pooled selection is spt_film_adaptive_select with one clause changed: an active pixel
 * stays iff keep allows it and (se_threshold < 0 or some channel has
 * g > (thr2 * (double)n) * (double)B_p), thr2 = se_threshold^2 once on the host: no division, no square
 * root. Where n == 0 the pixel's own rule (spt_film_adaptive_select's) decides. Every decision is taken
 * from the planes as they were before this selection marked anything. */
#define SPT_POOL_MAX_RADIUS 16
#define SPT_POOL_EXCLUDE_CENTER 1u /* other flag bits must be 0 */
/* The pooled map, rows*w*3 floats (DEVICE), enqueued on `stream`: any noise film with batches_done >=
 * 2 (an adaptive one: every pixel's own count). Rejected, nothing queued: a plain film, fewer than
 * two batches, radius outside [1, SPT_POOL_MAX_RADIUS], unknown flag bits. The film's pooling scratch
 * (52 bytes per pixel) is allocated at its first pooled call and freed by spt_film_destroy. */
spt_status spt_film_noise_pool_map(const spt_film* film, int32_t radius, uint32_t flags,
                                   float* se_dev, void* stream);
/* The pooled selection: marks, list, count and the wait on `stream` as spt_film_adaptive_select.
 * Rejected, nothing queued, film untouched: what spt_film_adaptive_select rejects (a NaN threshold, a
 * plain or non-adaptive film, front < 2), a radius outside [1, SPT_POOL_MAX_RADIUS], unknown flag
 * bits. A shard without rows returns SPT_OK and *n_active = 0. */
spt_status spt_film_adaptive_select_pooled(spt_film* film, double se_threshold, int32_t radius,
                                           uint32_t flags, const uint8_t* keep_dev_or_null,
                                           int64_t* n_active, void* stream);
/* Both as pure host functions (no device). counts_or_null: NULL = a uniform noise film (info's
 * samples_done, noise's batches_done >= 2), else an adaptive film's plane. band_rows >= 0 as above. */
spt_status spt_film_noise_pool_map_host(const uint64_t* sums, const uint64_t* m2,
                                        const uint32_t* counts_or_null, const spt_film_info* info,
                                        const spt_film_noise_info* noise, int32_t band_rows,
                                        int32_t radius, uint32_t flags, float* se_out);
spt_status spt_film_adaptive_select_pooled_host(const uint64_t* sums, const uint64_t* m2,
                                                const uint32_t* counts, const spt_film_info* info,
                                                const spt_film_noise_info* noise, int32_t band_rows,
                                                double se_threshold, int32_t radius, uint32_t flags,
                                                const uint8_t* keep_or_null, uint32_t* counts_out,
                                                uint32_t* list_out, int64_t* n_active);

/* ---- guide planes: first-hit albedo, normal, depth and coverage (SPT_HAS_GUIDE) ----
 * The noise-free per-pixel features of the first hit, for a denoiser's edge-stopping terms, an
 * adaptive pass's keep mask or a compositor. For pixel p, sample index s in [0, spp) and the seed, a
 * guide takes THE RENDER'S OWN first ray: Philox counter (p, s, 1, seed), the jitter from the low
 * bytes, the camera's fma chain of contract v5 in its general form, the direction normalised by the
 * scene's direction contract (rsq_nr with a sphere or a REFR primitive in the scene, else rsq_nr1) --
 * and its nearest hit (hit, t, id) of the contract, t the winner's exact t. Each sample that hits adds
 * one record to the pixel's 64-byte record int64[8]; a miss adds nothing (no "primitive 0 on a miss"):
 *   slots 0-2 albedo  fix(c_k), the hit primitive's colour (fp32 as uploaded), fix = the render's own
 *                     1.31 conversion: fminf(c * inv_spp, 1) * 2^31 truncated, inv_spp = 1 / spp
 *   slots 3-5 normal  sgn(nl_k) * fix(fabsf(nl_k)), nl the normal oriented against the ray: a
 *                     rectangle's +-axis, signed by the ray's component on that axis; a sphere's
 *                     gn = (x - centre) * (1 / r), x = o + d * t (a multiply, then an add), negated when
 *                     dot(gn, d) >= 0
 *   slot 6 depth      (uint64)(fminf(t, 2^20) * 65536.0f): a power-of-two scale, then truncation
 *   slot 7 hits       1
 * spp is at most 2^24 (slot 6 cannot overflow; SPT_ERR_INVALID_ARG at creation). All slots are
 * integers, so the sums depend on no lane mapping, window split, window order, shard or GPU: a guide
 * filled with every index of [0, spp) exactly once is one well-defined object. Records are in image
 * pixel order, a shard's guide holds its compact rows (spt_shard_rows), as a film does.
 * Depth is the ray parameter along the contract's direction: the distance where directions are unit,
 * and within the free-scale contract's 1.8e-3 of it in rect-only DIFF scenes. Albedo is the first
 * hit's own colour: in a first-hit guide a mirror or a glass ball reads as its .999; a guide created
 * with SPT_GUIDE_THROUGH_SPECULAR (below) reads what is seen in or through it.
 * The resolve, n = samples_done, r = (float)((double)spp_total / n) (device kernel and host statement
 * run the same IEEE operations):
 *   albedo_k = min(((float)S_k * 2^-31) [* r when n < spp_total], 1)     spt_film_resolve's rule
 *   normal_k = sgn(S_k) * (((float)|S_k| * 2^-31) [* r])     not clamped, not renormalised: a length
 *                                                             below 1 at an edge is information
 *   depth    = hits ? (float)((double)S_6 / ((double)hits * 65536.0)) : 0    the mean over the hits
 *   coverage = (float)((double)hits / (double)n)
 *   n == 0: zeros everywhere.
 *
 * THE SPECULAR CHAIN (SPT_HAS_GUIDE_CHAIN). A guide created by spt_guide_create_ex with
 * SPT_GUIDE_THROUGH_SPECULAR lets the guide ray continue through perfectly specular surfaces and
 * records the first DIFF surface it reaches. The mode belongs to the guide: every pass adds its kind of
 * record, so one guide never mixes the two. Segment 0 is the ray above (same counter, jitter, camera
 * chain, normaliser and nearest hit). A chain carries a throughput A = (1, 1, 1), a length D = 0.0f
 * and a segment count. At the nearest hit of a segment (o, d) on primitive H at parameter t, with the
 * hit point x and the geometric normal gn formed as the render forms them -- x = o + d * tr (a
 * multiply, then an add), tr = t for a sphere and, for a rectangle with plane k on axis a, t after one
 * correction step, fmaf(fmaf(-t, d_a, k - o_a), rcp_nr(d_a), t); gn a rectangle's +axis, a sphere's
 * (x - centre) * (1 / r); nl = gn oriented against d as above:
 *   H is DIFF, or this is segment SPT_GUIDE_MAX_CHAIN - 1 (the eighth): the chain ends and one record
 *     is added: slots 0-2 fix(A_k * c_k), slots 3-5 from nl (the rule above with this segment's d),
 *     slot 6 (uint64)(fminf(D + t, 2^20) * 65536.0f), slot 7 1. An exhausted chain so records its last
 *     specular hit as if it were diffuse.
 *   H is SPEC: A_k = A_k * c_k (fp32, in chain order: the first product is exact), D = D + t, and the
 *     next segment starts at x along the render's reflection d - gn * (2 * dot(gn, d)), the products
 *     and the subtraction rounded separately, renormalised (rsq_nr) where the scene's directions are
 *     unit (contract v8) and left as it is in the free-scale contract: bit for bit the ray the render's
 *     path takes.
 *   H is REFR: A and D as for SPEC (no Fresnel factor: a guide is a feature, not radiance). With
 *     into = dot(gn, nl) > 0, nnt = into ? 1/1.5 : 1.5, ddn = dot(d, nl),
 *     cos2t = 1 - nnt * nnt * (1 - ddn * ddn): when cos2t < 0 (total internal reflection) the next
 *     segment takes the reflection, else the render's refraction direction
 *     normalize(d * nnt - gn * ((into ? 1 : -1) * (ddn * nnt + sqrtf(cos2t)))). The branch is decided,
 *     never drawn: the guide stays noise-free.
 *   A miss on any segment adds nothing, as a first-segment miss does.
 * Depth is then the summed ray parameters along the chain (the optical path length where directions
 * are unit), and the normal is the world-space normal of the surface seen, not the mirror's. Each
 * sample still adds at most 2^36 to slot 6, so spp <= 2^24 bounds it as before. Record layout, resolve,
 * download, the host resolve, windows, shards and spt_film_denoise do not know the mode: a chain guide
 * is a guide. In a scene without SPEC or REFR primitives the two modes hold the same bits. */
typedef struct spt_guide spt_guide;
typedef struct spt_guide_info {
  int32_t width, rows, spp_total; /* rows = the shard's row count */
  int64_t samples_done;           /* samples per pixel added so far, 0 .. spp_total */
  int32_t lanes_per_pixel;        /* lanes of a wave that shared a pixel in the last launch (a power of
                                     two, 1..64: the launch's sizing, never a result); 0 before any */
  uint32_t flags;                 /* the guide's SPT_GUIDE_* flags (0: a first-hit guide) */
} spt_guide_info;
int32_t spt_guide_info_size(void); /* sizeof(spt_guide_info) as the library was built */
/* A zeroed guide on `device` for passes with p's width, height, spp (= spp_total) and shard fields. */
spt_status spt_guide_create(int32_t device, const spt_params* p, spt_guide** out);
/* The same with flags: 0 is spt_guide_create, SPT_GUIDE_THROUGH_SPECULAR a guide of the specular chain.
 * Unknown bits: SPT_ERR_INVALID_ARG (before any device is looked for), *out untouched. */
spt_status spt_guide_create_ex(int32_t device, const spt_params* p, uint32_t flags, spt_guide** out);
spt_status spt_guide_destroy(spt_guide* guide);
spt_status spt_guide_clear(spt_guide* guide, void* stream); /* records and samples_done back to 0 */
spt_status spt_guide_info_get(const spt_guide* guide, spt_guide_info* out);
/* Enqueue the guide pass of the window on `stream`. The rules are a film pass's: p's width, height,
 * spp and shard fields must equal the guide's, the window must lie in [0, spp) with sample_count >= 1,
 * samples_done + sample_count must not exceed spp -- SPT_ERR_INVALID_ARG otherwise, nothing queued, the
 * guide untouched. ctx and guide must be on one device. Keeping windows disjoint is the caller's duty.
 * The pass goes through ctx's scene upload and pinned staging (so spt_render_async's reuse rule
 * holds: a call first waits for the previous call's upload) and must be ordered with ctx's other calls
 * on one stream, but it is no render: spt_context_stats and spt_context_kernel still describe the
 * context's last render. A shard without rows only counts. */
spt_status spt_guide_render_async(spt_context* ctx, spt_guide* guide, const spt_prim* prims,
                                  int32_t n_prims, const spt_camera* cam, const spt_params* p,
                                  int32_t sample_base, int32_t sample_count, void* stream);
/* Guide -> float planes (DEVICE; any of them may be NULL): albedo and normal rows*w*3 floats, depth and
 * coverage rows*w floats. */
spt_status spt_guide_resolve(const spt_guide* guide, float* albedo_dev, float* normal_dev,
                             float* depth_dev, float* coverage_dev, void* stream);
/* The records to HOST memory (rows*w*8 int64, pixel order); waits for its copy on `stream`. */
spt_status spt_guide_download(const spt_guide* guide, int64_t* host_records, void* stream);
/* The resolve as a pure host function (no device); planes may be NULL. Uses info's width, rows,
 * spp_total and samples_done. */
spt_status spt_guide_resolve_host(const int64_t* records, const spt_guide_info* info, float* albedo,
                                  float* normal, float* depth, float* coverage);

/* ---- light guides: per-pixel light visibility and direct irradiance (SPT_HAS_GUIDE_LIGHT) ----
 * The feature the four guide planes lack: what the light does at the surface a pixel sees. A light guide
 * is its own object, spt_light_guide: spt_guide_create_ex keeps refusing every flag but
 * SPT_GUIDE_THROUGH_SPECULAR. It holds one record int64[4] per pixel, in image pixel order; a shard's
 * light guide holds its compact rows, as a guide does. For pixel p, sample s in [0, spp) and the seed:
 *   1. THE SURFACE is the guide's own ray and vertex, operation for operation: Philox counter
 *      (p, s, 1, seed), the jitter, contract v5's camera chain and the scene's normaliser; the nearest
 *      hit (hit, t, id), t the winner's exact t; the hit point x and the oriented normal nl formed as the
 *      chain guide forms them (a rectangle's t after one correction step, x = o + d * tr as a multiply
 *      then an add, a sphere's gn = (x - centre) * (1 / r)). A light guide created with
 *      SPT_GUIDE_THROUGH_SPECULAR follows the chain rule of SPT_HAS_GUIDE_CHAIN to the vertex where the
 *      chain guide takes its record; without it the vertex is the first hit. A miss on any segment adds
 *      nothing.
 *   2. ELIGIBILITY. The sample is TESTED iff the vertex's primitive is SPT_DIFF and its index is not
 *      light_id. The render does no NEE at a SPEC or REFR vertex, so an exhausted chain and a first-hit
 *      mirror are not tested; a vertex on the light is the emitter itself. Otherwise the sample adds
 *      nothing.
 *   3. THE LIGHT POINT. r = philox(p, s, 0, seed): word 2 = 0 is used by no render or guide draw (the
 *      render's vertex words start at 1, stream 1 is 1 | 2^31). xl = fmaf(u01(r.x), light_dx, light_x0),
 *      zl = fmaf(u01(r.y), light_dz, light_z0), yl = light_y: the render's SPT_LIGHT_UNIFORM arithmetic,
 *      used for either light_mode. A LIGHT GUIDE ALWAYS SAMPLES THE INTENDED RECTANGLE, also where the
 *      render's NEE samples the glibc-wrap patch of it (SPT_LIGHT_GLIBC_WRAP): it is a feature, not
 *      radiance.
 *   4. THE SHADOW RAY. dl = (xl - x.x, yl - x.y, zl - x.z), three fp32 subtractions; normalised (rsq_nr)
 *      iff the scene's directions are unit and left as it is in the free-scale contract: the render's
 *      own rule (:466). It is traced from x with the contract's nearest hit. The sample is LIT iff it
 *      hits and the hit's index equals light_id (the reference's test :467, for a light primitive of any
 *      kind; with light_id outside [0, n_prims) nothing is lit).
 *   5. THE WEIGHT of a lit sample is the render's PDF_inverse * BRDF of :471-472 restated operation for
 *      operation, t2 the winner's exact t of the shadow ray and nee_c = (float)((double)light_area / pi):
 *        unit directions: fabsf((light_area * dl.y) * rcp_nr(t2 * t2)) * fabsf(dot(dl, nl) * (1 / pi))
 *        free-scale:      ((fabsf(dl.y) * fabsf(dot(dl, nl))) * nee_c) * rcp_nr((t2 * t2) * (vv * vv)),
 *                         vv = dot(dl, dl)
 *   6. THE RECORD. slot 0 `tested` += 1 for a tested sample; slot 1 `lit` += 1 and slot 2 `weight` +=
 *      fix(wt) for a lit one, fix the render's own 1.31 conversion (fminf(wt * inv_spp, 1) * 2^31,
 *      truncated); slot 3 is reserved and stays 0. spp is at most 2^24, as for a guide.
 * All slots are integers, so the sums depend on no lane mapping, window split, window order, shard or
 * GPU, as a guide's.
 * The resolve, n = samples_done, r = (float)((double)spp_total / n) (device kernel and host statement run
 * the same IEEE operations):
 *   visibility   = tested ? (float)((double)lit / (double)tested) : 0
 *   tested_share = (float)((double)tested / (double)n)
 *   direct       = ((float)S_2 * 2^-31) [* r when n < spp_total]      not clamped
 *   n == 0: zeros everywhere.
 * `direct` is the pixel's mean of V * PDF_inverse * BRDF under uniform sampling of the light rectangle:
 * the direct irradiance factor the render's NEE multiplies the light's emission and the surface's colour
 * by, averaged over the pixel's samples (an untested sample counts as 0). Its per-sample clamp at spp
 * (a sample adds at most 2^31) is the film's own.
 * spt_guide_info describes a light guide too (flags: 0 or SPT_GUIDE_THROUGH_SPECULAR). */
typedef struct spt_light_guide spt_light_guide;
/* A zeroed light guide on `device` for passes with p's width, height, spp (= spp_total) and shard
 * fields. flags: 0 or SPT_GUIDE_THROUGH_SPECULAR. Unknown bits: SPT_ERR_INVALID_ARG (before any device is
 * looked for), *out untouched. */
spt_status spt_light_guide_create(int32_t device, const spt_params* p, uint32_t flags, spt_light_guide** out);
spt_status spt_light_guide_destroy(spt_light_guide* lg);
spt_status spt_light_guide_clear(spt_light_guide* lg, void* stream); /* records and samples_done back to 0 */
spt_status spt_light_guide_info_get(const spt_light_guide* lg, spt_guide_info* out);
/* Enqueue the light-guide pass of the window on `stream`: spt_guide_render_async's rules, rejections
 * (nothing queued, the light guide untouched) and use of ctx's scene upload and pinned staging. It is no
 * render: spt_context_stats and spt_context_kernel still describe the context's last render. The light
 * is p's (light_id, light_x0, light_dx, light_z0, light_dz, light_y, light_area). A shard without rows
 * only counts. */
spt_status spt_light_guide_render_async(spt_context* ctx, spt_light_guide* lg, const spt_prim* prims,
                                        int32_t n_prims, const spt_camera* cam, const spt_params* p,
                                        int32_t sample_base, int32_t sample_count, void* stream);
/* Light guide -> float planes (DEVICE, rows*w floats each; any of them may be NULL). */
spt_status spt_light_guide_resolve(const spt_light_guide* lg, float* visibility_dev, float* direct_dev,
                                   float* tested_dev, void* stream);
/* The records to HOST memory (rows*w*4 int64, pixel order); waits for its copy on `stream`. */
spt_status spt_light_guide_download(const spt_light_guide* lg, int64_t* host_records, void* stream);
/* The resolve as a pure host function (no device); planes may be NULL. Uses info's width, rows,
 * spp_total and samples_done. */
spt_status spt_light_guide_resolve_host(const int64_t* records, const spt_guide_info* info,
                                        float* visibility, float* direct, float* tested);
/* The first consumer: an albedo plane (n_pixels * 3 floats) shaded by a visibility plane (n_pixels),
 *   m = shade_floor + (1.0f - shade_floor) * visibility     a multiply, then an add, no contraction
 *   out_k = albedo_k * m
 * so that a shadow edge becomes an albedo edge for a filter that demodulates by and weights on albedo.
 * shade_floor must be finite and in (0, 1] (SPT_ERR_INVALID_ARG otherwise); 1 leaves the albedo as it is.
 * out may equal albedo. The device call runs on the calling thread's current device, where the planes
 * live; device kernel and host statement run the same IEEE operations. */
spt_status spt_light_shade_async(const float* albedo_dev, const float* visibility_dev, int64_t n_pixels,
                                 float shade_floor, float* out_dev, void* stream);
spt_status spt_light_shade_host(const float* albedo, const float* visibility, int64_t n_pixels,
                                float shade_floor, float* out);

/* ---- denoising: a variance-guided, feature-guided a-trous wavelet filter (SPT_HAS_DENOISE) ----
 * The consumer of a noise film's error map and of the guide planes, in the style of Dammertz et al.
 * 2010 and SVGF: a 5x5 B3-spline filter applied `iterations` times with the tap spacing doubling,
 * every tap weighted down where the normal, the depth, the albedo or the (variance-normalised) colour
 * says that it lies across an edge. Exact fp32 arithmetic: IEEE + - * /, fmaxf, fminf, fabsf and sqrtf
 * only (no exp, no pow), no contraction, every sum in the order given here, so the device kernels and
 * the host statement run the same operations and agree bit for bit.
 * Inputs, for a w x h image in pixel order: rgb (h*w*3, the resolved, clamped image), se (h*w*3, the
 * error map), albedo and normal (h*w*3 each) and depth (h*w) of the guide's resolve. Coverage is no
 * input: a missed or partly covered pixel already has a short normal.
 * Prepare, per pixel: a_k = fmaxf(albedo_k, albedo_floor), or a_k = 1 with SPT_DENOISE_NO_DEMODULATE;
 *   c_k = rgb_k / a_k;  e_k = se_k / a_k;  v = ((e_0*e_0 + e_1*e_1) + e_2*e_2) * (1.0f/3.0f).
 *   The depth gradient gx (along x; gy alike along y): 0.5f * (z(x+1) - z(x-1)) inside, the one-sided
 *   difference z(1) - z(0) or z(w-1) - z(w-2) at a border, 0 on an axis of length 1.
 * Iteration i = 0 .. iterations-1 has step s = 2^i and maps the planes (c, v) to (c', v'); every pixel
 * reads the previous iteration's values. For pixel p = (x, y):
 *   vt(p) = (sum of k*v(q)) / (sum of k) over the 3x3 window at spacing 1, k = (2-|dy|)*(2-|dx|)/16,
 *           rows ascending, then columns; a tap outside the image is skipped; both sums start at 0.0f.
 *   The 25 taps q = (x + i*s, y + j*s), j, i in -2..2, rows (j) ascending, then columns (i). A tap
 *   outside the image is skipped, not added with weight 0 (the two differ when an input is not
 *   finite). h = (1, 4, 6, 4, 1)/16. The centre tap has w = h_2*h_2 by rule. Every other tap has
 *     w = ((((h_j*h_i) * w_n) * w_z) * w_a) * w_c
 *     w_n = fmaxf(0, (nx_p*nx_q + ny_p*ny_q) + nz_p*nz_q), then squared normal_squarings times
 *     w_z = phi(fabsf(z_p - z_q) / ((sigma_depth * fabsf(gx_p*dx + gy_p*dy) + 1e-3f*z_p) + 1e-6f)),
 *           dx = (float)(i*s), dy = (float)(j*s)
 *     w_a = phi(((d_0*d_0 + d_1*d_1) + d_2*d_2) / sigma_albedo^2), d = albedo_p - albedo_q (the planes as
 *           given, not floored)
 *     w_c = phi(((d_0*d_0 + d_1*d_1) + d_2*d_2) / (sigma_color^2 * (vt_p + vt_q) + 1e-10f)), d = c_p - c_q
 *     phi(x) = t^4 as two squarings, t = fmaxf(0, 1 - 0.25f*x)
 *   The squares of the sigmas are taken once on the host in fp32. With W, C_k, V starting at 0.0f, each
 *   tap in order does W += w, C_k += w*c_q,k, V += (w*w)*v_q; then c'_k = C_k / W and v' = V / (W*W).
 *   W >= h_2*h_2 > 0: nothing divides by zero.
 * Finish: out_k = fminf(c_k * a_k, 1), se_out_k = sqrtf(v) * a_k (optional plane). iterations == 0: out
 * is rgb and se_out is se, copied bit for bit (no divide-and-multiply round trip).
 * What it is not. The denoised image is BIASED, unlike a film: it trades variance for blur wherever no
 * guide separates the signal (soft shadow edges, the rim of the light). se_out ignores the correlation
 * that earlier iterations introduce between neighbours: an optimistic estimate, not a bound. Inputs
 * that are not finite give unspecified values, never a fault. */
#define SPT_DENOISE_NO_DEMODULATE 1u /* filter rgb itself, not rgb / albedo; other flag bits must be 0 */
typedef struct spt_denoise_params {
  int32_t iterations;       /* 0..6; iteration i uses step 2^i. Default 5 */
  float sigma_color;        /* finite, > 0. Default 4 */
  float sigma_depth;        /* finite, > 0. Default 1 */
  float sigma_albedo;       /* finite, > 0. Default 0.1 */
  int32_t normal_squarings; /* 0..8: the normal weight is the clamped dot product ^ (2^this). Default 7 */
  float albedo_floor;       /* finite, > 0. Default 0.01 */
  uint32_t flags;           /* SPT_DENOISE_NO_DEMODULATE */
  uint32_t reserved;        /* 0 */
} spt_denoise_params;
void spt_denoise_default_params(spt_denoise_params* p);
/* A denoiser for width x height images on `device`. It owns all its scratch (124 bytes per pixel: two
 * ping-pong planes of (c, v), the packed guides, and five float planes for the film path below),
 * allocated here; no later call allocates. Rejected: width or height not positive, more than 2^31 - 1
 * pixels (the guide's limit), or a shape so narrow or so flat that its tiles do not fit one launch: the
 * kernels cover the image with tiles of 64 x 4 and of 32 x 8 pixels and a launch holds at most 2^24 - 1
 * tiles of either kind (a 1-pixel-wide image may have 2^24 - 1 tiles of 4 rows: 67108860 rows). Calls on
 * one denoiser are serialised by the caller on one stream. */
typedef struct spt_denoiser spt_denoiser;
spt_status spt_denoiser_create(int32_t device, int32_t width, int32_t height, spt_denoiser** out);
spt_status spt_denoiser_destroy(spt_denoiser* dn);
/* Enqueue the filter of five DEVICE planes on `stream`: out_dev (h*w*3) and, if given, se_out_dev
 * (h*w*3). Rejected with SPT_ERR_INVALID_ARG, nothing queued, out untouched: a null plane, a parameter
 * out of range or not finite, unknown flag bits, out_dev or se_out_dev equal to an input pointer or to
 * each other. No host synchronisation. */
spt_status spt_denoise_async(spt_denoiser* dn, const float* rgb_dev, const float* se_dev,
                             const float* albedo_dev, const float* normal_dev, const float* depth_dev,
                             const spt_denoise_params* params, float* out_dev,
                             float* se_out_dev_or_null, void* stream);
/* The same as a pure host function (no device), HOST pointers: the CPU statement of the filter. Also
 * rejects a width or height that is not positive or more than 2^31 - 1 pixels. */
spt_status spt_denoise_host(const float* rgb, const float* se, const float* albedo, const float* normal,
                            const float* depth, int32_t width, int32_t height,
                            const spt_denoise_params* params, float* out, float* se_out_or_null);
/* Film and guide in one call: the film's resolve, its error map and the guide's resolve go into the
 * denoiser's scratch and the filter runs on them, all enqueued on `stream` with no host
 * synchronisation; the result equals spt_denoise_async on the separately resolved planes bit for bit.
 * An adaptive film works unchanged (its resolve and error map take every pixel's own count).
 * Rejected, nothing queued, out untouched: what spt_denoise_async rejects; a plain film; a film with
 * batches_done < 2; a guide with samples_done == 0; a film or guide whose width or rows differ from the
 * denoiser's width and height; a film on another device; a film of a sharded render (shard_count > 1:
 * a shard's compact rows are not image neighbours -- a multi-GPU user gathers the five planes and
 * calls spt_denoise_async on the full image). A sharded guide is refused only through its row count,
 * which is below the image's height whenever another shard holds rows. THE GUIDE'S DEVICE IS NOT
 * CHECKED (a guide's public info does not name it): a guide on the denoiser's device is the caller's
 * duty, and one on another device is undefined behaviour, as a foreign device pointer is. */
spt_status spt_film_denoise(const spt_film* film, const spt_guide* guide, spt_denoiser* dn,
                            const spt_denoise_params* params, float* out_dev, float* se_out_dev_or_null,
                            void* stream);

/* ---- two-half denoising: cross-weighted a-trous and a measured error (SPT_HAS_DENOISE_PAIR) ----
 * The samples are split into two independent halves A and B (two noise films that took disjoint
 * windows: their spt_film_merge is the one-shot film bit for bit). Both halves run the filter above,
 * fused tap by tap; a half's colour weights come from the OTHER half (Rousselle et al. 2012, NFOR), so
 * a pixel's own noise no longer steers its own weights, and half the difference of the two results
 * measures the error of their mean. Same arithmetic rules as above: exact fp32, no contraction, every
 * sum in the order given, device and host agree bit for bit.
 * Inputs, for a w x h image: the halves (rgb_a, se_a) and (rgb_b, se_b), h*w*3 each; albedo, normal,
 * depth shared; an spt_denoise_params, validated as above; pair_flags, separate from params->flags: 0 or
 * SPT_DENOISE_PAIR_OWN_WEIGHTS, other bits rejected.
 * Prepare: each half by the prepare above with the shared divisor a_k: (c^A, v^A), (c^B, v^B). The depth
 *   gradient is the one above.
 * Iteration i (step 2^i): vt^A, vt^B = the 3x3 filter above of v^A, v^B. Tap order, the skipping of taps
 *   outside the image and the centre tap (w = h_2*h_2, both halves) are as above. Every other tap has
 *     g     = (((h_j*h_i) * w_n) * w_z) * w_a                 (shared; w_n, w_z, w_a as above)
 *     w_c^H = phi(((d_0*d_0 + d_1*d_1) + d_2*d_2) / (sigma_color^2 * (vt^H_p + vt^H_q) + 1e-10f)),
 *             d = c^H_p - c^H_q, for H = A and B
 *     w^A = g * w_c^B, w^B = g * w_c^A;   with SPT_DENOISE_PAIR_OWN_WEIGHTS w^A = g * w_c^A, w^B = g * w_c^B
 *   (g * w_c is the product above in its association order: equal halves give the single filter's bits).
 *   Each half keeps its own sums: W += w, C_k += w*c^H_q,k, V += (w*w)*v^H_q; c'^H_k = C_k / W,
 *   v'^H = V / (W*W).
 * Finish: o^H_k = fminf(c^H_k * a_k, 1);  out_k = 0.5f * (o^A_k + o^B_k);
 *   diff_k = 0.5f * (o^A_k - o^B_k), signed (optional plane);
 *   se_out_k = (0.5f * sqrtf(v^A + v^B)) * a_k (optional plane): the propagated estimate, for comparison.
 *   iterations == 0: o^H = rgb^H as given (no divide-and-multiply round trip), out and diff by the same
 *   formulas, se_out_k = 0.5f * sqrtf(se_a_k*se_a_k + se_b_k*se_b_k).
 * Swapping the halves leaves out and se_out bit-identical and negates diff exactly.
 * WHAT diff^2 IS. out = (o^A + o^B) / 2, so with independent halves Var(out) = Var(o^A - o^B) / 4 and
 * diff^2 is an estimate of out's variance with ONE degree of freedom per value: useless for one pixel,
 * meaningful as a mean over many (the summary below). With SPT_DENOISE_PAIR_OWN_WEIGHTS the two results
 * are functions of independent samples and E[diff^2] = Var(out) exactly. With cross weights A's weights
 * are B's data: the results correlate positively and diff^2 reads LOW (measured figures: README). In both
 * modes diff is blind to BIAS: blur that both halves share cancels in the difference, so diff^2 is
 * an estimate of variance, not of the squared error against the true image. */
#define SPT_DENOISE_PAIR_OWN_WEIGHTS 1u /* pair_flags: each half weighted by its own colours */
typedef struct spt_pair_summary {
  double rmse[3];    /* per channel: sqrt(mean over ALL pixels of (double)diff_k * (double)diff_k) */
  double rmse_all;   /* the same over the three channels together */
  float diff_max;    /* the largest fabsf(diff) */
  uint32_t reserved; /* 0 */
} spt_pair_summary;
/* Enqueue the pair filter of seven DEVICE planes on `stream`: out_dev and, if given, se_out_dev and
 * diff_dev (h*w*3 each). The first pair call on a denoiser allocates the pair scratch (a hipMalloc: it
 * may synchronise the device once), 60 bytes per pixel beside spt_denoiser_create's 124 (two more
 * ping-pong planes of (c, v), the second vt plane, the second film's rgb and se planes) and the
 * summary's partials, 32 bytes per 256 pixels; spt_denoiser_destroy frees it. SPT_ERR_OOM if it does not fit. Rejected with
 * SPT_ERR_INVALID_ARG, nothing queued, every output untouched: what spt_denoise_async rejects, unknown
 * pair_flags, an output plane equal to an input plane or to another output plane. */
spt_status spt_denoise_pair_async(spt_denoiser* dn, const float* rgb_a_dev, const float* se_a_dev,
                                  const float* rgb_b_dev, const float* se_b_dev, const float* albedo_dev,
                                  const float* normal_dev, const float* depth_dev,
                                  const spt_denoise_params* params, uint32_t pair_flags, float* out_dev,
                                  float* se_out_dev_or_null, float* diff_dev_or_null, void* stream);
/* The same as a pure host function: the CPU statement. */
spt_status spt_denoise_pair_host(const float* rgb_a, const float* se_a, const float* rgb_b,
                                 const float* se_b, const float* albedo, const float* normal,
                                 const float* depth, int32_t width, int32_t height,
                                 const spt_denoise_params* params, uint32_t pair_flags, float* out,
                                 float* se_out_or_null, float* diff_or_null);
/* The figures of a diff plane (DEVICE, the denoiser's h*w*3). Waits on `stream`. A two-stage reduction
 * in a fixed order (per-block partials, then one block; no floating-point atomics): the same plane gives
 * the same bits every time. The host statement sums in pixel order: the two agree to rounding. */
spt_status spt_denoise_pair_summary(spt_denoiser* dn, const float* diff_dev, spt_pair_summary* out,
                                    void* stream);
spt_status spt_denoise_pair_summary_host(const float* diff, int32_t width, int32_t height,
                                         spt_pair_summary* out);
/* Two films and a guide in one call: both films' resolves and error maps and the guide's resolve go into
 * the denoiser's scratch, then the pair filter, all enqueued on `stream` with no host synchronisation
 * (but the first pair call's allocation, above); the result equals spt_denoise_pair_async on the
 * separately resolved planes bit for bit. Adaptive films work as in spt_film_denoise. Rejected, nothing
 * queued, every output untouched: what spt_denoise_pair_async and spt_film_denoise reject, applied to
 * either film; film_a == film_b; films whose width, rows, spp_total or device differ. */
spt_status spt_film_pair_denoise(const spt_film* film_a, const spt_film* film_b, const spt_guide* guide,
                                 spt_denoiser* dn, const spt_denoise_params* params, uint32_t pair_flags,
                                 float* out_dev, float* se_out_dev_or_null, float* diff_dev_or_null,
                                 void* stream);

/* ---- the filter bank: a cross-validated per-pixel error picks the filter (SPT_HAS_DENOISE_BANK) ----
 * The pair filter run at 1..4 parameter sets (the candidates); per pixel and candidate an estimate of the
 * WHOLE squared error of the candidate's out, bias included, from the other half's noisy pixel
 * (Rousselle et al. 2012; Bitterli et al. 2016); the estimates smoothed along the guides; per pixel the
 * candidate of least estimate; the candidates blended by the smoothed choice. Same arithmetic rules as
 * above: exact fp32, no contraction, every sum in the order given, device and host agree bit for bit.
 * Inputs: the pair filter's seven planes; cands[0..n_cands-1], n_cands in 1..4, each validated as an
 * spt_denoise_params above; the bank parameters, an spt_bank_params as below.
 * 1. Candidates. For each k: o^A_k, o^B_k = the pair filter's finish values o^A, o^B under cands[k] and
 *    bank->pair_flags (iterations == 0: rgb_a, rgb_b as given); out_k = 0.5f * (o^A_k + o^B_k) and
 *    diff_k = 0.5f * (o^A_k - o^B_k), the pair filter's out and diff bit for bit.
 * 2. The cross-validated error of candidate k at a pixel. Per channel c:
 *      rA = o^A_k,c - rgb_b,c;   rB = o^B_k,c - rgb_a,c
 *      e_c = 0.5f * ((rA*rA - se_b,c*se_b,c) + (rB*rB - se_a,c*se_a,c))
 *      m_c = e_c - diff_k,c*diff_k,c
 *    and m_k = ((m_0 + m_1) + m_2) * (1.0f/3.0f). Signed.
 *    Why: with own weights o^A is a function of A's samples and the noise-free guides, so it is
 *    independent of rgb_b and E[rA^2] = MSE(o^A) + Var(rgb_b); se_b^2 is the film's estimate of
 *    Var(rgb_b). So E[e] = bias^2 + Var(o^A), while out's error is bias^2 + Var(o^A)/2 and E[diff^2] =
 *    Var(o^A)/2: E[m] = MSE(out). One value of m is as noisy as one value of diff^2 and may be negative.
 * 3. Smoothing along the guides: error_iterations passes, pass j = 0.. with step 2^j, every pixel reading
 *    the previous pass. The 25 taps in the filter's order, a tap outside the image skipped. A tap's weight
 *    is the pair statement's geometric factor alone, g = (((h_j*h_i) * w_n) * w_z) * w_a with sigma_depth,
 *    sigma_albedo and normal_squarings of cands[0] and the depth gradient above; the centre tap has
 *    g = h_2*h_2 by rule. With W and M_k starting at 0.0f each tap does W += g, M_k += g * m_k(q); then
 *    m_k(p) := M_k / W. No colour enters: the weights are independent of the samples, so a smoothed
 *    estimate is as unbiased as a raw one.
 * 4. Choice: k*(p) = the smallest k whose (smoothed) m_k(p) is least: k* = 0, then for k = 1.. in order
 *    k* = k where m_k(p) < m_k*(p).
 * 5. Blend: one more 5x5 pass at step 1 with the same g: W += g, S_k += g * (k*(q) == k ? 1.0f : 0.0f);
 *    s_k = S_k / W. Then out_c = fminf(sum over k of s_k * out_k,c, 1) and mse = sum over k of
 *    s_k * m_k(p) (the smoothed values at p), both sums from 0.0f with k ascending; choice = k*(p).
 *    With one candidate s_0 = W / W = 1.0f: out is the pair filter's out bit for bit (but a -0, which
 *    only an input below zero can give, becomes +0) and mse is m_0.
 * Swapping the halves leaves out, mse and choice bit-identical.
 * WHAT mse IS NOT. (a) With cross weights (pair_flags 0) o^A depends on B's samples, so rA^2 misses the
 * covariance and e reads LOW; allowed, measured (README), not the default. (b) The least of several noisy
 * estimates reads low by selection, as the adaptive film's pooled error did: with more than one candidate
 * the mean of mse is a slightly optimistic figure (measured: README). (c) rgb is clamped at 1: at the
 * light the estimate reads the clamped values. (d) se is itself an estimate from a few batches. Inputs
 * that are not finite give unspecified values, never a fault (choice stays below n_cands). */
#define SPT_BANK_MAX_CANDIDATES 4
typedef struct spt_bank_params {
  int32_t error_iterations; /* 0..3 smoothing passes of the error estimates. Default 2 */
  uint32_t pair_flags;      /* the pair filter's; default SPT_DENOISE_PAIR_OWN_WEIGHTS */
  uint32_t reserved[2];     /* 0 */
} spt_bank_params;
void spt_denoise_bank_default_params(spt_bank_params* b);
typedef struct spt_bank_summary {
  double mse_mean;  /* the mean over ALL pixels of (double)mse */
  double rmse_est;  /* sqrt(max(0, mse_mean)) */
  double share[4];  /* the fraction of pixels whose choice is k (a value above 3 counts for none) */
  float mse_min, mse_max;
} spt_bank_summary;
/* Enqueue the bank of seven DEVICE planes on `stream`: out_dev (h*w*3 floats) and, if given, mse_dev (h*w
 * floats, signed) and choice_dev (h*w bytes). Every candidate is a whole pair run (nothing is shared
 * between candidates). The first bank call on a denoiser allocates the pair scratch (above) and the bank
 * scratch (a hipMalloc: it may synchronise the device once), 104 bytes per pixel (the two halves' results,
 * four out_k planes, two ping-pong planes of four error estimates) and the summary's partials, 56 bytes per
 * 256 pixels; spt_denoiser_destroy frees it. SPT_ERR_OOM if it does not fit. Rejected with
 * SPT_ERR_INVALID_ARG before anything is queued, every output untouched: a null denoiser, input plane,
 * cands, bank or out_dev; n_cands outside 1..4; a candidate that spt_denoise_async rejects;
 * error_iterations outside 0..3; unknown pair_flags; a nonzero reserved word; an output plane equal to an
 * input plane or to another output plane. */
spt_status spt_denoise_bank_async(spt_denoiser* dn, const float* rgb_a_dev, const float* se_a_dev,
                                  const float* rgb_b_dev, const float* se_b_dev, const float* albedo_dev,
                                  const float* normal_dev, const float* depth_dev,
                                  const spt_denoise_params* cands, int32_t n_cands,
                                  const spt_bank_params* bank, float* out_dev, float* mse_dev_or_null,
                                  uint8_t* choice_dev_or_null, void* stream);
/* The same as a pure host function: the CPU statement. Also rejects a width or height that is not
 * positive or more than 2^31 - 1 pixels. */
spt_status spt_denoise_bank_host(const float* rgb_a, const float* se_a, const float* rgb_b,
                                 const float* se_b, const float* albedo, const float* normal,
                                 const float* depth, int32_t width, int32_t height,
                                 const spt_denoise_params* cands, int32_t n_cands,
                                 const spt_bank_params* bank, float* out, float* mse_or_null,
                                 uint8_t* choice_or_null);
/* The figures of an mse plane and a choice plane (DEVICE, the denoiser's h*w each). Waits on `stream`.
 * The pair summary's two-stage reduction in a fixed order (no floating-point atomics): the same planes
 * give the same bits every time. The host statement sums in pixel order: the two agree to rounding. */
spt_status spt_denoise_bank_summary(spt_denoiser* dn, const float* mse_dev, const uint8_t* choice_dev,
                                    spt_bank_summary* out, void* stream);
spt_status spt_denoise_bank_summary_host(const float* mse, const uint8_t* choice, int32_t width,
                                         int32_t height, spt_bank_summary* out);
/* Two films and a guide in one call, as spt_film_pair_denoise: the result equals spt_denoise_bank_async on
 * the separately resolved planes bit for bit. Rejected, nothing queued, every output untouched: what
 * spt_denoise_bank_async and spt_film_pair_denoise reject (sharded films included). */
spt_status spt_film_pair_denoise_bank(const spt_film* film_a, const spt_film* film_b,
                                      const spt_guide* guide, spt_denoiser* dn,
                                      const spt_denoise_params* cands, int32_t n_cands,
                                      const spt_bank_params* bank, float* out_dev, float* mse_dev_or_null,
                                      uint8_t* choice_dev_or_null, void* stream);

/* ---- temporal accumulation: the last frame's film reprojected through the guides (SPT_HAS_TEMPORAL) ----
 * The temporal half of SVGF in front of the a-trous filter above: the previous frame's accumulated colour
 * and variance are reprojected into the new camera, tested against the geometry and blended with the new
 * frame, and the filter is handed an input with a smaller se. Exact fp32 arithmetic as the filter's: IEEE
 * + - * /, fmaxf, fminf, fabsf, sqrtf, floorf and one float -> int conversion that is reached only after
 * float range checks; no contraction; every sum in the order given here, so the kernel and the host
 * statement agree bit for bit.
 * Inputs, for a w x h frame in pixel order (y = 0 the top row): rgb, se, albedo, normal (h*w*3 each) and
 * depth (h*w), the five planes of spt_denoise_async; the frame's camera; an spt_temporal_params.
 * State, kept between calls, per pixel: colour c[3], variance v[3], length n, world position X[3] and
 * normal N[3] (13 floats, the planes of an spt_temporal_state), and the camera that made them. The
 * object holds two copies, used ping-pong: a frame gathers from its predecessor's neighbours while it
 * writes its own.
 * Host constants, computed in double and rounded to fp32 once per value. For a camera: o = origin,
 * E = lower_left_corner - origin, Hx = horizontal / w, Vy = vertical / h. For the previous camera
 * (primed below): M, the inverse of the 3x3 matrix with the columns (Hx', Vy', E'), by cofactors:
 * rows (Vy' x E') / det, (E' x Hx') / det, (Hx' x Vy') / det with det = (Hx'_0*r_0 + Hx'_1*r_1) + Hx'_2*r_2,
 * r = Vy' x E'. A camera whose det is 0 or whose constants are not finite is rejected (SPT_ERR_INVALID_ARG)
 * in the call that brings it. These are the pixel's MEAN ray under the contract's jitter: a sample's
 * su = (x - 0.5 + ju) / w with ju uniform on [0, 1) has the mean x / w, and sv likewise has the mean
 * (h - 1 - y) / h: the reference's own half-pixel quirk (tests/guide_truth.py, camera_rays, builds the
 * same ray sample by sample: its fx and fy are x - 0.5 and h - 1 - y - 0.5 before the jitter is added).
 * Per pixel (x, y):
 * 1. The current estimate. a_k = fmaxf(albedo_k, albedo_floor), or 1 with SPT_TEMPORAL_NO_DEMODULATE;
 *    c_k = rgb_k / a_k;  e_k = se_k / a_k;  var_k = e_k * e_k.
 * 2. The world point. D_k = (E_k + Hx_k * (float)x) + Vy_k * (float)(h - 1 - y);
 *    len = sqrtf((D_0*D_0 + D_1*D_1) + D_2*D_2);  X_k = o_k + (D_k / len) * z, z the pixel's depth. A pixel
 *    with z == 0 (a miss) has no surface: it takes no history and its state and n_out get n = 0, which
 *    no later tap accepts.
 * 3. The previous pixel. q = X - o';  (A, B, C) = M q, rows in order, each (m_0*q_0 + m_1*q_1) + m_2*q_2.
 *    History is refused unless C > 0. fx = A / C;  fy = (float)(h - 1) - B / C. History is refused unless
 *    fx >= -1, fx < (float)w, fy >= -1 and fy < (float)h (float compares: a NaN fails them).
 *    x0 = floorf(fx), tx = fx - x0, and y0, ty likewise.
 * 4. The taps (x0 + i, y0 + j), j then i in {0, 1}. A tap outside the image is skipped. Its weight is
 *    b = (i ? tx : 1 - tx) * (j ? ty : 1 - ty). A tap q is valid iff n_q > 0, and
 *    (N_p,0*N_q,0 + N_p,1*N_q,1) + N_p,2*N_q,2 >= normal_min with N_p the current normal as given (a short
 *    normal at an edge fails this on purpose), and fabsf((N_p,0*d_0 + N_p,1*d_1) + N_p,2*d_2) <=
 *    plane_tol * z_p with d = X_q - X_p. With W, Ch_k, Vh_k, Nh starting at 0.0f, each valid tap in order
 *    does W += b, Ch_k += b*c_q,k, Vh_k += b*v_q,k, Nh += b*n_q. History is refused unless W >= 0.25f;
 *    otherwise c_h = Ch / W, v_h = Vh / W, n_h = Nh / W.
 * 5. The same-camera rule. When the twelve doubles of the previous camera equal the current camera's
 *    (the host decides once per call), steps 3 and 4 use the single tap (x, y) with b = 1 under the same
 *    validity tests: progressive use with a static camera has no resampling blur at all.
 * 6. The blend. n' = fminf(n_h + 1, n_max);  alpha = 1 / n';  beta = 1 - alpha;
 *    c'_k = beta*c_h,k + alpha*c_k;  v'_k = (beta*beta)*v_h,k + (alpha*alpha)*var_k. With history refused,
 *    or on the first frame: c' = c, v' = var, n' = 1 (0 at a miss).
 * 7. The outputs. rgb_out_k = fminf(c'_k * a_k, 1);  se_out_k = sqrtf(v'_k) * a_k; the optional plane
 *    n_out (h*w) = n'; the optional plane hist (h*w*3) = c_h,k * a_k, or rgb_k copied where history was
 *    refused (for debugging and tests). The new state is (c', v', n', X, N_p) and the camera.
 * What it is not. There are no motion vectors: the scene must be static between frames, and a moved
 * primitive is either refused by the tests of step 4 or ghosts. A first-hit guide reprojects a mirror's
 * surface, not what is seen in it, so reflections and refractions lag the camera; a chain guide's depth
 * is an optical length, not a position, and the film path refuses it. v' treats frames as independent and
 * the bilinear taps as one sample: an estimate, like se_out of the filter. While n' < n_max a static
 * camera gives v' = var / n'; once n' stays at n_max the blend is an exponential average and v' falls on
 * towards var / (2 n_max - 1). plane_tol's default 0.01 sits five times above the 1.8e-3 relative depth
 * error that the free-scale direction contract allows. Inputs that are not finite give unspecified
 * values, never a fault: no address is formed before the range checks of steps 3 and 4. */
#define SPT_TEMPORAL_NO_DEMODULATE 1u /* accumulate rgb itself, not rgb / albedo; other flag bits must be 0 */
typedef struct spt_temporal_params {
  float n_max;        /* finite, >= 1: the history's length at most. Default 32 */
  float normal_min;   /* -1..1. Default 0.9 */
  float plane_tol;    /* finite, >= 0. Default 0.01 */
  float albedo_floor; /* finite, > 0. Default 0.01 */
  uint32_t flags;     /* SPT_TEMPORAL_NO_DEMODULATE */
  uint32_t reserved;  /* 0 */
} spt_temporal_params;
void spt_temporal_default_params(spt_temporal_params* p);
/* The 13 planes of a state, HOST pointers: c, v, X, N of h*w*3 floats, n of h*w. */
typedef struct spt_temporal_state {
  float *c, *v, *n, *X, *N;
} spt_temporal_state;
typedef struct spt_temporal_info {
  int64_t frames;        /* accepted accumulate calls since creation or the last reset */
  int32_t width, height;
  int32_t has_history;   /* frames > 0: the next call reprojects */
  int32_t reserved;
} spt_temporal_info;
/* An accumulator for width x height frames on `device`. It owns the two copies of the state (52 bytes
 * per pixel each: three 16-byte words and a float) and five planes for the film path below, allocated
 * here; no later call allocates on the device. Rejected: width or height not positive, more than
 * 2^31 - 1 pixels, or a shape whose tiles of 64 x 4 pixels do not fit one launch (2^24 - 1 tiles). Calls
 * on one accumulator are serialised by the caller on one stream. */
typedef struct spt_temporal spt_temporal;
spt_status spt_temporal_create(int32_t device, int32_t width, int32_t height, spt_temporal** out);
spt_status spt_temporal_destroy(spt_temporal* tp);
/* Drop the history: the next frame is a first frame. Queues nothing. */
spt_status spt_temporal_reset(spt_temporal* tp);
spt_status spt_temporal_info_get(const spt_temporal* tp, spt_temporal_info* out);
/* Enqueue one frame of five DEVICE planes on `stream`: rgb_out_dev and se_out_dev (h*w*3 each) and, if
 * given, n_out_dev (h*w) and hist_dev (h*w*3). No host synchronisation. Rejected with
 * SPT_ERR_INVALID_ARG, nothing queued, the outputs and the state untouched: a null plane, a parameter
 * that is not finite or out of range, unknown flag bits, a nonzero reserved word, a singular camera, an
 * output pointer equal to an input or to another output. */
spt_status spt_temporal_accumulate_async(spt_temporal* tp, const float* rgb_dev, const float* se_dev,
                                         const float* albedo_dev, const float* normal_dev,
                                         const float* depth_dev, const spt_camera* cam,
                                         const spt_temporal_params* params, float* rgb_out_dev,
                                         float* se_out_dev, float* n_out_dev_or_null,
                                         float* hist_dev_or_null, void* stream);
/* The same as a pure host function (no device), HOST pointers: the CPU statement. prev and prev_cam are
 * the previous state and its camera, both NULL on a first frame; next receives the new state (its planes
 * are outputs: none may be an input, a plane of prev or another output). Also rejects a width or height
 * that is not positive or more than 2^31 - 1 pixels. */
spt_status spt_temporal_accumulate_host(const float* rgb, const float* se, const float* albedo,
                                        const float* normal, const float* depth, int32_t width,
                                        int32_t height, const spt_camera* cam,
                                        const spt_temporal_params* params,
                                        const spt_temporal_state* prev_or_null,
                                        const spt_camera* prev_cam_or_null, float* rgb_out, float* se_out,
                                        float* n_out_or_null, float* hist_or_null,
                                        const spt_temporal_state* next);
/* The state of the last accepted frame into 13 HOST planes, and its camera if asked. Waits on `stream`.
 * Rejected: no frame since the last reset. For tests and checkpoints. */
spt_status spt_temporal_state_download(spt_temporal* tp, const spt_temporal_state* out,
                                       spt_camera* cam_out_or_null, void* stream);
/* Film and guide in one call: the film's resolve, its error map and the guide's resolve go into the
 * accumulator's planes and the frame is accumulated from them, all enqueued on `stream` with no host
 * synchronisation; the result equals spt_temporal_accumulate_async on the separately resolved planes bit
 * for bit. Where albedo_out_dev, normal_out_dev (h*w*3) or depth_out_dev (h*w) is given, the guide's
 * plane is resolved there instead, so that spt_denoise_async can follow without a second resolve. An
 * adaptive film works unchanged. Rejected, nothing queued, outputs and state untouched: what
 * spt_temporal_accumulate_async rejects (the three planes count as outputs); what spt_film_denoise rejects
 * (a plain film, batches_done < 2, an empty guide, a size or device mismatch, a sharded film); a guide
 * created with SPT_GUIDE_THROUGH_SPECULAR. The guide's device is the caller's duty, as there. */
spt_status spt_film_temporal_accumulate(const spt_film* film, const spt_guide* guide, spt_temporal* tp,
                                        const spt_camera* cam, const spt_temporal_params* params,
                                        float* rgb_out_dev, float* se_out_dev, float* n_out_dev_or_null,
                                        float* hist_dev_or_null, float* albedo_out_dev_or_null,
                                        float* normal_out_dev_or_null, float* depth_out_dev_or_null,
                                        void* stream);

/* ---- multi-GPU: row-tile shards and ONE framebuffer gather over RCCL ----
 * The reference's only parallel construct is the OpenMP pragma over its row loop (:526-528). Here
 * rows are sharded in tiles of tile_rows across ranks (tile t -> rank t % n, spt_shard_rows);
 * every rank renders its rows with spt_render_async into a compact buffer, and rank 0 receives
 * all of them in one grouped ncclSend/ncclRecv over xGMI and de-interleaves the tiles into the
 * image (h*w*3 floats). The image is bit-identical for any rank count. */
#define SPT_COMM_ID_BYTES 128
typedef struct spt_comm spt_comm;
/* One process per GPU: rank 0 creates the id and the caller hands it to every rank (any channel). */
spt_status spt_comm_unique_id(uint8_t id[SPT_COMM_ID_BYTES]);
spt_status spt_comm_create(const uint8_t id[SPT_COMM_ID_BYTES], int32_t nranks, int32_t rank,
                           int32_t device, spt_comm** out);
spt_status spt_comm_destroy(spt_comm* comm);
/* Allocate rank 0's receive slots for renders of this size ahead of a timed loop (optional). */
spt_status spt_comm_reserve(spt_comm* comm, const spt_params* p);
/* The gather, enqueued on `stream` after this rank's render: shard_dev = the rank's compact rows
 * (spt_render_async's output for p with shard_index = rank), image_dev = the full image on rank 0
 * (ignored elsewhere). p->shard_count must equal nranks. No host synchronisation. */
spt_status spt_gather_framebuffer(spt_comm* comm, const spt_params* p, const float* shard_dev,
                                  float* image_dev, void* stream);
/* The de-interleave alone (rank 0's last step): shards_dev[k] = shard k's compact rows (device
 * pointers on the current device), image_dev = h*w*3 floats. */
spt_status spt_deinterleave_rows(const spt_params* p, int32_t nranks, const float* const* shards_dev,
                                 float* image_dev, void* stream);
/* The gather as pure host functions (no device, no RCCL; spt_gather_framebuffer executes exactly
 * this plan): the transfers `rank` posts inside the gather's ncclGroupStart/End. Rank k > 0 sends
 * its compact shard (count = its rows * w * 3 floats) to rank 0; rank 0 receives each rank k > 0
 * that owns rows into its staging buffer at offset (k - 1) * (shard 0's floats) -- shard 0 never
 * owns fewer rows than another shard. Returns the number of ops (<= cap), or -1 on bad arguments
 * or a too small cap. */
typedef struct spt_gather_op {
  int32_t kind;    /* SPT_GATHER_SEND or SPT_GATHER_RECV */
  int32_t peer;    /* the other rank */
  uint64_t count;  /* floats */
  uint64_t offset; /* RECV: float offset into rank 0's staging buffer; SEND: 0 */
} spt_gather_op;
enum { SPT_GATHER_SEND = 0, SPT_GATHER_RECV = 1 };
int32_t spt_gather_plan(const spt_params* p, int32_t nranks, int32_t rank, spt_gather_op* ops,
                        int32_t cap);
uint64_t spt_gather_staging_floats(const spt_params* p, int32_t nranks); /* rank 0's staging size */
/* Where rank 0's de-interleave reads image row `row`: shard *rank's compact row *compact_row (the
 * device kernel's own row map). */
spt_status spt_deinterleave_source(const spt_params* p, int32_t nranks, int32_t row, int32_t* rank,
                                   int32_t* compact_row);
/* One process driving n_dev GPUs (smallpt_amd --devices N): shard k renders on devices[k]
 * (distinct), the gather lands on devices[0], rgb_out = the full image on the host (h*w*3 floats).
 * p's shard fields are ignored. stats: summed over devices, kernel_ms = the slowest device's. */
spt_status spt_render_multi(const spt_prim* prims, int32_t n_prims, const spt_camera* cam,
                            const spt_params* p, const int32_t* devices, int32_t n_dev,
                            float* rgb_out, spt_stats* stats);

/* ---- image output (:313-321 toInt/clamp, :548-551 the P3 writer) ----
 * The encoder turns a DEVICE framebuffer (h*w*3 floats, row-major, y=0 top: what spt_render_async
 * writes) into file bytes on the GPU. P3 is byte-identical to the reference's fprintf loop
 * ("P3\n%d %d\n%d\n" then "%d %d %d " per pixel, toInt = int(pow(clamp(x), 1/2.2)*255 + .5) in
 * double); P6 is its binary form; PFM is the linear framebuffer ("PF", scale -1 = little endian,
 * scanlines bottom to top, header padded so the floats are dword-aligned). */
typedef enum spt_image_format { SPT_IMAGE_P3 = 0, SPT_IMAGE_P6 = 1, SPT_IMAGE_PFM = 2 } spt_image_format;
typedef struct spt_encoder spt_encoder;
uint64_t spt_image_bound(int32_t w, int32_t h, int32_t format); /* max encoded bytes (0 if invalid) */
spt_status spt_encoder_create(int32_t device, spt_encoder** out);
spt_status spt_encoder_destroy(spt_encoder* enc);
/* Encode on `stream` into out_dev (cap bytes). *len_out = encoded length. P3's length depends on
 * the data, so P3 synchronises `stream` once (after its passes); P6/PFM do not. rgb_dev must be
 * 16-byte aligned (SPT_ERR_INVALID_ARG otherwise; P6/PFM also need out_dev past the header 16-byte
 * aligned) and 3*w*h <= 2^32 - 8192; a call rejected for its arguments queues nothing and leaves
 * out_dev untouched. One encoder runs one encode at a time (its scratch is reused). */
spt_status spt_encode_image(spt_encoder* enc, const float* rgb_dev, int32_t w, int32_t h,
                            int32_t format, uint8_t* out_dev, uint64_t cap, uint64_t* len_out,
                            void* stream);
/* Encode (rgb: host or device pointer) and write the file. Replaces the writer of :548-551. */
spt_status spt_write_image(int32_t device, const float* rgb, int32_t w, int32_t h, int32_t format,
                           const char* path);

/* ---- introspection ---- */
int32_t spt_abi_version(void);
/* sha256[:16] of the kernel sources this library was built from (the Makefile's HASHED list; equals
 * the Python package's kernel_sources_sha16() over an unchanged tree). */
const char* spt_build_sources_sha16(void);
const char* spt_status_string(spt_status s);
const char* spt_last_error(void); /* thread-local text of the last failure */
int32_t spt_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* SPT_H_ */

// smallpt_main.cpp — the reference's main() (smallpt.cpp:502-557) on the MI355X:
//   smallpt_amd [W H SPP [SEED [OUT.ppm]]] [--cos] [--uniform] [--reference-leaks] [--q Q]
//               [--specular | --classic | --mirror-glass | --spheres32 [--max-depth D]]
//               [--device N | --devices N] [--p6 | --pfm]
//               [--noise T [--batch B] [--adaptive [--min-batches M] [--pool R [--pool-loo]]]]
//               [--guides PREFIX] [--denoise [--denoise-iters N] [--denoise-sigma S]
//               [--pair [--pair-own] [--bank S,S,.. [--bank-map PREFIX]]]] [--through-specular] [--help]
//               [--light] [--light-guide [--shade-floor F]]
//               [--frames N --orbit DEG [--temporal [--temporal-nmax M]]]
//   --frames N --orbit DEG: N frames, frame k from LOOKFROM rotated about the vertical axis through the
//               look-at point by k * DEG degrees, with the seed SEED + k, each through a noise film
//               (every sample, 8 batches or --batch B). The frame index goes before OUT's extension:
//               image.ppm -> image.0000.ppm ... With --denoise each frame is filtered (--denoise-iters and
//               --denoise-sigma as given; a first-hit guide of min(SPP, 64) samples). --temporal: every
//               frame is first accumulated over the frames before it (spt_film_temporal_accumulate:
//               the last frame's film reprojected through the guide's depth and normal; the scene does
//               not move), --temporal-nmax M the history's length at most (default 32). One device; not
//               with --noise, --film, --passes, --repeat, --guides, --pair, --adaptive,
//               --through-specular or --light-guide.
//   --light (with --guides PREFIX): also PREFIX_visibility.pfm and PREFIX_direct.pfm, the light guide's
//               planes (spt_light_guide_*) of the same window and kind as the guide's, grey like the depth.
//   --light-guide (with --denoise, also with --pair; not with --bank): the guide's albedo plane is shaded
//               by the visibility of a light guide over the guide's window (spt_light_shade_async,
//               --shade-floor F in (0, 1], default 0.25) before the filter takes it, so a shadow edge
//               stops the filter as an albedo edge does. The planes are then resolved one by one and
//               filtered by spt_denoise_async / spt_denoise_pair_async.
//   --bank S,S,.. (with --denoise --pair): the filter bank (spt_film_pair_denoise_bank): one candidate per
//               colour sigma in the list (1 to 4 of them), each half weighted by its own colours, three
//               smoothing passes of the error estimates, per pixel the candidate of least cross-validated
//               error, blended. Prints "BANK : rmse_est
//               share.. after N / SPP": the bank summary's estimate of the output's RMSE, bias included,
//               and the fraction of pixels that chose each candidate. With --noise T the run stops on
//               rmse_est. --bank-map PREFIX also writes PREFIX_mse.pfm (the blended estimate of the squared
//               error, signed, replicated to three channels) and PREFIX_choice.pgm (binary P5, the chosen
//               candidate's index times 85). Not with --denoise-sigma.
//   --pair (with --denoise): two-half denoising (spt_film_pair_denoise). The batches go alternately
//               into two noise films (even batch indices into A, odd into B; SPP / B must be even and
//               at least 4), each half is filtered with colour weights taken from the other half, and
//               the output is the mean of the two results. Prints "PAIR : r g b after N / SPP", the RMS
//               of half the difference of the two results per channel (spt_denoise_pair_summary).
//               --pair-own: each half is weighted by its own colours (SPT_DENOISE_PAIR_OWN_WEIGHTS):
//               the image of the single filter, and a PAIR figure that is an unbiased estimate of the
//               output's variance (with cross weights it reads low, include/spt.h). With --noise T the
//               run stops on that figure instead of the film's: after every second batch from
//               --min-batches (default 4) on, once the largest channel's is at most T. Not with
//               --adaptive, --film or --passes.
//   --through-specular: with --guides and / or --denoise, the guide follows mirrors and glass to the
//               first diffuse surface (spt_guide_create_ex, SPT_GUIDE_THROUGH_SPECULAR); alone it is a
//               usage error.
//   --denoise: the output file becomes the image denoised by the edge-stopping a-trous filter
//               (spt_film_denoise: the film's image and error map, and guide planes of the first
//               min(SPP, 64) samples' camera rays). The render goes through a noise film: --noise T
//               and --batch B as given (with --adaptive if wanted), else every sample in 8 batches (or
//               --batch B). --denoise-iters N (0..6, default 5) and --denoise-sigma S (the colour
//               sigma, default 4) replace those two defaults. One device (no --devices above 1).
//   --guides PREFIX: beside the image, the guide planes of the same scene, camera, W H SPP and SEED
//               (spt_guide_*: the first hit of every sample's own camera ray) as PREFIX_albedo.pfm,
//               PREFIX_normal.pfm and PREFIX_depth.pfm. The PFM encoder writes the floats as they
//               are, so the normal is stored signed (components in [-1, 1], not 0.5 + 0.5 n) and the
//               depth (the mean ray parameter of the samples that hit) is replicated to the three
//               channels. The image file is the same bytes as without the flag.
//   --uniform: random_scattering from the commented-out uniform hemisphere code (:352-359)
//   --reference-leaks: leaked paths go on from the miss vertex as the reference's (:371-377)
//                      instead of ending at their first miss (SPT_FLAG_REFERENCE_LEAKS)
//   --q Q: the NEE-mix probability of :464 (`q < Q`; 1 = HEAD, 0 = --cos)
//   --specular: smallpt's mirror and glass balls (SPEC/REFR, :481-495) in the HEAD room
//   --classic: the classic smallpt sphere box of the shipped image*.ppm (pure path tracing)
//   --mirror-glass: that box with smallpt's mirror and glass balls (pure path tracing)
//   --spheres32: config 5's 32-sphere scene (room + light of :288-294 and 32 DIFF spheres)
//   --devices N: row tiles sharded over GPUs 0..N-1, one RCCL gather to GPU 0 (spt_render_multi)
//   --repeat N: render N times (spt_render keeps its device context between calls) and print
//               each call's wall time beside its kernel time (tools/dropin_e2e.py)
//   --passes K: render the SPP samples as K near-equal sample windows through a film (spt_film_*):
//               the same file as without it, bit for bit
//   --film PATH [--add N]: progressive rendering with a checkpoint. Loads the film PATH if it exists
//               (it must match W H SPP; else starts empty), renders the next N samples of the SPP
//               (default: all that remain; the film holds the samples [0, samples_done)), saves the
//               film and writes the image resolved from it (a preview while samples remain). Fails
//               when the film is full. Film file: 32-byte header (magic "SPTFILM1", int32 width,
//               rows, spp_total, 0, int64 samples_done; little endian), then the raw uint64 sums.
//   --noise T [--batch B]: render until the image's estimated RMSE (spt_film_noise_summary: the
//               largest of the three channels') is at most T, in batches of B samples (default SPP / 8
//               when 8 divides SPP, else --batch is required; B must divide SPP into >= 2 batches),
//               at least two batches and at most SPP samples. Prints "NOISE : r g b after N / SPP".
//               --noise 0 renders every batch: the same file as without it, bit for bit. With --film
//               the checkpoint is a noise film's ("SPTFILM2": the header goes on with int32 batch, 0,
//               int64 batches_done -- 48 bytes --, and the moment plane, rows*width*3 pairs (lo, hi)
//               of uint64, follows the sums) and --add N (a multiple of B) caps this run's samples.
//   --adaptive (with --noise T): the samples go where the error is (spt_film_adaptive_*). Full
//               batches until M (--min-batches, default 4, at least 2); after every pass from then on
//               the run ends once the estimated RMSE is at most T, otherwise the pixels whose every
//               channel has a standard error <= T retire and the next pass renders the rest, until
//               none is left or every batch is in. Prints "SAMPLES_TOTAL : N" (the pixel-samples
//               spent) beside DURATION. Not with --film: the counts plane has no file format.
//   --pool R [--pool-loo] (with --adaptive): a pixel retires on the error pooled over its (2R + 1)^2
//               neighbourhood (spt_film_adaptive_select_pooled, R in 1..16) instead of its own
//               estimate; --pool-loo leaves the pixel itself out of its window
//               (SPT_POOL_EXCLUDE_CENTER), so that the decision does not depend on its own samples.
// Same scene, camera (:521), clamp/toInt and P3 output; the pixel loop is one spt_render() call.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>

#include <hip/hip_runtime_api.h>

#include "smallpt.hpp"

using namespace smallpt_amd;

namespace {

struct FilmHeader {  // the film file's first 32 bytes (little endian)
  char magic[8];
  int32_t width, rows, spp_total, zero;
  int64_t samples_done;
};
static_assert(sizeof(FilmHeader) == 32, "film file header");
const char kFilmMagic[8] = {'S', 'P', 'T', 'F', 'I', 'L', 'M', '1'};
struct NoiseHeader {  // a noise film's file goes on with these 16 bytes
  int32_t batch, zero;
  int64_t batches_done;
};
static_assert(sizeof(NoiseHeader) == 16, "noise film file header");
const char kFilmMagicNoise[8] = {'S', 'P', 'T', 'F', 'I', 'L', 'M', '2'};

struct NoiseOpts {
  bool on = false;
  double target = 0.0;
  int batch = 0;  // 0: SPP / 8
  bool adaptive = false;
  int min_batches = 4;
  int pool_radius = 0;  // 0: a pixel retires on its own estimate
  bool pool_loo = false;
  int64_t samples_total = -1;  // out: the pixel-samples an adaptive run spent
};

struct DenoiseOpts {
  bool on = false;
  bool iters_given = false, sigma_given = false;  // not given: the library's default
  bool through_specular = false;                  // the guide follows the specular chain
  int iters = 0;
  double sigma = 0.0;
  bool pair = false, pair_own = false;  // --pair [--pair-own]: two films, spt_film_pair_denoise
  bool light_guide = false;             // --light-guide: the albedo plane shaded by a light guide's visibility
  float shade_floor = 0.25f;            // --shade-floor F: the shade of a fully shadowed pixel, in (0, 1]
  std::vector<float> bank;              // --bank S,S,..: the candidates' colour sigmas (spt_film_pair_denoise_bank)
  const char* bank_map = nullptr;       // --bank-map PREFIX
};

void check(spt_status s) {
  if (s != SPT_OK) throw std::runtime_error(std::string(spt_status_string(s)) + ": " + spt_last_error());
}

// --denoise --light-guide: the guide's planes resolved one by one into a new DEVICE buffer -- albedo,
// normal (3 floats a pixel each), depth, visibility (1 each) -- with the albedo shaded by the visibility
// of a light guide over the guide's own window and of its kind (spt_light_shade_async, in place).
float* shaded_guides(spt_context* ctx, const spt_guide* guide, const std::vector<spt_prim>& scene,
                     const Camera& cam, const spt_params& p, const DenoiseOpts& denoise) {
  const size_t npix = (size_t)p.width * (size_t)p.height;
  float* dev = nullptr;
  if (hipMalloc(&dev, std::max<size_t>(npix, 1) * 8 * sizeof(float)) != hipSuccess)
    throw std::runtime_error("device allocation failed");
  spt_light_guide* lg = nullptr;
  check(spt_light_guide_create(p.device, &p, denoise.through_specular ? SPT_GUIDE_THROUGH_SPECULAR : 0u, &lg));
  check(spt_light_guide_render_async(ctx, lg, scene.data(), (int32_t)scene.size(), &cam.abi(), &p, 0,
                                     std::min(p.spp, 64), nullptr));
  check(spt_guide_resolve(guide, dev, dev + 3 * npix, dev + 6 * npix, nullptr, nullptr));
  check(spt_light_guide_resolve(lg, dev + 7 * npix, nullptr, nullptr, nullptr));
  check(spt_light_shade_async(dev, dev + 7 * npix, (int64_t)npix, denoise.shade_floor, dev, nullptr));
  if (hipDeviceSynchronize() != hipSuccess) throw std::runtime_error("light guide failed on the device");
  check(spt_light_guide_destroy(lg));
  return dev;
}

// SPP samples through a film: `passes` near-equal windows of the samples to render -- all of them,
// or with film_path the next `add` after those the film file holds. With noise.on the film keeps
// its moment plane, the passes are the batches in index order, and the run ends early once the
// estimated RMSE is at most noise.target. Returns the DEVICE image.
float* render_film(const std::vector<spt_prim>& scene, const Camera& cam, const spt_params& p,
                   int passes, const char* film_path, int add, NoiseOpts& noise,
                   const DenoiseOpts& denoise, spt_stats* total) {
  spt_context* ctx = nullptr;
  spt_film* film = nullptr;
  check(spt_context_create(p.device, &ctx));
  check(spt_film_create(p.device, &p, &film));
  spt_film_info info{};
  check(spt_film_info_get(film, &info));
  const size_t n = 3ull * (size_t)info.rows * (size_t)info.width;
  std::vector<uint64_t> sums(n), m2(noise.on ? 2 * n : 0);
  int batch = 0;
  if (noise.on) {
    if (noise.batch <= 0 && p.spp % 8 != 0)
      throw std::runtime_error("--noise: SPP is no multiple of 8, give --batch");
    batch = noise.batch > 0 ? noise.batch : p.spp / 8;
    check(spt_film_noise_enable(film, batch));
    if (noise.adaptive) check(spt_film_adaptive_enable(film));
  }
  const char* magic = noise.on ? kFilmMagicNoise : kFilmMagic;
  if (film_path) {
    std::ifstream in(film_path, std::ios::binary);
    if (in) {
      FilmHeader h{};
      in.read((char*)&h, sizeof h);
      if (in && std::memcmp(h.magic, noise.on ? kFilmMagic : kFilmMagicNoise, 8) == 0)
        throw std::runtime_error(std::string(film_path) + (noise.on ? ": a plain film (no --noise)"
                                                                    : ": a noise film (--noise)"));
      if (!in || std::memcmp(h.magic, magic, 8) != 0)
        throw std::runtime_error(std::string(film_path) + ": not a film file");
      NoiseHeader nh{};
      if (noise.on) {
        in.read((char*)&nh, sizeof nh);
        if (!in) throw std::runtime_error(std::string(film_path) + ": truncated or oversized film file");
        if (nh.batch != batch) throw std::runtime_error(std::string(film_path) + ": the film has another --batch");
      }
      if (h.width != info.width || h.rows != info.rows || h.spp_total != info.spp_total)
        throw std::runtime_error(std::string(film_path) + ": the film is not W H SPP");
      in.read((char*)sums.data(), (std::streamsize)(n * sizeof(uint64_t)));
      if (noise.on) in.read((char*)m2.data(), (std::streamsize)(2 * n * sizeof(uint64_t)));
      if (!in || in.peek() != std::ifstream::traits_type::eof())
        throw std::runtime_error(std::string(film_path) + ": truncated or oversized film file");
      check(spt_film_upload(film, sums.data(), h.samples_done, nullptr));
      if (noise.on) check(spt_film_noise_upload(film, m2.data(), nh.batches_done, nullptr));
      info.samples_done = h.samples_done;
    }
  }
  const int left = p.spp - (int)info.samples_done;
  if (left <= 0) throw std::runtime_error("the film is full: all SPP samples are in it");
  if (add > left) throw std::runtime_error("--add asks for more samples than the film has room for");
  const int todo = add > 0 ? add : left, base0 = (int)info.samples_done;
  float* dev = nullptr;
  if (hipMalloc(&dev, std::max<size_t>(n, 1) * sizeof(float)) != hipSuccess)
    throw std::runtime_error("device allocation failed");
  passes = std::max(1, passes);
  std::memset(total, 0, sizeof *total);
  if (noise.on) {  // the batches in index order, the summary after each from the second on
    if (todo % batch != 0 || base0 % batch != 0)
      throw std::runtime_error("--add and the film's samples must be multiples of the batch");
    spt_film_noise_info ni{};
    spt_noise_summary sm{};
    bool measured = false;
    for (int k = 0; k < todo / batch; ++k) {
      check(spt_film_render_async(ctx, film, scene.data(), (int32_t)scene.size(), &cam.abi(), &p,
                                  base0 + k * batch, batch, nullptr, nullptr));
      spt_stats st{};
      check(spt_context_stats(ctx, &st));
      total->samples += st.samples;
      total->vertices += st.vertices;
      total->kernel_ms += st.kernel_ms;
      check(spt_film_noise_info_get(film, &ni));
      measured = ni.batches_done >= (noise.adaptive ? std::max(2, noise.min_batches) : 2);
      if (!measured) continue;
      check(spt_film_noise_summary(film, &sm, nullptr));
      if (std::max(sm.rmse[0], std::max(sm.rmse[1], sm.rmse[2])) <= noise.target) break;
      if (noise.adaptive && k + 1 < todo / batch) {  // retire what is below the target, render the rest
        int64_t n_active = 0;
        if (noise.pool_radius)
          check(spt_film_adaptive_select_pooled(film, noise.target, noise.pool_radius,
                                                noise.pool_loo ? SPT_POOL_EXCLUDE_CENTER : 0u, nullptr,
                                                &n_active, nullptr));
        else
          check(spt_film_adaptive_select(film, noise.target, nullptr, &n_active, nullptr));
        if (n_active == 0) break;
      }
    }
    if (noise.adaptive) {
      spt_film_adaptive_info ai{};
      check(spt_film_adaptive_info_get(film, &ai));
      noise.samples_total = ai.samples_total;
    }
    check(spt_film_resolve(film, dev, nullptr));
    check(spt_film_info_get(film, &info));
    if (measured)
      std::cout << "NOISE : " << sm.rmse[0] << " " << sm.rmse[1] << " " << sm.rmse[2] << " after "
                << info.samples_done << " / " << info.spp_total << std::endl;
    passes = 0;
  }
  for (int k = 0; k < passes; ++k) {
    const int a = (int)((int64_t)todo * k / passes), b = (int)((int64_t)todo * (k + 1) / passes);
    if (b == a) continue;
    check(spt_film_render_async(ctx, film, scene.data(), (int32_t)scene.size(), &cam.abi(), &p,
                                base0 + a, b - a, b == todo ? dev : nullptr, nullptr));
    spt_stats st{};
    check(spt_context_stats(ctx, &st));
    total->samples += st.samples;
    total->vertices += st.vertices;
    total->kernel_ms += st.kernel_ms;
  }
  if (film_path) {
    check(spt_film_download(film, sums.data(), nullptr));
    check(spt_film_info_get(film, &info));
    FilmHeader h{};
    std::memcpy(h.magic, magic, 8);
    h.width = info.width; h.rows = info.rows; h.spp_total = info.spp_total;
    h.samples_done = info.samples_done;
    std::ofstream o(film_path, std::ios::binary | std::ios::trunc);
    o.write((const char*)&h, sizeof h);
    if (noise.on) {
      spt_film_noise_info ni{};
      check(spt_film_noise_info_get(film, &ni));
      check(spt_film_noise_download(film, m2.data(), nullptr));
      const NoiseHeader nh{ni.batch, 0, ni.batches_done};
      o.write((const char*)&nh, sizeof nh);
    }
    o.write((const char*)sums.data(), (std::streamsize)(n * sizeof(uint64_t)));
    if (noise.on) o.write((const char*)m2.data(), (std::streamsize)(2 * n * sizeof(uint64_t)));
    if (!o) throw std::runtime_error(std::string("cannot write ") + film_path);
    std::cout << "FILM : " << info.samples_done << " / " << info.spp_total << " samples" << std::endl;
  }
  if (denoise.on) {  // the image in dev becomes the filtered one; the film file above is the film's own
    spt_denoise_params dp;
    spt_denoise_default_params(&dp);
    if (denoise.iters_given) dp.iterations = denoise.iters;
    if (denoise.sigma_given) dp.sigma_color = (float)denoise.sigma;
    spt_guide* guide = nullptr;
    spt_denoiser* dn = nullptr;
    check(spt_guide_create_ex(p.device, &p, denoise.through_specular ? SPT_GUIDE_THROUGH_SPECULAR : 0u,
                              &guide));
    check(spt_denoiser_create(p.device, p.width, p.height, &dn));
    check(spt_guide_render_async(ctx, guide, scene.data(), (int32_t)scene.size(), &cam.abi(), &p, 0,
                                 std::min(p.spp, 64), nullptr));
    if (denoise.light_guide) {  // the planes one by one, the albedo shaded, spt_denoise_async
      const size_t n = 3ull * (size_t)p.width * (size_t)p.height;
      float* planes = shaded_guides(ctx, guide, scene, cam, p, denoise);
      float* tmp = nullptr;  // the film's image, then its error map
      if (hipMalloc(&tmp, std::max<size_t>(n, 1) * 2 * sizeof(float)) != hipSuccess)
        throw std::runtime_error("device allocation failed");
      check(spt_film_resolve(film, tmp, nullptr));
      check(spt_film_noise_map(film, tmp + n, nullptr));
      check(spt_denoise_async(dn, tmp, tmp + n, planes, planes + n, planes + 2 * n, &dp, dev, nullptr, nullptr));
      if (hipDeviceSynchronize() != hipSuccess) throw std::runtime_error("denoise failed on the device");
      (void)hipFree(tmp);
      (void)hipFree(planes);
    } else {
      check(spt_film_denoise(film, guide, dn, &dp, dev, nullptr, nullptr));
    }
    if (hipDeviceSynchronize() != hipSuccess) throw std::runtime_error("denoise failed on the device");
    check(spt_denoiser_destroy(dn));
    check(spt_guide_destroy(guide));
  }
  check(spt_film_destroy(film));
  check(spt_context_destroy(ctx));
  return dev;
}

// --bank-map: the mse plane and, behind it, the choice plane of the last bank call, from the device.
void write_bank_map(const std::string& prefix, const float* mse_dev, const spt_params& p) {
  const size_t npix = (size_t)p.width * (size_t)p.height;
  std::vector<float> mse(npix), mse3(3 * npix);
  std::vector<uint8_t> choice(npix);
  if (hipMemcpy(mse.data(), mse_dev, npix * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(choice.data(), mse_dev + npix, npix, hipMemcpyDeviceToHost) != hipSuccess)
    throw std::runtime_error("bank map download failed");
  for (size_t i = 0; i < npix; ++i) mse3[3 * i] = mse3[3 * i + 1] = mse3[3 * i + 2] = mse[i];
  const std::string mse_path = prefix + "_mse.pfm", choice_path = prefix + "_choice.pgm";
  if (write_ppm(mse_path.c_str(), p.width, p.height, mse3.data(), p.device, SPT_IMAGE_PFM))
    throw std::runtime_error("cannot write " + mse_path + ": " + spt_last_error());
  for (uint8_t& c : choice) c = (uint8_t)(c * 85);
  FILE* f = std::fopen(choice_path.c_str(), "wb");
  if (!f) throw std::runtime_error("cannot write " + choice_path);
  std::fprintf(f, "P5\n%d %d\n255\n", p.width, p.height);
  const bool ok = std::fwrite(choice.data(), 1, npix, f) == npix;
  if (std::fclose(f) != 0 || !ok) throw std::runtime_error("cannot write " + choice_path);
}

// --denoise --pair: the batches alternately into two noise films, the guide, the two-half filter. With
// noise.target > 0 the filter runs after every second batch from noise.min_batches on and the run ends
// once the largest channel's RMS half-difference is at most the target. Returns the DEVICE image.
float* render_pair(const std::vector<spt_prim>& scene, const Camera& cam, const spt_params& p,
                   const NoiseOpts& noise, const DenoiseOpts& denoise, spt_stats* total) {
  if (noise.batch <= 0 && p.spp % 8 != 0) throw std::runtime_error("--pair: SPP is no multiple of 8, give --batch");
  const int batch = noise.batch > 0 ? noise.batch : p.spp / 8;
  if (p.spp % batch != 0 || (p.spp / batch) % 2 != 0 || p.spp / batch < 4)
    throw std::runtime_error("--pair: the batch must divide SPP into an even number of batches, at least 4");
  spt_denoise_params dp;
  spt_denoise_default_params(&dp);
  if (denoise.iters_given) dp.iterations = denoise.iters;
  if (denoise.sigma_given) dp.sigma_color = (float)denoise.sigma;
  const uint32_t pair_flags = denoise.pair_own ? SPT_DENOISE_PAIR_OWN_WEIGHTS : 0u;
  const bool bank_on = !denoise.bank.empty();
  std::vector<spt_denoise_params> cands(denoise.bank.size(), dp);
  for (size_t k = 0; k < cands.size(); ++k) cands[k].sigma_color = denoise.bank[k];
  spt_bank_params bp;
  spt_denoise_bank_default_params(&bp);  // own weights
  bp.error_iterations = 3;  // render_denoised_bank's choice: the widest smoothing picks best
  spt_bank_summary bs{};
  spt_context* ctx = nullptr;
  spt_film* film[2] = {nullptr, nullptr};
  spt_guide* guide = nullptr;
  spt_denoiser* dn = nullptr;
  check(spt_context_create(p.device, &ctx));
  for (spt_film*& f : film) {
    check(spt_film_create(p.device, &p, &f));
    check(spt_film_noise_enable(f, batch));
  }
  check(spt_guide_create_ex(p.device, &p, denoise.through_specular ? SPT_GUIDE_THROUGH_SPECULAR : 0u, &guide));
  check(spt_denoiser_create(p.device, p.width, p.height, &dn));
  const size_t n = 3ull * (size_t)p.width * (size_t)p.height;
  float* dev = nullptr;  // out, then diff (the bank: mse, then choice)
  if (hipMalloc(&dev, std::max<size_t>(n, 1) * 2 * sizeof(float)) != hipSuccess)
    throw std::runtime_error("device allocation failed");
  std::memset(total, 0, sizeof *total);
  check(spt_guide_render_async(ctx, guide, scene.data(), (int32_t)scene.size(), &cam.abi(), &p, 0,
                               std::min(p.spp, 64), nullptr));
  float *planes = nullptr, *halves = nullptr;  // --light-guide: the shaded guide planes; rgb and se of A, of B
  if (denoise.light_guide) {
    planes = shaded_guides(ctx, guide, scene, cam, p, denoise);
    if (hipMalloc(&halves, std::max<size_t>(n, 1) * 4 * sizeof(float)) != hipSuccess)
      throw std::runtime_error("device allocation failed");
  }
  const int batches = p.spp / batch, need = std::max(4, noise.min_batches + (noise.min_batches & 1));
  spt_pair_summary sm{};
  int done = 0;
  for (int k = 0; k < batches; ++k) {
    check(spt_film_render_async(ctx, film[k & 1], scene.data(), (int32_t)scene.size(), &cam.abi(), &p,
                                k * batch, batch, nullptr, nullptr));
    spt_stats st{};
    check(spt_context_stats(ctx, &st));
    total->samples += st.samples;
    total->vertices += st.vertices;
    total->kernel_ms += st.kernel_ms;
    done = k + 1;
    const bool look = noise.target > 0.0 && done >= need && done % 2 == 0;
    if (!look && done < batches) continue;
    if (bank_on) {
      float* mse = dev + n;
      uint8_t* choice = (uint8_t*)(mse + n / 3);
      check(spt_film_pair_denoise_bank(film[0], film[1], guide, dn, cands.data(), (int32_t)cands.size(), &bp, dev,
                                       mse, choice, nullptr));
      check(spt_denoise_bank_summary(dn, mse, choice, &bs, nullptr));
      if (look && bs.rmse_est <= noise.target) break;
      continue;
    }
    if (denoise.light_guide) {
      for (int h = 0; h < 2; ++h) {
        check(spt_film_resolve(film[h], halves + 2 * h * n, nullptr));
        check(spt_film_noise_map(film[h], halves + (2 * h + 1) * n, nullptr));
      }
      check(spt_denoise_pair_async(dn, halves, halves + n, halves + 2 * n, halves + 3 * n, planes, planes + n,
                                   planes + 2 * n, &dp, pair_flags, dev, nullptr, dev + n, nullptr));
    } else {
      check(spt_film_pair_denoise(film[0], film[1], guide, dn, &dp, pair_flags, dev, nullptr, dev + n, nullptr));
    }
    check(spt_denoise_pair_summary(dn, dev + n, &sm, nullptr));
    if (look && std::max(sm.rmse[0], std::max(sm.rmse[1], sm.rmse[2])) <= noise.target) break;
  }
  if (bank_on) {
    std::cout << "BANK : " << bs.rmse_est;
    for (size_t k = 0; k < cands.size(); ++k) std::cout << " " << bs.share[k];
    std::cout << " after " << (int64_t)done * batch << " / " << p.spp << std::endl;
    if (denoise.bank_map) write_bank_map(denoise.bank_map, dev + n, p);
  } else {
    std::cout << "PAIR : " << sm.rmse[0] << " " << sm.rmse[1] << " " << sm.rmse[2] << " after "
              << (int64_t)done * batch << " / " << p.spp << std::endl;
  }
  if (halves) (void)hipFree(halves);
  if (planes) (void)hipFree(planes);
  check(spt_denoiser_destroy(dn));
  check(spt_guide_destroy(guide));
  for (spt_film* f : film) check(spt_film_destroy(f));
  check(spt_context_destroy(ctx));
  return dev;
}

// --guides: the guide planes of the full window, resolved on the device and written as three PFMs.
// light: also the light guide's visibility and direct planes of the same window, as two more PFMs.
void write_guides(const std::vector<spt_prim>& scene, const Camera& cam, const spt_params& p,
                  const std::string& prefix, bool through_specular, bool light) {
  spt_context* ctx = nullptr;
  spt_guide* guide = nullptr;
  check(spt_context_create(p.device, &ctx));
  check(spt_guide_create_ex(p.device, &p, through_specular ? SPT_GUIDE_THROUGH_SPECULAR : 0u, &guide));
  spt_guide_info info{};
  check(spt_guide_info_get(guide, &info));
  const size_t npix = (size_t)info.rows * (size_t)info.width;
  float* dev = nullptr;  // albedo, normal (3 floats each), depth (1)
  if (hipMalloc(&dev, std::max<size_t>(npix, 1) * 7 * sizeof(float)) != hipSuccess)
    throw std::runtime_error("device allocation failed");
  check(spt_guide_render_async(ctx, guide, scene.data(), (int32_t)scene.size(), &cam.abi(), &p, 0,
                               p.spp, nullptr));
  check(spt_guide_resolve(guide, dev, dev + 3 * npix, dev + 6 * npix, nullptr, nullptr));
  std::vector<float> host(7 * npix), depth3(3 * npix);
  if (hipMemcpy(host.data(), dev, host.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
    throw std::runtime_error("guide download failed");
  for (size_t i = 0; i < npix; ++i) depth3[3 * i] = depth3[3 * i + 1] = depth3[3 * i + 2] = host[6 * npix + i];
  const struct { const char* name; const float* data; } planes[3] = {
      {"_albedo.pfm", host.data()}, {"_normal.pfm", host.data() + 3 * npix}, {"_depth.pfm", depth3.data()}};
  for (const auto& pl : planes) {
    const std::string path = prefix + pl.name;
    if (write_ppm(path.c_str(), info.width, info.rows, pl.data, p.device, SPT_IMAGE_PFM))
      throw std::runtime_error("cannot write " + path + ": " + spt_last_error());
  }
  if (light) {
    spt_light_guide* lg = nullptr;
    check(spt_light_guide_create(p.device, &p, through_specular ? SPT_GUIDE_THROUGH_SPECULAR : 0u, &lg));
    check(spt_light_guide_render_async(ctx, lg, scene.data(), (int32_t)scene.size(), &cam.abi(), &p, 0, p.spp,
                                       nullptr));
    check(spt_light_guide_resolve(lg, dev, dev + npix, nullptr, nullptr));
    if (hipMemcpy(host.data(), dev, 2 * npix * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
      throw std::runtime_error("light guide download failed");
    const char* names[2] = {"_visibility.pfm", "_direct.pfm"};
    for (int k = 0; k < 2; ++k) {
      for (size_t i = 0; i < npix; ++i) depth3[3 * i] = depth3[3 * i + 1] = depth3[3 * i + 2] = host[k * npix + i];
      const std::string path = prefix + names[k];
      if (write_ppm(path.c_str(), info.width, info.rows, depth3.data(), p.device, SPT_IMAGE_PFM))
        throw std::runtime_error("cannot write " + path + ": " + spt_last_error());
    }
    check(spt_light_guide_destroy(lg));
  }
  (void)hipFree(dev);
  check(spt_guide_destroy(guide));
  check(spt_context_destroy(ctx));
}

// --frames N --orbit DEG: frame k's camera, LOOKFROM rotated about the vertical axis through the look-at
// point by k * DEG degrees.
Camera orbit_camera(int k, double degrees, float aspect) {
  const Vec at(50, 40, 5);
  if (k == 0) return Camera(LOOKFROM, at, Vec(0, 1, 0), 65, aspect);
  const double t = (k * degrees) * (M_PI / 180.0), c = std::cos(t), s = std::sin(t);
  const double dx = LOOKFROM.x - at.x, dz = LOOKFROM.z - at.z;
  const double cx = c * dx, sz = s * dz, sx = s * dx, cz = c * dz;
  return Camera(Vec((at.x + cx) + sz, LOOKFROM.y, (at.z - sx) + cz), at, Vec(0, 1, 0), 65, aspect);
}

struct OrbitOpts {
  int frames = 0;
  double degrees = 0.0;
  bool orbit_given = false, temporal = false, nmax_given = false;
  float nmax = 32.0f;
};

// The frames of an orbit, one file each: a noise film per frame (every sample, in batches), accumulated
// over its predecessors with --temporal, filtered with --denoise.
void render_orbit(const std::vector<spt_prim>& scene, spt_params p, const OrbitOpts& orbit, int batch,
                  const DenoiseOpts& denoise, const char* out, int format, spt_stats* total) {
  if (batch <= 0 && p.spp % 8 != 0) throw std::runtime_error("--frames: SPP is no multiple of 8, give --batch");
  if (batch <= 0) batch = p.spp / 8;
  if (p.spp % batch != 0 || p.spp / batch < 2)
    throw std::runtime_error("--frames: the batch must divide SPP into at least two batches");
  const size_t npix = (size_t)p.width * (size_t)p.height;
  const uint32_t seed0 = p.seed;
  spt_context* ctx = nullptr;
  spt_temporal* tp = nullptr;
  spt_denoiser* dn = nullptr;
  check(spt_context_create(p.device, &ctx));
  if (orbit.temporal) check(spt_temporal_create(p.device, p.width, p.height, &tp));
  if (denoise.on) check(spt_denoiser_create(p.device, p.width, p.height, &dn));
  spt_denoise_params dp;
  spt_denoise_default_params(&dp);
  if (denoise.iters_given) dp.iterations = denoise.iters;
  if (denoise.sigma_given) dp.sigma_color = (float)denoise.sigma;
  spt_temporal_params tpp;
  spt_temporal_default_params(&tpp);
  if (orbit.nmax_given) tpp.n_max = orbit.nmax;
  float* dev = nullptr;  // rgb, se, albedo, normal (3 floats a pixel each), depth (1), the filtered image (3)
  if (hipMalloc(&dev, std::max<size_t>(npix, 1) * 16 * sizeof(float)) != hipSuccess)
    throw std::runtime_error("device allocation failed");
  float *rgb = dev, *se = dev + 3 * npix, *albedo = dev + 6 * npix, *normal = dev + 9 * npix;
  float *depth = dev + 12 * npix, *filtered = dev + 13 * npix;
  std::string name(out);
  const size_t dot = name.find_last_of('.'), slash = name.find_last_of('/');
  const size_t cut = dot != std::string::npos && (slash == std::string::npos || dot > slash) ? dot : name.size();
  std::memset(total, 0, sizeof *total);
  for (int k = 0; k < orbit.frames; ++k) {
    const Camera cam = orbit_camera(k, orbit.degrees, float(p.width) / float(p.height));
    p.seed = seed0 + (uint32_t)k;
    spt_film* film = nullptr;
    spt_guide* guide = nullptr;
    check(spt_film_create(p.device, &p, &film));
    check(spt_film_noise_enable(film, batch));
    for (int b = 0; b < p.spp / batch; ++b) {
      check(spt_film_render_async(ctx, film, scene.data(), (int32_t)scene.size(), &cam.abi(), &p, b * batch, batch,
                                  nullptr, nullptr));
      spt_stats st{};
      check(spt_context_stats(ctx, &st));
      total->samples += st.samples;
      total->vertices += st.vertices;
      total->kernel_ms += st.kernel_ms;
    }
    const float* image = rgb;
    if (orbit.temporal || denoise.on) {
      check(spt_guide_create(p.device, &p, &guide));
      check(spt_guide_render_async(ctx, guide, scene.data(), (int32_t)scene.size(), &cam.abi(), &p, 0,
                                   std::min(p.spp, 64), nullptr));
    }
    if (orbit.temporal) {
      check(spt_film_temporal_accumulate(film, guide, tp, &cam.abi(), &tpp, rgb, se, nullptr, nullptr, albedo,
                                         normal, depth, nullptr));
      if (denoise.on) {
        check(spt_denoise_async(dn, rgb, se, albedo, normal, depth, &dp, filtered, nullptr, nullptr));
        image = filtered;
      }
    } else if (denoise.on) {
      check(spt_film_denoise(film, guide, dn, &dp, filtered, nullptr, nullptr));
      image = filtered;
    } else {
      check(spt_film_resolve(film, rgb, nullptr));
    }
    if (hipDeviceSynchronize() != hipSuccess) throw std::runtime_error("a frame failed on the device");
    char index[16];
    std::snprintf(index, sizeof index, ".%04d", k);
    const std::string path = name.substr(0, cut) + index + name.substr(cut);
    if (write_ppm(path.c_str(), p.width, p.height, image, p.device, format))
      throw std::runtime_error("cannot write " + path + ": " + spt_last_error());
    if (guide) check(spt_guide_destroy(guide));
    check(spt_film_destroy(film));
  }
  (void)hipFree(dev);
  if (dn) check(spt_denoiser_destroy(dn));
  if (tp) check(spt_temporal_destroy(tp));
  check(spt_context_destroy(ctx));
}

const char kUsage[] =
    "smallpt_amd [W H SPP [SEED [OUT.ppm]]] [--cos] [--uniform] [--reference-leaks] [--q Q]\n"
    "            [--specular | --classic | --mirror-glass | --spheres32 [--max-depth D]]\n"
    "            [--device N | --devices N] [--p6 | --pfm] [--repeat N] [--passes K]\n"
    "            [--film PATH [--add N]]\n"
    "            [--noise T [--batch B] [--adaptive [--min-batches M] [--pool R [--pool-loo]]]]\n"
    "            [--guides PREFIX] [--denoise [--denoise-iters N] [--denoise-sigma S]\n"
    "            [--pair [--pair-own] [--bank S,S,.. [--bank-map PREFIX]]]] [--through-specular]\n"
    "            [--light] [--light-guide [--shade-floor F]]\n"
    "            [--frames N --orbit DEG [--temporal [--temporal-nmax M]]]\n"
    "  --frames N --orbit DEG  N frames, the camera rotated about the vertical axis through the look-at\n"
    "                   point by DEG per frame, seed SEED + k, the frame index before OUT's extension\n"
    "                   (image.0000.ppm ...); goes with --denoise and --batch, one device\n"
    "  --temporal       with --frames: accumulate every frame over the frames before it, reprojected\n"
    "                   through the first-hit guide (the scene does not move), before it is written or filtered\n"
    "  --temporal-nmax M  with --temporal: the history's length at most, >= 1 (default 32)\n"
    "  --light          with --guides: also PREFIX_visibility.pfm and PREFIX_direct.pfm, the light guide's\n"
    "                   share of lit shadow rays and mean direct irradiance factor per pixel\n"
    "  --light-guide    with --denoise (also --pair; not --bank): shade the guide's albedo by a light\n"
    "                   guide's visibility, albedo * (F + (1 - F) * visibility), before it is filtered on\n"
    "  --shade-floor F  with --light-guide: the shade of a fully shadowed pixel, in (0, 1] (default 0.25)\n"
    "  --guides PREFIX  also write the first-hit guide planes PREFIX_albedo.pfm, PREFIX_normal.pfm\n"
    "                   and PREFIX_depth.pfm (linear PFM). The normal is stored signed, components\n"
    "                   in [-1, 1] (not 0.5 + 0.5 n); the depth is the mean ray parameter of the\n"
    "                   samples that hit, replicated to three channels. One device (no --devices).\n"
    "  --denoise        write the image denoised by the edge-stopping a-trous filter over the noise\n"
    "                   film's image, its error map and the guide planes (--noise/--batch as given,\n"
    "                   else 8 batches; goes with --adaptive; one device)\n"
    "  --through-specular  with --guides and/or --denoise: the guide follows mirrors and glass to\n"
    "                   the first diffuse surface (at most 8 segments)\n"
    "  --denoise-iters N  filter iterations, 0..6 (default 5)\n"
    "  --denoise-sigma S  the colour sigma (default 4)\n"
    "  --pair           with --denoise: two-half denoising. The batches go alternately into two films\n"
    "                   (SPP / batch even, at least 4), each half is filtered with colour weights\n"
    "                   from the other half, the output is the mean of the two results; prints PAIR,\n"
    "                   the RMS of half their difference. With --noise T the run stops on that figure.\n"
    "                   Not with --adaptive, --film or --passes.\n"
    "  --pair-own       with --pair: each half weighted by its own colours; the PAIR figure is then an\n"
    "                   unbiased estimate of the output's variance (with cross weights it reads low)\n"
    "  --bank S,S,..    with --pair: the filter bank, one candidate per colour sigma (1 to 4), own weights;\n"
    "                   per pixel the candidate of least cross-validated error, blended; prints BANK, the\n"
    "                   estimated RMSE (bias included) and each candidate's share of the pixels. With\n"
    "                   --noise T the run stops on that estimate. Not with --denoise-sigma.\n"
    "  --bank-map PREFIX  with --bank: also write PREFIX_mse.pfm and PREFIX_choice.pgm\n";

}  // namespace

int main(int argc, char* argv[]) {
  int pos[4] = {512, 512, 16, 1};  // :507-508 defaults, seed 1
  const char* out = "image.ppm";
  bool cosine = false, uniform = false, specular = false, classic = false, mirror_glass = false;
  bool spheres = false, ref_leaks = false;
  int device = 0, devices = 0, max_depth = 0, npos = 0, format = SPT_IMAGE_P3, repeat = 1;
  int passes = 0, add = 0;
  const char* film_path = nullptr;
  const char* guides = nullptr;
  bool shade_floor_given = false;
  bool light_planes = false;  // --light (with --guides): also PREFIX_visibility.pfm and PREFIX_direct.pfm
  NoiseOpts noise;
  DenoiseOpts denoise;
  OrbitOpts orbit;
  float q = -1.0f;
  for (int i = 1; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--cos")) cosine = true;
    else if (!std::strcmp(argv[i], "--uniform")) uniform = true;
    else if (!std::strcmp(argv[i], "--reference-leaks")) ref_leaks = true;
    else if (!std::strcmp(argv[i], "--specular")) specular = true;
    else if (!std::strcmp(argv[i], "--classic")) classic = true;
    else if (!std::strcmp(argv[i], "--mirror-glass")) mirror_glass = true;
    else if (!std::strcmp(argv[i], "--spheres32")) spheres = true;
    else if (!std::strcmp(argv[i], "--max-depth") && i + 1 < argc) max_depth = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--q") && i + 1 < argc) q = (float)std::atof(argv[++i]);
    else if (!std::strcmp(argv[i], "--device") && i + 1 < argc) device = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--devices") && i + 1 < argc) devices = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--repeat") && i + 1 < argc) repeat = std::max(1, std::atoi(argv[++i]));
    else if (!std::strcmp(argv[i], "--passes") && i + 1 < argc) passes = std::max(1, std::atoi(argv[++i]));
    else if (!std::strcmp(argv[i], "--film") && i + 1 < argc) film_path = argv[++i];
    else if (!std::strcmp(argv[i], "--add") && i + 1 < argc) add = std::max(1, std::atoi(argv[++i]));
    else if (!std::strcmp(argv[i], "--noise") && i + 1 < argc) { noise.on = true; noise.target = std::atof(argv[++i]); }
    else if (!std::strcmp(argv[i], "--batch") && i + 1 < argc) noise.batch = std::max(1, std::atoi(argv[++i]));
    else if (!std::strcmp(argv[i], "--adaptive")) noise.adaptive = true;
    else if (!std::strcmp(argv[i], "--min-batches") && i + 1 < argc) noise.min_batches = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--pool") && i + 1 < argc) noise.pool_radius = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--pool-loo")) noise.pool_loo = true;
    else if (!std::strcmp(argv[i], "--guides") && i + 1 < argc) guides = argv[++i];
    else if (!std::strcmp(argv[i], "--light")) light_planes = true;
    else if (!std::strcmp(argv[i], "--light-guide")) denoise.light_guide = true;
    else if (!std::strcmp(argv[i], "--shade-floor") && i + 1 < argc) { shade_floor_given = true; denoise.shade_floor = std::strtof(argv[++i], nullptr); }
    else if (!std::strcmp(argv[i], "--denoise")) denoise.on = true;
    else if (!std::strcmp(argv[i], "--through-specular")) denoise.through_specular = true;
    else if (!std::strcmp(argv[i], "--pair")) denoise.pair = true;
    else if (!std::strcmp(argv[i], "--pair-own")) denoise.pair_own = true;
    else if (!std::strcmp(argv[i], "--bank") && i + 1 < argc) {
      char* s = argv[++i];
      for (char* end = s; *s; s = *end == ',' ? end + 1 : end) {
        denoise.bank.push_back(std::strtof(s, &end));
        if (end == s || (*end && *end != ',')) { denoise.bank.assign(1, -1.0f); break; }
      }
      if (denoise.bank.empty()) denoise.bank.assign(1, -1.0f);
    }
    else if (!std::strcmp(argv[i], "--bank-map") && i + 1 < argc) denoise.bank_map = argv[++i];
    else if (!std::strcmp(argv[i], "--denoise-iters") && i + 1 < argc) { denoise.iters_given = true; denoise.iters = std::atoi(argv[++i]); }
    else if (!std::strcmp(argv[i], "--denoise-sigma") && i + 1 < argc) { denoise.sigma_given = true; denoise.sigma = std::atof(argv[++i]); }
    else if (!std::strcmp(argv[i], "--frames") && i + 1 < argc) orbit.frames = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--orbit") && i + 1 < argc) { orbit.orbit_given = true; orbit.degrees = std::atof(argv[++i]); }
    else if (!std::strcmp(argv[i], "--temporal")) orbit.temporal = true;
    else if (!std::strcmp(argv[i], "--temporal-nmax") && i + 1 < argc) { orbit.nmax_given = true; orbit.nmax = std::strtof(argv[++i], nullptr); }
    else if (!std::strcmp(argv[i], "--help")) { std::cout << kUsage; return 0; }
    else if (!std::strcmp(argv[i], "--p6")) format = SPT_IMAGE_P6;
    else if (!std::strcmp(argv[i], "--pfm")) format = SPT_IMAGE_PFM;
    else if (npos < 4) pos[npos++] = std::atoi(argv[i]);
    else out = argv[i];
  }
  if (denoise.through_specular && !guides && !denoise.on) {
    std::cerr << "--through-specular goes with --guides PREFIX or --denoise\n" << kUsage;
    return 2;
  }
  const auto t1 = std::chrono::high_resolution_clock::now();
  spt_params p;
  spt_default_params(&p);
  p.width = pos[0]; p.height = pos[1]; p.spp = pos[2]; p.seed = (uint32_t)pos[3];
  const bool box = classic || mirror_glass;
  p.nee_prob = q >= 0.0f ? q : (cosine || box ? 0.0f : 1.0f);  // :464 (the sphere box: emission only)
  p.max_depth = max_depth;
  if (uniform) p.flags |= SPT_FLAG_UNIFORM_SCATTER;
  if (ref_leaks) p.flags |= SPT_FLAG_REFERENCE_LEAKS;
  p.device = device;
  Camera cam(LOOKFROM, Vec(50, 40, 5), Vec(0, 1, 0), 65, float(p.width) / float(p.height));  // :521
  spt_stats st{};
  std::vector<float> c;
  const float* image = nullptr;  // what the writer reads: c's data, or the film's device image
  std::vector<spt_prim> guide_scene;
  try {
    if (guides && devices > 0) throw std::runtime_error("--guides goes with one device");
    const std::vector<spt_prim> scene = classic ? smallpt_classic_scene()
                                        : mirror_glass ? smallpt_mirror_glass_scene()
                                        : specular ? cornell_specular_scene()
                                        : spheres ? spheres32_scene()
                                                  : cornell_scene();
    if (guides) guide_scene = scene;
    if ((denoise.iters_given || denoise.sigma_given) && !denoise.on)
      throw std::runtime_error("--denoise-iters / --denoise-sigma go with --denoise");
    if ((denoise.pair || denoise.pair_own) && !denoise.on) throw std::runtime_error("--pair goes with --denoise");
    if (light_planes && !guides) throw std::runtime_error("--light goes with --guides PREFIX");
    if (denoise.light_guide && !denoise.on) throw std::runtime_error("--light-guide goes with --denoise");
    if (shade_floor_given && !denoise.light_guide) throw std::runtime_error("--shade-floor goes with --light-guide");
    if (denoise.light_guide && !denoise.bank.empty()) throw std::runtime_error("--light-guide does not go with --bank");
    if (!(denoise.shade_floor > 0.0f && denoise.shade_floor <= 1.0f))
      throw std::runtime_error("--shade-floor: a number in (0, 1]");
    if (denoise.pair_own && !denoise.pair) throw std::runtime_error("--pair-own goes with --pair");
    if (!denoise.bank.empty() && !denoise.pair) throw std::runtime_error("--bank goes with --denoise --pair");
    if (denoise.bank_map && denoise.bank.empty()) throw std::runtime_error("--bank-map goes with --bank");
    if (!denoise.bank.empty()) {
      if (denoise.sigma_given) throw std::runtime_error("--bank gives the colour sigmas: not with --denoise-sigma");
      if (denoise.bank.size() > SPT_BANK_MAX_CANDIDATES) throw std::runtime_error("--bank: 1 to 4 colour sigmas");
      for (float v : denoise.bank)
        if (!(v > 0.0f && std::isfinite(v))) throw std::runtime_error("--bank: a comma-separated list of positive, finite numbers");
    }
    if ((orbit.temporal || orbit.nmax_given || orbit.orbit_given) && orbit.frames == 0)
      throw std::runtime_error("--orbit / --temporal / --temporal-nmax go with --frames N");
    if (orbit.nmax_given && !orbit.temporal) throw std::runtime_error("--temporal-nmax goes with --temporal");
    if (orbit.frames != 0) {
      if (orbit.frames < 1 || orbit.frames > 9999) throw std::runtime_error("--frames: 1..9999");
      if (!orbit.orbit_given || !std::isfinite(orbit.degrees)) throw std::runtime_error("--frames goes with --orbit DEG");
      if (!(orbit.nmax >= 1.0f && std::isfinite(orbit.nmax))) throw std::runtime_error("--temporal-nmax: a finite number >= 1");
      if (devices > 0 || repeat > 1 || passes > 0 || film_path || noise.on || noise.adaptive || noise.pool_radius ||
          noise.pool_loo || guides || denoise.pair || denoise.through_specular || denoise.light_guide)
        throw std::runtime_error("--frames goes with one device and not with --noise, --film, --passes, --repeat, "
                                 "--guides, --pair, --adaptive, --through-specular or --light-guide");
      if (denoise.iters_given && (denoise.iters < 0 || denoise.iters > 6)) throw std::runtime_error("--denoise-iters: 0..6");
      if (denoise.sigma_given && !(denoise.sigma > 0.0 && std::isfinite((float)denoise.sigma)))
        throw std::runtime_error("--denoise-sigma: a positive, finite number");
      render_orbit(scene, p, orbit, noise.batch, denoise, out, format, &st);
      const auto t2 = std::chrono::high_resolution_clock::now();
      const double samples = (double)p.width * p.height * p.spp * orbit.frames;
      std::cout << "FRAMES : " << orbit.frames << "  KERNEL_MS : " << st.kernel_ms << "  MSAMPLES/S : "
                << samples / (st.kernel_ms * 1e3) << std::endl;
      std::cout << " DURATION : " << std::chrono::duration_cast<std::chrono::milliseconds>(t2 - t1).count()
                << std::endl;
      return 0;
    }
    if (denoise.on) {
      if (devices > 1) throw std::runtime_error("--denoise goes with one device: a shard's rows are not image neighbours");
      if (denoise.iters_given && (denoise.iters < 0 || denoise.iters > 6))
        throw std::runtime_error("--denoise-iters: 0..6");
      if (denoise.sigma_given && !(denoise.sigma > 0.0 && std::isfinite((float)denoise.sigma)))
        throw std::runtime_error("--denoise-sigma: a positive, finite number");
      if (!noise.on) { noise.on = true; noise.target = 0.0; }  // every sample, in batches
    }
    if (passes > 0 || film_path || noise.on || noise.adaptive || noise.pool_radius || noise.pool_loo) {
      if (devices > 0 || repeat > 1)
        throw std::runtime_error("--passes / --film / --noise go with one device and no --repeat");
      if (noise.adaptive && !noise.on) throw std::runtime_error("--adaptive goes with --noise T");
      if ((noise.pool_radius || noise.pool_loo) && !noise.adaptive)
        throw std::runtime_error("--pool goes with --noise T --adaptive");
      if (noise.pool_loo && !noise.pool_radius) throw std::runtime_error("--pool-loo goes with --pool R");
      if (noise.pool_radius < 0 || noise.pool_radius > SPT_POOL_MAX_RADIUS)
        throw std::runtime_error("--pool: the radius is 1..16");
      if (noise.adaptive && film_path)
        throw std::runtime_error("--adaptive does not go with --film: the counts plane has no file format");
      if (denoise.pair && (noise.adaptive || film_path || passes > 0))
        throw std::runtime_error("--pair does not go with --adaptive, --film or --passes");
      image = denoise.pair ? render_pair(scene, cam, p, noise, denoise, &st)
                           : render_film(scene, cam, p, passes, film_path, add, noise, denoise, &st);
      repeat = 0;
    }
    for (int k = 0; k < repeat; ++k) {
      const auto c0 = std::chrono::high_resolution_clock::now();
      if (devices > 0) {
        std::vector<int32_t> devs(devices);
        for (int j = 0; j < devices; ++j) devs[j] = j;
        c = render_multi(scene, cam, p, devs, &st);
      } else {
        c = render(scene, cam, p, &st);
      }
      const auto c1 = std::chrono::high_resolution_clock::now();
      if (repeat > 1)
        std::cout << "CALL " << k << " : WALL_MS " << std::chrono::duration<double, std::milli>(c1 - c0).count()
                  << "  KERNEL_MS " << st.kernel_ms << std::endl;
    }
  } catch (const std::exception& e) {
    std::cerr << "render failed: " << e.what() << std::endl;
    return 1;
  }
  if (!image) image = c.data();
  const auto w0 = std::chrono::high_resolution_clock::now();
  if (write_ppm(out, p.width, p.height, image, device, format)) {
    std::cerr << "cannot write " << out << ": " << spt_last_error() << std::endl;
    return 1;
  }
  if (guides) {  // after the image: its bytes are those of a run without the flag
    try {
      write_guides(guide_scene, cam, p, guides, denoise.through_specular, light_planes);
    } catch (const std::exception& e) {
      std::cerr << "guides failed: " << e.what() << std::endl;
      return 1;
    }
  }
  const auto t2 = std::chrono::high_resolution_clock::now();
  std::cout << "WRITE_MS : " << std::chrono::duration<double, std::milli>(t2 - w0).count() << std::endl;
  const double samples = (double)p.width * p.height * p.spp;
  std::cout << "KERNEL_MS : " << st.kernel_ms << "  MSAMPLES/S : " << samples / (st.kernel_ms * 1e3)
            << "  VERTICES/SAMPLE : " << (double)st.vertices / samples << std::endl;
  if (noise.samples_total >= 0) std::cout << "SAMPLES_TOTAL : " << noise.samples_total << std::endl;
  std::cout << " DURATION : " << std::chrono::duration_cast<std::chrono::milliseconds>(t2 - t1).count()
            << std::endl;  // :554-556
  return 0;
}

"""small-pathtracer_amd — MI355X-native drop-in for the smallpt per-pixel sampling loop.

Python mirror of the reference's host API over the C ABI in ``include/spt.h`` (libspt.so):

=====================================  ==================================================
reference (/root/reference/src/...)    here
=====================================  ==================================================
``Rectangle_xz/xy/yz`` smallpt.cpp:92-221  ``Rectangle_xz/xy/yz`` (same ctor argument order)
``Sphere`` :223-254                     ``Sphere``
``Refl_t {DIFF, SPEC, REFR}`` :72-74    ``DIFF, SPEC, REFR``
``Camera`` :256-285                     ``Camera`` (constructor semantics via spt_camera_init)
``Hitable *rect[]`` :287-311            ``cornell_scene()``
pixel loop :528-542 (+ radiance :419)   ``render()`` / ``Renderer`` (HIP kernel, gfx950)
``toInt`` :319-321 + PPM writer :548-551  ``write_ppm()`` / ``write_image()`` / ``Encoder``
                                        (GPU encoder: byte-identical P3, plus P6 and PFM)
=====================================  ==================================================

The product path is the HIP kernel only: ``render()`` and the writers raise if libspt.so or a
gfx950 device is missing — there is no CPU fallback in this package.
"""
from __future__ import annotations

import atexit
import ctypes
import math
import os
from contextlib import contextmanager as _contextmanager
from typing import Iterable, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SPT_LIB overrides the library (A/B builds in tools/ab.sh); the default is the in-tree build.
LIB_PATH = os.environ.get("SPT_LIB") or os.path.join(_HERE, "libspt.so")

DIFF, SPEC, REFR = 0, 1, 2
RECT_XY, RECT_XZ, RECT_YZ, SPHERE = 0, 1, 2, 3
LIGHT_GLIBC_WRAP, LIGHT_UNIFORM = 0, 1
PHILOX_KEY1 = 0x53505431

STATUS = {0: "ok", 1: "invalid argument", 2: "HIP runtime error", 3: "no usable gfx950 device",
          4: "device out of memory", 5: "unsupported feature", 6: "RCCL error"}


class SptError(RuntimeError):
    def __init__(self, status: int, msg: str = ""):
        super().__init__(f"spt error {status} ({STATUS.get(status, '?')}): {msg}")
        self.status = status


# ---------------------------------------------------------------------------------------------
# ctypes mirror of include/spt.h
# ---------------------------------------------------------------------------------------------
class spt_prim(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("refl", ctypes.c_int32),
                ("geom", ctypes.c_double * 5), ("e", ctypes.c_double * 3),
                ("c", ctypes.c_double * 3)]


class spt_camera(ctypes.Structure):
    _fields_ = [("origin", ctypes.c_double * 3), ("lower_left_corner", ctypes.c_double * 3),
                ("horizontal", ctypes.c_double * 3), ("vertical", ctypes.c_double * 3)]


class spt_params(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("spp", ctypes.c_int32),
                ("seed", ctypes.c_uint32), ("nee_prob", ctypes.c_float),
                ("rr_depth", ctypes.c_int32), ("max_depth", ctypes.c_int32),
                ("light_id", ctypes.c_int32),
                ("light_x0", ctypes.c_float), ("light_dx", ctypes.c_float),
                ("light_z0", ctypes.c_float), ("light_dz", ctypes.c_float),
                ("light_y", ctypes.c_float), ("light_area", ctypes.c_float),
                ("light_mode", ctypes.c_int32),
                ("tile_rows", ctypes.c_int32), ("shard_index", ctypes.c_int32),
                ("shard_count", ctypes.c_int32), ("chunk", ctypes.c_int32),
                ("device", ctypes.c_int32), ("flags", ctypes.c_uint32)]


class spt_stats(ctypes.Structure):
    _fields_ = [("samples", ctypes.c_uint64), ("path_rays", ctypes.c_uint64),
                ("shadow_rays", ctypes.c_uint64), ("vertices", ctypes.c_uint64),
                ("nee_events", ctypes.c_uint64), ("nee_light_hits", ctypes.c_uint64),
                ("cosine_samples", ctypes.c_uint64), ("misses", ctypes.c_uint64),
                ("shadow_traced", ctypes.c_uint64), ("sphere_vertices", ctypes.c_uint64),
                ("shadow_proven", ctypes.c_uint64), ("flop", ctypes.c_double), ("flop_executed", ctypes.c_double),
                ("kernel_ms", ctypes.c_double)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class spt_kernel_choice(ctypes.Structure):
    _fields_ = [("kernel", ctypes.c_int32), ("leak_end", ctypes.c_int32),
                ("early_resolve", ctypes.c_int32)]


class spt_film_info(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("rows", ctypes.c_int32), ("spp_total", ctypes.c_int32),
                ("samples_done", ctypes.c_int64)]


class spt_film_noise_info(ctypes.Structure):
    _fields_ = [("enabled", ctypes.c_int32), ("batch", ctypes.c_int32),
                ("batches_done", ctypes.c_int64)]


class spt_noise_summary(ctypes.Structure):
    _fields_ = [("rmse", ctypes.c_double * 3), ("rmse_all", ctypes.c_double),
                ("se_max", ctypes.c_float), ("clamped", ctypes.c_uint64),
                ("batches_done", ctypes.c_int64)]

    def as_dict(self) -> dict:
        return {"rmse": [float(x) for x in self.rmse], "rmse_all": float(self.rmse_all),
                "se_max": float(self.se_max), "clamped": int(self.clamped),
                "batches_done": int(self.batches_done)}


class spt_film_adaptive_info(ctypes.Structure):
    _fields_ = [("enabled", ctypes.c_int32), ("reserved", ctypes.c_int32), ("front", ctypes.c_int64),
                ("n_active", ctypes.c_int64), ("samples_total", ctypes.c_int64)]


class spt_guide_info(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("rows", ctypes.c_int32), ("spp_total", ctypes.c_int32),
                ("samples_done", ctypes.c_int64), ("lanes_per_pixel", ctypes.c_int32),
                ("flags", ctypes.c_uint32)]


class spt_denoise_params(ctypes.Structure):
    _fields_ = [("iterations", ctypes.c_int32), ("sigma_color", ctypes.c_float),
                ("sigma_depth", ctypes.c_float), ("sigma_albedo", ctypes.c_float),
                ("normal_squarings", ctypes.c_int32), ("albedo_floor", ctypes.c_float),
                ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class spt_pair_summary(ctypes.Structure):
    _fields_ = [("rmse", ctypes.c_double * 3), ("rmse_all", ctypes.c_double),
                ("diff_max", ctypes.c_float), ("reserved", ctypes.c_uint32)]

    def as_dict(self) -> dict:
        return {"rmse": [float(x) for x in self.rmse], "rmse_all": float(self.rmse_all),
                "diff_max": float(self.diff_max)}


class spt_bank_params(ctypes.Structure):
    _fields_ = [("error_iterations", ctypes.c_int32), ("pair_flags", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32 * 2)]


class spt_bank_summary(ctypes.Structure):
    _fields_ = [("mse_mean", ctypes.c_double), ("rmse_est", ctypes.c_double), ("share", ctypes.c_double * 4),
                ("mse_min", ctypes.c_float), ("mse_max", ctypes.c_float)]

    def as_dict(self) -> dict:
        return {"mse_mean": float(self.mse_mean), "rmse_est": float(self.rmse_est),
                "share": [float(x) for x in self.share], "mse_min": float(self.mse_min),
                "mse_max": float(self.mse_max)}


class spt_temporal_params(ctypes.Structure):
    _fields_ = [("n_max", ctypes.c_float), ("normal_min", ctypes.c_float), ("plane_tol", ctypes.c_float),
                ("albedo_floor", ctypes.c_float), ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class spt_temporal_state(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("c", "v", "n", "X", "N")]


class spt_temporal_info(ctypes.Structure):
    _fields_ = [("frames", ctypes.c_int64), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("has_history", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class spt_gather_op(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("peer", ctypes.c_int32), ("count", ctypes.c_uint64),
                ("offset", ctypes.c_uint64)]


GATHER_SEND, GATHER_RECV = 0, 1

STAT_KEYS = ["samples", "path_rays", "shadow_rays", "vertices", "nee_events", "nee_light_hits",
             "cosine_samples", "misses", "shadow_traced", "sphere_vertices"]

# Every entry point declared in include/spt.h (checked by tests/test_capi.py).
EXPORTS = ["spt_default_params", "spt_camera_init", "spt_scene_cornell", "spt_scene_spheres32",
           "spt_scene_cornell_specular", "spt_scene_smallpt_classic", "spt_scene_smallpt_mirror_glass",
           "spt_shard_rows", "spt_render", "spt_context_create", "spt_context_destroy",
           "spt_context_reserve", "spt_render_async", "spt_context_stats", "spt_abi_version",
           "spt_status_string", "spt_last_error", "spt_device_count", "spt_image_bound",
           "spt_encoder_create", "spt_encoder_destroy", "spt_encode_image", "spt_write_image",
           "spt_comm_unique_id", "spt_comm_create", "spt_comm_destroy", "spt_comm_reserve",
           "spt_gather_framebuffer", "spt_deinterleave_rows", "spt_render_multi", "spt_shutdown",
           "spt_gather_plan", "spt_gather_staging_floats", "spt_deinterleave_source",
           "spt_build_sources_sha16", "spt_kernel_count", "spt_kernel_name", "spt_select_kernel",
           "spt_context_kernel", "spt_film_create", "spt_film_destroy", "spt_film_info_get",
           "spt_film_clear", "spt_film_render_async", "spt_film_resolve", "spt_film_merge",
           "spt_film_download", "spt_film_upload", "spt_film_resolve_host",
           "spt_film_noise_enable", "spt_film_noise_info_get", "spt_film_noise_download",
           "spt_film_noise_upload", "spt_film_noise_map", "spt_film_noise_summary",
           "spt_film_noise_map_host", "spt_film_noise_summary_host",
           "spt_film_adaptive_enable", "spt_film_adaptive_info_get", "spt_film_adaptive_select",
           "spt_film_adaptive_download", "spt_film_adaptive_upload",
           "spt_film_adaptive_resolve_host", "spt_film_adaptive_noise_map_host",
           "spt_film_adaptive_noise_summary_host", "spt_film_adaptive_select_host",
           "spt_film_noise_pool_map", "spt_film_adaptive_select_pooled",
           "spt_film_noise_pool_map_host", "spt_film_adaptive_select_pooled_host",
           "spt_guide_info_size", "spt_guide_create", "spt_guide_create_ex", "spt_guide_destroy", "spt_guide_clear",
           "spt_guide_info_get", "spt_guide_render_async", "spt_guide_resolve", "spt_guide_download",
           "spt_guide_resolve_host",
           "spt_light_guide_create", "spt_light_guide_destroy", "spt_light_guide_clear",
           "spt_light_guide_info_get", "spt_light_guide_render_async", "spt_light_guide_resolve",
           "spt_light_guide_download", "spt_light_guide_resolve_host", "spt_light_shade_async",
           "spt_light_shade_host",
           "spt_denoise_default_params", "spt_denoiser_create", "spt_denoiser_destroy",
           "spt_denoise_async", "spt_denoise_host", "spt_film_denoise",
           "spt_denoise_pair_async", "spt_denoise_pair_host", "spt_denoise_pair_summary",
           "spt_denoise_pair_summary_host", "spt_film_pair_denoise",
           "spt_denoise_bank_default_params", "spt_denoise_bank_async", "spt_denoise_bank_host",
           "spt_denoise_bank_summary", "spt_denoise_bank_summary_host", "spt_film_pair_denoise_bank",
           "spt_temporal_default_params", "spt_temporal_create", "spt_temporal_destroy", "spt_temporal_reset",
           "spt_temporal_info_get", "spt_temporal_accumulate_async", "spt_temporal_accumulate_host",
           "spt_temporal_state_download", "spt_film_temporal_accumulate"]
SPT_HAS_TEMPORAL = 1        # include/spt.h: temporal accumulation (TemporalAccumulator, temporal_accumulate_host)
TEMPORAL_NO_DEMODULATE = 1  # SPT_TEMPORAL_NO_DEMODULATE: accumulate rgb itself, not rgb / albedo
TEMPORAL_STATE_PLANES = (("c", 3), ("v", 3), ("n", 1), ("X", 3), ("N", 3))  # spt_temporal_state, in order
SPT_HAS_DENOISE_BANK = 1    # include/spt.h: the filter bank (denoise_bank_host, Denoiser.denoise_bank, ...)
BANK_MAX_CANDIDATES = 4     # SPT_BANK_MAX_CANDIDATES
SPT_HAS_DENOISE_PAIR = 1    # include/spt.h: the two-half filter (denoise_pair_host, Denoiser.denoise_pair, ...)
DENOISE_PAIR_OWN_WEIGHTS = 1  # SPT_DENOISE_PAIR_OWN_WEIGHTS: each half weighted by its own colours
SPT_HAS_DENOISE = 1         # include/spt.h: the a-trous filter (Denoiser, denoise_host, render_denoised)
DENOISE_NO_DEMODULATE = 1   # SPT_DENOISE_NO_DEMODULATE: filter rgb itself, not rgb / albedo
SPT_HAS_GUIDE = 1           # include/spt.h: the spt_guide_* calls (Guide, render_guides)
GUIDE_SLOTS = 8             # a guide record: albedo 0-2, normal 3-5, depth 6 (48.16), hits 7
GUIDE_MAX_SPP = 1 << 24
SPT_HAS_GUIDE_CHAIN = 1     # include/spt.h: spt_guide_create_ex (Guide(..., through_specular=True))
GUIDE_THROUGH_SPECULAR = 1  # SPT_GUIDE_THROUGH_SPECULAR: the guide ray follows SPEC / REFR to a DIFF hit
GUIDE_MAX_CHAIN = 8         # SPT_GUIDE_MAX_CHAIN: segments of a chain at most
SPT_HAS_GUIDE_LIGHT = 1     # include/spt.h: the spt_light_guide_* calls (LightGuide, render_light_guides)
LIGHT_GUIDE_SLOTS = 4       # a light guide record: tested 0, lit 1, weight 2 (1.31 sums), reserved 3
COUNT_RETIRED = 0x80000000  # bit 31 of an adaptive film's counts: the pixel takes no more batches
COUNT_MASK = 0x7FFFFFFF     # ... and the batches it holds
POOL_MAX_RADIUS = 16        # SPT_POOL_MAX_RADIUS: the pooled calls take a radius in [1, 16]
POOL_EXCLUDE_CENTER = 1     # SPT_POOL_EXCLUDE_CENTER: a pixel's window without the pixel itself
IMAGE_FORMATS = {"p3": 0, "p6": 1, "pfm": 2}
FLAG_UNIFORM_SCATTER = 1  # spt_params.flags: random_scattering from the uniform code of :352-359
# spt_params.flags: leaked paths go on from the miss vertex as the reference's (:371-377) instead of
# ending at their first miss (contract v6's leak-end rule, the default where it applies)
FLAG_REFERENCE_LEAKS = 4
# spt_params.flags bits 8-9: cap on the kernel specialisation (A/B and tests; never changes results).
# "head"/"auto": the most specialised kernel the host can prove applicable.
KERNEL_LEVELS = {"auto": 0, "head": 0, "generic": 1, "cornell": 2, "const": 3}


def kernel_flag(name: str) -> int:
    """spt_params.flags bits selecting the kernel specialisation cap `name` (KERNEL_LEVELS)."""
    return KERNEL_LEVELS[name] << 8

_lib = None


def load_library(path: str = LIB_PATH) -> ctypes.CDLL:
    """Load libspt.so (built by __graft_entry__.build()). Fails loudly if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise SptError(2, f"{path} not built; run `python -c 'import __graft_entry__ as g; g.build()'`")
    # One HIP runtime per process: PyTorch ships its own libamdhip64.so.7 / libhsa-runtime64.so.1
    # (same SONAMEs as /opt/rocm's). Loading torch first makes libspt bind to torch's copy, so
    # device pointers and streams from torch are valid here; loading libspt first would pin the
    # system runtime and torch's later HIP init fails ("No HIP GPUs are available").
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(path)
    P, I32, U32 = ctypes.POINTER, ctypes.c_int32, ctypes.c_uint32
    lib.spt_default_params.argtypes = [P(spt_params)]
    lib.spt_camera_init.argtypes = [P(spt_camera), P(ctypes.c_double), P(ctypes.c_double),
                                    P(ctypes.c_double), ctypes.c_float, ctypes.c_float]
    lib.spt_scene_cornell.argtypes = [P(spt_prim), I32, P(I32)]
    lib.spt_scene_spheres32.argtypes = [P(spt_prim), I32, P(I32)]
    lib.spt_scene_cornell_specular.argtypes = [P(spt_prim), I32, P(I32)]
    lib.spt_scene_smallpt_classic.argtypes = [P(spt_prim), I32, P(I32)]
    lib.spt_scene_smallpt_mirror_glass.argtypes = [P(spt_prim), I32, P(I32)]
    lib.spt_shard_rows.argtypes = [P(spt_params), P(I32), I32]
    lib.spt_shard_rows.restype = I32
    lib.spt_render.argtypes = [P(spt_prim), I32, P(spt_camera), P(spt_params),
                               P(ctypes.c_float), P(spt_stats)]
    lib.spt_context_create.argtypes = [I32, P(ctypes.c_void_p)]
    lib.spt_context_destroy.argtypes = [ctypes.c_void_p]
    lib.spt_context_reserve.argtypes = [ctypes.c_void_p, I32, P(spt_params)]
    lib.spt_render_async.argtypes = [ctypes.c_void_p, P(spt_prim), I32, P(spt_camera),
                                     P(spt_params), ctypes.c_void_p, ctypes.c_void_p]
    lib.spt_context_stats.argtypes = [ctypes.c_void_p, P(spt_stats)]
    lib.spt_abi_version.restype = I32
    lib.spt_build_sources_sha16.restype = ctypes.c_char_p
    lib.spt_status_string.argtypes = [I32]
    lib.spt_status_string.restype = ctypes.c_char_p
    lib.spt_last_error.restype = ctypes.c_char_p
    lib.spt_device_count.restype = I32
    U64 = ctypes.c_uint64
    lib.spt_image_bound.argtypes = [I32, I32, I32]
    lib.spt_image_bound.restype = U64
    lib.spt_encoder_create.argtypes = [I32, P(ctypes.c_void_p)]
    lib.spt_encoder_destroy.argtypes = [ctypes.c_void_p]
    lib.spt_encode_image.argtypes = [ctypes.c_void_p, ctypes.c_void_p, I32, I32, I32,
                                     ctypes.c_void_p, U64, P(U64), ctypes.c_void_p]
    lib.spt_write_image.argtypes = [I32, ctypes.c_void_p, I32, I32, I32, ctypes.c_char_p]
    for name in ("spt_encoder_create", "spt_encoder_destroy", "spt_encode_image",
                 "spt_write_image"):
        getattr(lib, name).restype = I32
    VP = ctypes.c_void_p
    lib.spt_comm_unique_id.argtypes = [P(ctypes.c_uint8)]
    lib.spt_comm_create.argtypes = [P(ctypes.c_uint8), I32, I32, I32, P(VP)]
    lib.spt_comm_destroy.argtypes = [VP]
    lib.spt_comm_reserve.argtypes = [VP, P(spt_params)]
    lib.spt_gather_framebuffer.argtypes = [VP, P(spt_params), VP, VP, VP]
    lib.spt_deinterleave_rows.argtypes = [P(spt_params), I32, P(VP), VP, VP]
    lib.spt_render_multi.argtypes = [P(spt_prim), I32, P(spt_camera), P(spt_params), P(I32), I32,
                                     P(ctypes.c_float), P(spt_stats)]
    lib.spt_gather_plan.argtypes = [P(spt_params), I32, I32, P(spt_gather_op), I32]
    lib.spt_gather_plan.restype = I32
    lib.spt_gather_staging_floats.argtypes = [P(spt_params), I32]
    lib.spt_gather_staging_floats.restype = U64
    lib.spt_deinterleave_source.argtypes = [P(spt_params), I32, I32, P(I32), P(I32)]
    lib.spt_shutdown.argtypes = []
    lib.spt_kernel_count.argtypes = []
    lib.spt_kernel_count.restype = I32
    lib.spt_kernel_name.argtypes = [I32]
    lib.spt_kernel_name.restype = ctypes.c_char_p
    lib.spt_select_kernel.argtypes = [P(spt_prim), I32, P(spt_camera), P(spt_params),
                                      P(spt_kernel_choice)]
    lib.spt_select_kernel.restype = I32
    lib.spt_context_kernel.argtypes = [VP]
    lib.spt_context_kernel.restype = ctypes.c_char_p
    I64 = ctypes.c_int64
    lib.spt_film_create.argtypes = [I32, P(spt_params), P(VP)]
    lib.spt_film_destroy.argtypes = [VP]
    lib.spt_film_info_get.argtypes = [VP, P(spt_film_info)]
    lib.spt_film_clear.argtypes = [VP, VP]
    lib.spt_film_render_async.argtypes = [VP, VP, P(spt_prim), I32, P(spt_camera), P(spt_params),
                                          I32, I32, VP, VP]
    lib.spt_film_resolve.argtypes = [VP, VP, VP]
    lib.spt_film_merge.argtypes = [VP, VP, VP]
    lib.spt_film_download.argtypes = [VP, VP, VP]
    lib.spt_film_upload.argtypes = [VP, VP, I64, VP]
    lib.spt_film_resolve_host.argtypes = [VP, P(spt_film_info), VP]
    lib.spt_film_noise_enable.argtypes = [VP, I32]
    lib.spt_film_noise_info_get.argtypes = [VP, P(spt_film_noise_info)]
    lib.spt_film_noise_download.argtypes = [VP, VP, VP]
    lib.spt_film_noise_upload.argtypes = [VP, VP, I64, VP]
    lib.spt_film_noise_map.argtypes = [VP, VP, VP]
    lib.spt_film_noise_summary.argtypes = [VP, P(spt_noise_summary), VP]
    lib.spt_film_noise_map_host.argtypes = [VP, VP, P(spt_film_info), P(spt_film_noise_info), VP]
    lib.spt_film_noise_summary_host.argtypes = [VP, VP, P(spt_film_info), P(spt_film_noise_info),
                                                P(spt_noise_summary)]
    lib.spt_film_adaptive_enable.argtypes = [VP]
    lib.spt_film_adaptive_info_get.argtypes = [VP, P(spt_film_adaptive_info)]
    lib.spt_film_adaptive_select.argtypes = [VP, ctypes.c_double, VP, P(I64), VP]
    lib.spt_film_adaptive_download.argtypes = [VP, VP, VP]
    lib.spt_film_adaptive_upload.argtypes = [VP, VP, VP]
    lib.spt_film_adaptive_resolve_host.argtypes = [VP, VP, P(spt_film_info), P(spt_film_noise_info), VP]
    lib.spt_film_adaptive_noise_map_host.argtypes = [VP, VP, VP, P(spt_film_info),
                                                     P(spt_film_noise_info), VP]
    lib.spt_film_adaptive_noise_summary_host.argtypes = [VP, VP, VP, P(spt_film_info),
                                                         P(spt_film_noise_info), P(spt_noise_summary)]
    lib.spt_film_adaptive_select_host.argtypes = [VP, VP, VP, P(spt_film_info), P(spt_film_noise_info),
                                                  ctypes.c_double, VP, VP, VP, P(I64)]
    lib.spt_film_noise_pool_map.argtypes = [VP, I32, U32, VP, VP]
    lib.spt_film_adaptive_select_pooled.argtypes = [VP, ctypes.c_double, I32, U32, VP, P(I64), VP]
    lib.spt_film_noise_pool_map_host.argtypes = [VP, VP, VP, P(spt_film_info), P(spt_film_noise_info),
                                                 I32, I32, U32, VP]
    lib.spt_film_adaptive_select_pooled_host.argtypes = [VP, VP, VP, P(spt_film_info),
                                                         P(spt_film_noise_info), I32, ctypes.c_double,
                                                         I32, U32, VP, VP, VP, P(I64)]
    lib.spt_guide_info_size.argtypes = []
    lib.spt_guide_create.argtypes = [I32, P(spt_params), P(VP)]
    lib.spt_guide_create_ex.argtypes = [I32, P(spt_params), ctypes.c_uint32, P(VP)]
    lib.spt_guide_destroy.argtypes = [VP]
    lib.spt_guide_clear.argtypes = [VP, VP]
    lib.spt_guide_info_get.argtypes = [VP, P(spt_guide_info)]
    lib.spt_guide_render_async.argtypes = [VP, VP, P(spt_prim), I32, P(spt_camera), P(spt_params),
                                           I32, I32, VP]
    lib.spt_guide_resolve.argtypes = [VP, VP, VP, VP, VP, VP]
    lib.spt_guide_download.argtypes = [VP, VP, VP]
    lib.spt_guide_resolve_host.argtypes = [VP, P(spt_guide_info), VP, VP, VP, VP]
    lib.spt_light_guide_create.argtypes = [I32, P(spt_params), ctypes.c_uint32, P(VP)]
    lib.spt_light_guide_destroy.argtypes = [VP]
    lib.spt_light_guide_clear.argtypes = [VP, VP]
    lib.spt_light_guide_info_get.argtypes = [VP, P(spt_guide_info)]
    lib.spt_light_guide_render_async.argtypes = [VP, VP, P(spt_prim), I32, P(spt_camera), P(spt_params),
                                                 I32, I32, VP]
    lib.spt_light_guide_resolve.argtypes = [VP, VP, VP, VP, VP]
    lib.spt_light_guide_download.argtypes = [VP, VP, VP]
    lib.spt_light_guide_resolve_host.argtypes = [VP, P(spt_guide_info), VP, VP, VP]
    lib.spt_light_shade_async.argtypes = [VP, VP, I64, ctypes.c_float, VP, VP]
    lib.spt_light_shade_host.argtypes = [VP, VP, I64, ctypes.c_float, VP]
    lib.spt_denoise_default_params.argtypes = [P(spt_denoise_params)]
    lib.spt_denoise_default_params.restype = None
    lib.spt_denoiser_create.argtypes = [I32, I32, I32, P(VP)]
    lib.spt_denoiser_destroy.argtypes = [VP]
    lib.spt_denoise_async.argtypes = [VP, VP, VP, VP, VP, VP, P(spt_denoise_params), VP, VP, VP]
    lib.spt_denoise_host.argtypes = [VP, VP, VP, VP, VP, I32, I32, P(spt_denoise_params), VP, VP]
    lib.spt_film_denoise.argtypes = [VP, VP, VP, P(spt_denoise_params), VP, VP, VP]
    lib.spt_denoise_pair_async.argtypes = [VP] + [VP] * 7 + [P(spt_denoise_params), ctypes.c_uint32, VP, VP,
                                                             VP, VP]
    lib.spt_denoise_pair_host.argtypes = [VP] * 7 + [I32, I32, P(spt_denoise_params), ctypes.c_uint32, VP,
                                                     VP, VP]
    lib.spt_denoise_pair_summary.argtypes = [VP, VP, P(spt_pair_summary), VP]
    lib.spt_denoise_pair_summary_host.argtypes = [VP, I32, I32, P(spt_pair_summary)]
    lib.spt_film_pair_denoise.argtypes = [VP, VP, VP, VP, P(spt_denoise_params), ctypes.c_uint32, VP, VP,
                                          VP, VP]
    lib.spt_denoise_bank_default_params.argtypes = [P(spt_bank_params)]
    lib.spt_denoise_bank_default_params.restype = None
    lib.spt_denoise_bank_async.argtypes = [VP] + [VP] * 7 + [P(spt_denoise_params), I32, P(spt_bank_params), VP,
                                                             VP, VP, VP]
    lib.spt_denoise_bank_host.argtypes = [VP] * 7 + [I32, I32, P(spt_denoise_params), I32, P(spt_bank_params),
                                                     VP, VP, VP]
    lib.spt_denoise_bank_summary.argtypes = [VP, VP, VP, P(spt_bank_summary), VP]
    lib.spt_denoise_bank_summary_host.argtypes = [VP, VP, I32, I32, P(spt_bank_summary)]
    lib.spt_film_pair_denoise_bank.argtypes = [VP, VP, VP, VP, P(spt_denoise_params), I32, P(spt_bank_params),
                                               VP, VP, VP, VP]
    lib.spt_temporal_default_params.argtypes = [P(spt_temporal_params)]
    lib.spt_temporal_default_params.restype = None
    lib.spt_temporal_create.argtypes = [I32, I32, I32, P(VP)]
    lib.spt_temporal_destroy.argtypes = [VP]
    lib.spt_temporal_reset.argtypes = [VP]
    lib.spt_temporal_info_get.argtypes = [VP, P(spt_temporal_info)]
    lib.spt_temporal_accumulate_async.argtypes = [VP] + [VP] * 5 + [P(spt_camera), P(spt_temporal_params), VP, VP,
                                                                    VP, VP, VP]
    lib.spt_temporal_accumulate_host.argtypes = [VP] * 5 + [I32, I32, P(spt_camera), P(spt_temporal_params),
                                                            P(spt_temporal_state), P(spt_camera), VP, VP, VP, VP,
                                                            P(spt_temporal_state)]
    lib.spt_temporal_state_download.argtypes = [VP, P(spt_temporal_state), P(spt_camera), VP]
    lib.spt_film_temporal_accumulate.argtypes = [VP, VP, VP, P(spt_camera), P(spt_temporal_params)] + [VP] * 8
    for name in ("spt_temporal_create", "spt_temporal_destroy", "spt_temporal_reset", "spt_temporal_info_get",
                 "spt_temporal_accumulate_async", "spt_temporal_accumulate_host", "spt_temporal_state_download"):
        getattr(lib, name).restype = I32
    for name in ("spt_denoiser_create", "spt_denoiser_destroy", "spt_denoise_async", "spt_denoise_host",
                 "spt_denoise_pair_async", "spt_denoise_pair_host", "spt_denoise_pair_summary",
                 "spt_denoise_pair_summary_host", "spt_denoise_bank_async", "spt_denoise_bank_host",
                 "spt_denoise_bank_summary", "spt_denoise_bank_summary_host"):
        getattr(lib, name).restype = I32
    for name in EXPORTS:
        if name.startswith(("spt_film_", "spt_guide_", "spt_light_")):
            getattr(lib, name).restype = I32
    for name in ("spt_comm_unique_id", "spt_comm_create", "spt_comm_destroy", "spt_comm_reserve",
                 "spt_gather_framebuffer", "spt_deinterleave_rows", "spt_render_multi",
                 "spt_deinterleave_source", "spt_shutdown"):
        getattr(lib, name).restype = I32
    for name in ("spt_default_params", "spt_camera_init", "spt_scene_cornell",
                 "spt_scene_spheres32", "spt_scene_cornell_specular", "spt_scene_smallpt_classic",
                 "spt_scene_smallpt_mirror_glass",
                 "spt_render", "spt_context_create",
                 "spt_context_destroy", "spt_context_reserve", "spt_render_async",
                 "spt_context_stats"):
        getattr(lib, name).restype = I32
    del U32
    _lib = lib
    # spt_render's cached per-device contexts (unit slots: ~200-400 MB) are returned when the
    # interpreter exits, not held until the process dies (a no-op when spt_render never ran)
    atexit.register(_release_dropin_contexts)
    return lib


# The sources the render kernel is compiled from: their hash identifies a kernel build, so a PMC
# profile committed under profiles/ can say which kernel it measured (bench.py omits hardware-counter
# figures whose profile was taken on other sources).
KERNEL_SOURCES = ("csrc/spt_kernel.hip", "csrc/spt_trace.h", "csrc/spt_variants.h", "csrc/spt_kparams.h",
                  "csrc/spt_launch.h", "csrc/spt_dispatch.cpp", "csrc/spt_context.cpp",
                  "csrc/spt_device.h", "csrc/spt_cornell.h", "csrc/spt_diag.h", "csrc/Makefile", "../include/spt.h", "../include/spt_flops.h", "csrc/spt_film.hip",
                  "csrc/spt_film.h", "csrc/spt_film_math.h", "csrc/spt_film_host.cpp",
                  "csrc/spt_guide.hip", "csrc/spt_guide_host.cpp", "csrc/spt_guide.h",
                  "csrc/spt_denoise.hip", "csrc/spt_denoise_host.cpp", "csrc/spt_denoise.h",
                  "csrc/spt_status.h", "csrc/spt_window_shape.h", "csrc/spt_guide_device.h",
                  "csrc/spt_guide_light.hip", "csrc/spt_guide_light_host.cpp", "csrc/spt_guide_light.h",
                  "csrc/spt_temporal.hip", "csrc/spt_temporal_host.cpp", "csrc/spt_temporal.h")


def kernel_sources_sha16() -> str:
    import hashlib

    h = hashlib.sha256()
    for rel in KERNEL_SOURCES:
        with open(os.path.join(_HERE, rel), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def build_sources_sha16() -> str:
    """kernel_sources_sha16() of the sources the loaded libspt.so was built from (embedded by make)."""
    return load_library().spt_build_sources_sha16().decode()


def _release_dropin_contexts() -> None:
    if _lib is not None:
        try:
            _lib.spt_shutdown()
        except Exception:  # noqa: BLE001 -- interpreter shutdown: nothing left to report to
            pass


def _check(status: int) -> None:
    if status != 0:
        msg = (load_library().spt_last_error() or b"").decode(errors="replace")
        raise SptError(status, msg)


# ---------------------------------------------------------------------------------------------
# Reference-shaped host API
# ---------------------------------------------------------------------------------------------
def _v3(v) -> tuple:
    if isinstance(v, (int, float)):
        return (float(v), 0.0, 0.0)
    t = tuple(float(x) for x in v)
    return t + (0.0,) * (3 - len(t))


class Vec(tuple):
    """Vec :24-62 (only what scene construction needs: Vec(x=0, y=0, z=0), * scalar)."""

    def __new__(cls, x=0.0, y=0.0, z=0.0):
        return super().__new__(cls, (float(x), float(y), float(z)))

    def __mul__(self, b):
        return Vec(self[0] * b, self[1] * b, self[2] * b)

    __rmul__ = __mul__


def _prim(kind, geom, e, c, refl) -> spt_prim:
    p = spt_prim()
    p.kind, p.refl = kind, int(refl)
    for i, g in enumerate(geom):
        p.geom[i] = float(g)
    for i, x in enumerate(_v3(e)):
        p.e[i] = x
    for i, x in enumerate(_v3(c)):
        p.c[i] = x
    return p


def Rectangle_xz(x1, x2, z1, z2, y, e, c, refl=DIFF) -> spt_prim:  # :97-98
    return _prim(RECT_XZ, (x1, x2, z1, z2, y), e, c, refl)


def Rectangle_xy(x1, x2, y1, y2, z, e, c, refl=DIFF) -> spt_prim:  # :142
    return _prim(RECT_XY, (x1, x2, y1, y2, z), e, c, refl)


def Rectangle_yz(y1, y2, z1, z2, x, e, c, refl=DIFF) -> spt_prim:  # :185
    return _prim(RECT_YZ, (y1, y2, z1, z2, x), e, c, refl)


def Sphere(rad, p, e, c, refl=DIFF) -> spt_prim:  # :228
    pp = _v3(p)
    return _prim(SPHERE, (rad, pp[0], pp[1], pp[2], 0.0), e, c, refl)


LOOKFROM = Vec(50, 40, 168)  # :65


class Camera:
    """Camera :256-285: Camera(lookfrom, lookat, vup, vfov, aspect); get_ray(s, t)."""

    def __init__(self, lookfrom=LOOKFROM, lookat=(50, 40, 5), vup=(0, 1, 0), vfov=65.0,
                 aspect=1.0):
        lib = load_library()
        self._c = spt_camera()
        arr = lambda v: (ctypes.c_double * 3)(*_v3(v))  # noqa: E731
        _check(lib.spt_camera_init(ctypes.byref(self._c), arr(lookfrom), arr(lookat), arr(vup),
                                   float(vfov), float(aspect)))

    @property
    def origin(self):
        return tuple(self._c.origin)

    @property
    def lower_left_corner(self):
        return tuple(self._c.lower_left_corner)

    @property
    def horizontal(self):
        return tuple(self._c.horizontal)

    @property
    def vertical(self):
        return tuple(self._c.vertical)

    def get_ray(self, s: float, t: float):  # :276-279
        o, l, h, v = self.origin, self.lower_left_corner, self.horizontal, self.vertical
        return o, tuple(l[i] + h[i] * s + v[i] * t - o[i] for i in range(3))


def cornell_scene() -> list:
    """rect[] of :287-311 via the library's builder (17 primitives)."""
    lib = load_library()
    arr = (spt_prim * 64)()
    n = ctypes.c_int32()
    _check(lib.spt_scene_cornell(arr, 64, ctypes.byref(n)))
    return [arr[i] for i in range(n.value)]


def smallpt_classic_scene() -> list:
    """spt_scene_smallpt_classic(): the classic smallpt sphere box of the reference's older revision
    and its shipped image*.ppm (walls of radius 1e5, fp64-tested; two matte white balls; the
    radius-600 light sphere, prim 8). Render with nee_prob = 0 (no light rectangle)."""
    lib = load_library()
    arr = (spt_prim * 16)()
    n = ctypes.c_int32()
    _check(lib.spt_scene_smallpt_classic(arr, 16, ctypes.byref(n)))
    return [arr[i] for i in range(n.value)]


def smallpt_mirror_glass_scene() -> list:
    """spt_scene_smallpt_mirror_glass(): the same box with smallpt's mirror (SPEC) and glass (REFR)
    balls."""
    lib = load_library()
    arr = (spt_prim * 16)()
    n = ctypes.c_int32()
    _check(lib.spt_scene_smallpt_mirror_glass(arr, 16, ctypes.byref(n)))
    return [arr[i] for i in range(n.value)]


def spheres32_scene() -> list:
    lib = load_library()
    arr = (spt_prim * 64)()
    n = ctypes.c_int32()
    _check(lib.spt_scene_spheres32(arr, 64, ctypes.byref(n)))
    return [arr[i] for i in range(n.value)]


def move_short_box(prims: list, dx: float) -> list:
    """rect[] of :287-311 with the short box (:305-309, prims 12-16) moved by dx along x: the HEAD
    topology with edited geometry (the uploaded-geometry kernels; the compile-time one matches only
    the unedited table)."""
    out = [spt_prim.from_buffer_copy(p) for p in prims]
    for i in (12, 13, 16):  # XY faces and the XZ top: x bounds geom[0:2]
        out[i].geom[0] += dx
        out[i].geom[1] += dx
    for i in (14, 15):  # YZ faces: plane x = geom[4]
        out[i].geom[4] += dx
    return out


def edit_light(prims: list, x=(32.0, 68.0), z=(63.0, 96.0), y=81.5, e=None) -> list:
    """rect[] of :287-311 with the light (:294, prim 6) moved or resized: Rectangle_xz(x0, x1, z0,
    z1, y) and optionally its emission e. The room and the boxes stay (the boxes-only-uploaded
    kernels take the light from LDS; the early shadow-ray resolve needs the light's plane at most
    81.5 and its rectangle >= 1 inside the walls)."""
    out = [spt_prim.from_buffer_copy(p) for p in prims]
    g = out[6].geom
    g[0], g[1], g[2], g[3], g[4] = float(x[0]), float(x[1]), float(z[0]), float(z[1]), float(y)
    if e is not None:
        for i, v in enumerate(_v3(e)):
            out[6].e[i] = v
    return out


def edit_room(prims: list, depth: float = 170.0, width=(1.0, 99.0), height: float = 81.6) -> list:
    """rect[] of :287-311 with the room (:288-293, prims 0-5) resized: back wall at z = depth, side
    walls at x = width, ceiling at y = height, every wall's extents to match (a closed room, the
    HEAD topology)."""
    out = [spt_prim.from_buffer_copy(p) for p in prims]
    x0, x1 = float(width[0]), float(width[1])
    for i in (0, 1):  # Front / Back: Rectangle_xy(x0, x1, 0, height, z)
        g = out[i].geom
        g[0], g[1], g[3] = x0, x1, float(height)
    out[1].geom[4] = float(depth)
    for i, xw in ((2, x0), (3, x1)):  # Left / Right: Rectangle_yz(0, height, 0, depth, x)
        g = out[i].geom
        g[1], g[3], g[4] = float(height), float(depth), xw
    for i in (4, 5):  # Bottom / Top: Rectangle_xz(x0, x1, 0, depth, y)
        g = out[i].geom
        g[0], g[1], g[3] = x0, x1, float(depth)
    out[5].geom[4] = float(height)
    return out


def drop_short_box(prims: list) -> list:
    """rect[] of :287-311 without the short box (:305-309, prims 12-16): another topology (the
    uploaded-geometry rect-only kernels)."""
    return [spt_prim.from_buffer_copy(p) for p in prims[:12]]


def cornell_specular_scene() -> list:
    """Room + light of :288-294 with smallpt's mirror (SPEC) and glass (REFR) balls (:296-297)."""
    lib = load_library()
    arr = (spt_prim * 16)()
    n = ctypes.c_int32()
    _check(lib.spt_scene_cornell_specular(arr, 16, ctypes.byref(n)))
    return [arr[i] for i in range(n.value)]


def default_params(**kw) -> spt_params:
    p = spt_params()
    _check(load_library().spt_default_params(ctypes.byref(p)))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError(f"unknown spt_params field {k!r}")
        setattr(p, k, v)
    return p


def shard_rows(params: spt_params) -> np.ndarray:
    lib = load_library()
    n = lib.spt_shard_rows(ctypes.byref(params), None, 0)
    rows = (ctypes.c_int32 * max(n, 1))()
    lib.spt_shard_rows(ctypes.byref(params), rows, n)
    return np.frombuffer(rows, dtype=np.int32, count=n).copy()


def _scene_array(prims: Sequence[spt_prim]):
    arr = (spt_prim * len(prims))()
    for i, p in enumerate(prims):
        arr[i] = p
    return arr


def kernel_names() -> list:
    """The render kernel's variants by id (spt_kernel_count / spt_kernel_name)."""
    lib = load_library()
    return [lib.spt_kernel_name(i).decode() for i in range(lib.spt_kernel_count())]


def select_kernel(prims: Sequence[spt_prim], cam: Camera, params: spt_params) -> dict:
    """spt_select_kernel(): the kernel variant a render of these arguments launches -- {"id", "name",
    "leak_end", "early_resolve"}. A pure host function (no device)."""
    lib = load_library()
    ch = spt_kernel_choice()
    _check(lib.spt_select_kernel(_scene_array(prims), len(prims), ctypes.byref(cam._c),
                                 ctypes.byref(params), ctypes.byref(ch)))
    return {"id": int(ch.kernel), "name": lib.spt_kernel_name(ch.kernel).decode(),
            "leak_end": int(ch.leak_end), "early_resolve": bool(ch.early_resolve)}


def _kernel_of(ctx) -> str | None:
    name = load_library().spt_context_kernel(ctx)
    return name.decode() if name is not None else None


def render(prims: Sequence[spt_prim], cam: Camera, params: spt_params, return_stats=False):
    """Drop-in for :528-542: returns (rows, w, 3) float32 linear clamped RGB (rows = this shard's
    rows, the whole image when shard_count == 1), y=0 top row. Runs on the GPU only.
    return_stats: also the spt_stats as a dict, plus "kernel": the name of the variant that ran
    (None for a shard without rows)."""
    lib = load_library()
    rows = int(lib.spt_shard_rows(ctypes.byref(params), None, 0))
    out = np.empty((rows, params.width, 3), dtype=np.float32)
    st = spt_stats()
    _check(lib.spt_render(_scene_array(prims), len(prims), ctypes.byref(cam._c),
                          ctypes.byref(params),
                          out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ctypes.byref(st)))
    if not return_stats:
        return out
    d = st.as_dict()
    d["kernel"] = _kernel_of(None)
    return out, d


class Renderer:
    """Persistent device context for repeated renders into device buffers (torch tensors or raw
    pointers) on a given HIP stream — what bench.py and the multi-GPU path use."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        self._ctx = ctypes.c_void_p()
        _check(self.lib.spt_context_create(int(device), ctypes.byref(self._ctx)))
        self.device = device

    def close(self):
        if self._ctx:
            self.lib.spt_context_destroy(self._ctx)
            self._ctx = None

    def __del__(self):  # at interpreter exit module globals (ctypes) may already be gone
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def reserve(self, n_prims: int, params: spt_params):
        _check(self.lib.spt_context_reserve(self._ctx, int(n_prims), ctypes.byref(params)))

    def render_async(self, prims, cam: Camera, params: spt_params, rgb_dev_ptr: int,
                     stream_ptr: int = 0):
        self._prims = _scene_array(prims)
        _check(self.lib.spt_render_async(self._ctx, self._prims, len(prims), ctypes.byref(cam._c),
                                         ctypes.byref(params), ctypes.c_void_p(rgb_dev_ptr),
                                         ctypes.c_void_p(stream_ptr)))

    def stats(self) -> dict:
        st = spt_stats()
        _check(self.lib.spt_context_stats(self._ctx, ctypes.byref(st)))
        return st.as_dict()

    def kernel(self) -> str | None:
        """spt_context_kernel(): the variant of the last launch (None before any, and for a shard
        without rows)."""
        return _kernel_of(self._ctx)


# ---------------------------------------------------------------------------------------------
# Progressive rendering: sample windows into a resumable integer film (spt_film_*)
# ---------------------------------------------------------------------------------------------
FILM_MAGIC = b"SPTFILM1"
_FILM_HEADER = "<8siiiiq"  # magic, width, rows, spp_total, 0, samples_done: 32 bytes, then the sums
# a noise film's file: the same 32 bytes under its own magic, then batch, 0, batches_done (48 bytes),
# the sums, and the moment plane M2 (rows * width * 3 pairs (lo, hi) of uint64)
FILM_MAGIC_NOISE = b"SPTFILM2"
_FILM_HEADER_NOISE = "<8siiiiqiiq"


def sample_windows(spp: int, passes: int) -> list:
    """[0, spp) cut into `passes` near-equal windows [(base, count), ...] (empty ones dropped)."""
    if passes < 1:
        raise ValueError("passes must be >= 1")
    edges = [spp * i // passes for i in range(passes + 1)]
    return [(a, b - a) for a, b in zip(edges, edges[1:]) if b > a]


def film_resolve_host(sums: np.ndarray, width: int, rows: int, spp_total: int,
                      samples_done: int) -> np.ndarray:
    """spt_film_resolve_host(): the CPU statement of the film's resolve (no device)."""
    a = np.ascontiguousarray(sums, dtype=np.uint64)
    info = spt_film_info(int(width), int(rows), int(spp_total), int(samples_done))
    if a.size != 3 * max(info.rows, 0) * max(info.width, 0):
        raise SptError(1, "sums do not have rows * width * 3 elements")
    out = np.empty((max(info.rows, 0), max(info.width, 0), 3), dtype=np.float32)
    _check(load_library().spt_film_resolve_host(a.ctypes.data, ctypes.byref(info), out.ctypes.data))
    return out


def film_noise_map_host(sums: np.ndarray, m2: np.ndarray, width: int, rows: int, spp_total: int,
                        samples_done: int, batch: int, batches_done: int) -> np.ndarray:
    """spt_film_noise_map_host(): the CPU statement of the error map (no device). m2: rows * width
    * 3 pairs (lo, hi) of uint64. -> (rows, width, 3) float32 standard errors."""
    a, m, _, info, noise = _film_host_args(sums, m2, None, width, rows, spp_total, samples_done, batch,
                                           batches_done)
    out = np.empty((max(info.rows, 0), max(info.width, 0), 3), dtype=np.float32)
    _check(load_library().spt_film_noise_map_host(a.ctypes.data, m.ctypes.data, ctypes.byref(info),
                                                  ctypes.byref(noise), out.ctypes.data))
    return out


def film_noise_summary_host(sums: np.ndarray, m2: np.ndarray, width: int, rows: int, spp_total: int,
                            samples_done: int, batch: int, batches_done: int) -> dict:
    """spt_film_noise_summary_host(): the CPU statement of the image figures -> {"rmse": [r, g, b],
    "rmse_all", "se_max", "clamped", "batches_done"}."""
    a, m, _, info, noise = _film_host_args(sums, m2, None, width, rows, spp_total, samples_done, batch,
                                           batches_done)
    out = spt_noise_summary()
    _check(load_library().spt_film_noise_summary_host(a.ctypes.data, m.ctypes.data,
                                                      ctypes.byref(info), ctypes.byref(noise),
                                                      ctypes.byref(out)))
    return out.as_dict()


def _film_host_args(sums, m2, counts, width, rows, spp_total, samples_done, batch, batches_done):
    """The host statements' arguments: contiguous arrays of the film's sizes (m2 / counts: None where
    the statement takes none), the film info and the noise info."""
    a = np.ascontiguousarray(sums, dtype=np.uint64)
    m = None if m2 is None else np.ascontiguousarray(m2, dtype=np.uint64)
    c = None if counts is None else np.ascontiguousarray(counts, dtype=np.uint32)
    info = spt_film_info(int(width), int(rows), int(spp_total), int(samples_done))
    noise = spt_film_noise_info(1, int(batch), int(batches_done))
    npix = max(info.rows, 0) * max(info.width, 0)
    if a.size != 3 * npix or (m is not None and m.size != 6 * npix) or \
            (c is not None and c.size != npix):
        raise SptError(1, "sums / m2 do not have rows * width * 3 elements / pairs" if c is None else
                       "sums / m2 / counts do not have the film's elements")
    return a, m, c, info, noise


def film_adaptive_resolve_host(sums, counts, width: int, rows: int, spp_total: int,
                               batch: int) -> np.ndarray:
    """spt_film_adaptive_resolve_host(): the resolve with every pixel's own count (no device)."""
    a, _, c, info, noise = _film_host_args(sums, None, counts, width, rows, spp_total, 0, batch, 0)
    out = np.empty((max(info.rows, 0), max(info.width, 0), 3), dtype=np.float32)
    _check(load_library().spt_film_adaptive_resolve_host(a.ctypes.data, c.ctypes.data,
                                                         ctypes.byref(info), ctypes.byref(noise),
                                                         out.ctypes.data))
    return out


def film_adaptive_noise_map_host(sums, m2, counts, width: int, rows: int, spp_total: int,
                                 batch: int) -> np.ndarray:
    """spt_film_adaptive_noise_map_host(): the error map with every pixel's own count."""
    a, m, c, info, noise = _film_host_args(sums, m2, counts, width, rows, spp_total, 0, batch, 0)
    out = np.empty((max(info.rows, 0), max(info.width, 0), 3), dtype=np.float32)
    _check(load_library().spt_film_adaptive_noise_map_host(a.ctypes.data, m.ctypes.data, c.ctypes.data,
                                                           ctypes.byref(info), ctypes.byref(noise),
                                                           out.ctypes.data))
    return out


def film_adaptive_noise_summary_host(sums, m2, counts, width: int, rows: int, spp_total: int,
                                     batch: int, front: int) -> dict:
    """spt_film_adaptive_noise_summary_host(): the image figures (the mean over all pixels), each
    pixel with its own count; batches_done reports `front`."""
    a, m, c, info, noise = _film_host_args(sums, m2, counts, width, rows, spp_total,
                                           int(front) * int(batch), batch, front)
    out = spt_noise_summary()
    _check(load_library().spt_film_adaptive_noise_summary_host(a.ctypes.data, m.ctypes.data,
                                                               c.ctypes.data, ctypes.byref(info),
                                                               ctypes.byref(noise), ctypes.byref(out)))
    return out.as_dict()


def film_adaptive_select_host(sums, m2, counts, width: int, rows: int, spp_total: int, batch: int,
                              front: int, threshold: float, keep=None):
    """spt_film_adaptive_select_host(): -> (the new counts plane (rows, width) uint32, the new active
    list ascending). keep: rows * width bytes or None."""
    a, m, c, info, noise = _film_host_args(sums, m2, counts, width, rows, spp_total,
                                           int(front) * int(batch), batch, front)
    k = None if keep is None else np.ascontiguousarray(keep, dtype=np.uint8)
    if k is not None and k.size != c.size:
        raise SptError(1, "keep does not have rows * width bytes")
    out = np.zeros((max(info.rows, 0), max(info.width, 0)), dtype=np.uint32)
    lst = np.zeros(max(1, c.size), dtype=np.uint32)
    n = ctypes.c_int64(0)
    _check(load_library().spt_film_adaptive_select_host(
        a.ctypes.data, m.ctypes.data, c.ctypes.data, ctypes.byref(info), ctypes.byref(noise),
        float(threshold), None if k is None else k.ctypes.data, out.ctypes.data, lst.ctypes.data,
        ctypes.byref(n)))
    return out, lst[: n.value].copy()


def film_noise_pool_map_host(sums, m2, counts, width: int, rows: int, spp_total: int, batch: int,
                             batches_done: int, radius: int, exclude_center: bool = False,
                             band_rows: int = 0) -> np.ndarray:
    """spt_film_noise_pool_map_host(): the error pooled over every pixel's (2 radius + 1)^2 window.
    counts: None for a uniform noise film (batches_done batches everywhere), else an adaptive film's
    plane. band_rows: 0, or the tile_rows of a sharded film (no window crosses a band)."""
    a, m, c, info, noise = _film_host_args(sums, m2, counts, width, rows, spp_total,
                                           int(batches_done) * int(batch), batch, batches_done)
    out = np.empty((max(info.rows, 0), max(info.width, 0), 3), dtype=np.float32)
    _check(load_library().spt_film_noise_pool_map_host(
        a.ctypes.data, m.ctypes.data, None if c is None else c.ctypes.data, ctypes.byref(info),
        ctypes.byref(noise), int(band_rows), int(radius),
        POOL_EXCLUDE_CENTER if exclude_center else 0, out.ctypes.data))
    return out


def film_adaptive_select_pooled_host(sums, m2, counts, width: int, rows: int, spp_total: int,
                                     batch: int, front: int, threshold: float, radius: int,
                                     exclude_center: bool = False, keep=None, band_rows: int = 0):
    """spt_film_adaptive_select_pooled_host(): film_adaptive_select_host with the pooled clause ->
    (the new counts plane (rows, width) uint32, the new active list ascending)."""
    a, m, c, info, noise = _film_host_args(sums, m2, counts, width, rows, spp_total,
                                           int(front) * int(batch), batch, front)
    k = None if keep is None else np.ascontiguousarray(keep, dtype=np.uint8)
    if k is not None and k.size != c.size:
        raise SptError(1, "keep does not have rows * width bytes")
    out = np.zeros((max(info.rows, 0), max(info.width, 0)), dtype=np.uint32)
    lst = np.zeros(max(1, c.size), dtype=np.uint32)
    n = ctypes.c_int64(0)
    _check(load_library().spt_film_adaptive_select_pooled_host(
        a.ctypes.data, m.ctypes.data, c.ctypes.data, ctypes.byref(info), ctypes.byref(noise),
        int(band_rows), float(threshold), int(radius), POOL_EXCLUDE_CENTER if exclude_center else 0,
        None if k is None else k.ctypes.data, out.ctypes.data, lst.ctypes.data, ctypes.byref(n)))
    return out, lst[: n.value].copy()


def write_film_file(path: str, sums: np.ndarray, width: int, rows: int, spp_total: int,
                    samples_done: int, m2: np.ndarray | None = None, batch: int = 0,
                    batches_done: int = 0) -> None:
    """The film file: a 32-byte header (FILM_MAGIC, width, rows, spp_total, 0, samples_done; little
    endian) and the rows * width * 3 sums as raw little-endian uint64. With m2 (a noise film): the
    magic is FILM_MAGIC_NOISE, the header goes on with batch, 0, batches_done (48 bytes), and the
    moment plane (rows * width * 3 pairs (lo, hi) of uint64) follows the sums."""
    import struct
    a = np.ascontiguousarray(sums, dtype="<u8")
    if a.size != 3 * rows * width:
        raise SptError(1, "sums do not have rows * width * 3 elements")
    if m2 is None:
        with open(path, "wb") as f:
            f.write(struct.pack(_FILM_HEADER, FILM_MAGIC, width, rows, spp_total, 0, samples_done))
            f.write(a.tobytes())
        return
    m = np.ascontiguousarray(m2, dtype="<u8")
    if m.size != 6 * rows * width or batch < 1 or batches_done < 0:
        raise SptError(1, "m2 does not have rows * width * 3 pairs, or a bad batch")
    with open(path, "wb") as f:
        f.write(struct.pack(_FILM_HEADER_NOISE, FILM_MAGIC_NOISE, width, rows, spp_total, 0,
                            samples_done, batch, 0, batches_done))
        f.write(a.tobytes())
        f.write(m.tobytes())


def read_film_file(path: str, with_noise: bool = False):
    """-> (sums (rows, width, 3) uint64, {"width", "rows", "spp_total", "samples_done"}).
    with_noise: -> (sums, m2, info), for a noise film's file m2 = (rows, width, 3, 2) uint64 and info
    also holds "batch" and "batches_done"; for a plain film's m2 is None. Without with_noise a noise
    film's file is refused (its moments would be dropped)."""
    import struct
    data = open(path, "rb").read()
    n = struct.calcsize(_FILM_HEADER)
    if len(data) < n:
        raise SptError(1, f"{path}: not a film file")
    magic, w, rows, spp, _, done = struct.unpack(_FILM_HEADER, data[:n])
    if magic == FILM_MAGIC_NOISE and with_noise:
        n2 = struct.calcsize(_FILM_HEADER_NOISE)
        if len(data) < n2:
            raise SptError(1, f"{path}: not a film file")
        batch, _, bdone = struct.unpack("<iiq", data[n:n2])
        if w <= 0 or rows < 0 or spp <= 0 or not 0 <= done <= spp or batch < 1 or spp % batch \
                or spp // batch < 2 or not 0 <= bdone <= spp // batch or done % batch \
                or len(data) != n2 + 72 * rows * w:
            raise SptError(1, f"{path}: not a film file")
        words = np.frombuffer(data, dtype="<u8", offset=n2).astype(np.uint64)
        sums = words[: 3 * rows * w].reshape(rows, w, 3)
        m2 = words[3 * rows * w:].reshape(rows, w, 3, 2)
        return sums, m2, {"width": w, "rows": rows, "spp_total": spp, "samples_done": done,
                          "batch": batch, "batches_done": bdone}
    if magic != FILM_MAGIC or w <= 0 or rows < 0 or spp <= 0 or not 0 <= done <= spp \
            or len(data) != n + 24 * rows * w:
        raise SptError(1, f"{path}: not a film file")
    sums = np.frombuffer(data, dtype="<u8", offset=n).astype(np.uint64).reshape(rows, w, 3)
    info = {"width": w, "rows": rows, "spp_total": spp, "samples_done": done}
    return (sums, None, info) if with_noise else (sums, info)


class Film:
    """spt_film: the uint64 sums of the samples rendered so far, on the device. Passes over disjoint
    sample windows of one spp-sample image add up to the one-shot render bit for bit."""

    def __init__(self, params: spt_params, device: int = 0):
        self.lib = load_library()
        self._f = ctypes.c_void_p()
        _check(self.lib.spt_film_create(int(device), ctypes.byref(params), ctypes.byref(self._f)))
        self.device = device

    def close(self):
        if self._f:
            self.lib.spt_film_destroy(self._f)
            self._f = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def info(self) -> dict:
        i = spt_film_info()
        _check(self.lib.spt_film_info_get(self._f, ctypes.byref(i)))
        return {k: int(getattr(i, k)) for k, _ in i._fields_}

    def clear(self, stream_ptr: int = 0):
        _check(self.lib.spt_film_clear(self._f, ctypes.c_void_p(stream_ptr or None)))

    def render(self, renderer: "Renderer", prims, cam: Camera, params: spt_params, base: int,
               count: int, rgb_dev_ptr: int = 0, stream_ptr: int = 0):
        """Enqueue samples [base, base + count) of the params.spp-sample image and add them;
        rgb_dev_ptr (optional): the film resolved after the add, written by the same pass."""
        renderer._prims = _scene_array(prims)
        _check(self.lib.spt_film_render_async(renderer._ctx, self._f, renderer._prims, len(prims),
                                              ctypes.byref(cam._c), ctypes.byref(params), int(base),
                                              int(count), ctypes.c_void_p(rgb_dev_ptr or None),
                                              ctypes.c_void_p(stream_ptr or None)))

    def _float_plane(self, call, dev_ptr: int, stream_ptr: int):
        """A "device float plane" call (rows * width * 3 floats). With dev_ptr: enqueued into that
        buffer. Without: into a buffer of this call's own, returned on the host as (rows, width, 3)."""
        if dev_ptr:
            _check(call(self._f, ctypes.c_void_p(dev_ptr), ctypes.c_void_p(stream_ptr or None)))
            return None
        import torch
        with torch.cuda.device(self.device):
            buf = _film_buffer(self)
            _check(call(self._f, ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(stream_ptr or None)))
        return _film_image(self, buf)

    def _download(self, call, per_pixel: tuple, dtype, stream_ptr: int) -> np.ndarray:
        i = self.info()
        out = np.zeros((i["rows"], i["width"]) + per_pixel, dtype=dtype)
        _check(call(self._f, out.ctypes.data, ctypes.c_void_p(stream_ptr or None)))
        return out

    def _upload(self, call, plane, per_pixel: int, dtype, mismatch: str, stream_ptr: int, *state):
        i = self.info()
        a = np.ascontiguousarray(plane, dtype=dtype)
        if a.size != i["rows"] * i["width"] * per_pixel:
            raise SptError(1, mismatch)
        _check(call(self._f, a.ctypes.data, *state, ctypes.c_void_p(stream_ptr or None)))

    def resolve(self, rgb_dev_ptr: int = 0, stream_ptr: int = 0):
        """Film -> float image. With rgb_dev_ptr: enqueued into that device buffer. Without: into a
        buffer of this call's own, returned on the host as (rows, width, 3) float32."""
        return self._float_plane(self.lib.spt_film_resolve, rgb_dev_ptr, stream_ptr)

    def merge(self, other: "Film", stream_ptr: int = 0):
        """self += other (equal width, rows, spp_total; one device)."""
        _check(self.lib.spt_film_merge(self._f, other._f, ctypes.c_void_p(stream_ptr or None)))

    def to_numpy(self, stream_ptr: int = 0) -> np.ndarray:
        """The sums on the host: (rows, width, 3) uint64."""
        return self._download(self.lib.spt_film_download, (3,), np.uint64, stream_ptr)

    def from_numpy(self, sums: np.ndarray, samples_done: int, stream_ptr: int = 0):
        """Replace the sums (rows * width * 3 uint64) and samples_done: resume from a checkpoint."""
        self._upload(self.lib.spt_film_upload, sums, 3, np.uint64,
                     "sums do not have rows * width * 3 elements", stream_ptr, int(samples_done))

    def save(self, path: str):
        if self.adaptive_info()["enabled"]:
            raise SptError(1, "an adaptive film has no file format: checkpoint it with to_numpy, "
                              "noise_to_numpy and counts_to_numpy")
        i, n = self.info(), self.noise_info()
        if not n["enabled"]:
            write_film_file(path, self.to_numpy(), i["width"], i["rows"], i["spp_total"],
                            i["samples_done"])
        else:
            write_film_file(path, self.to_numpy(), i["width"], i["rows"], i["spp_total"],
                            i["samples_done"], self.noise_to_numpy(), n["batch"], n["batches_done"])

    # ---- the noise film (spt_film_noise_*) ----
    def enable_noise(self, batch: int):
        """Keep the moment plane from now on (an empty film only): every pass is then one batch of
        `batch` samples at a base that is a multiple of it; batch must divide spp into >= 2."""
        _check(self.lib.spt_film_noise_enable(self._f, int(batch)))

    def noise_info(self) -> dict:
        i = spt_film_noise_info()
        _check(self.lib.spt_film_noise_info_get(self._f, ctypes.byref(i)))
        return {k: int(getattr(i, k)) for k, _ in i._fields_}

    def noise_to_numpy(self, stream_ptr: int = 0) -> np.ndarray:
        """The moment plane on the host: (rows, width, 3, 2) uint64, [..., 0] = lo, [..., 1] = hi."""
        return self._download(self.lib.spt_film_noise_download, (3, 2), np.uint64, stream_ptr)

    def noise_from_numpy(self, m2: np.ndarray, batches_done: int, stream_ptr: int = 0):
        """Replace the moment plane and batches_done (beside from_numpy: a checkpoint's other half)."""
        self._upload(self.lib.spt_film_noise_upload, m2, 6, np.uint64,
                     "m2 does not have rows * width * 3 pairs", stream_ptr, int(batches_done))

    def noise_map(self, se_dev_ptr: int = 0, stream_ptr: int = 0):
        """The standard error of every resolved value. With se_dev_ptr: enqueued into that device
        buffer (rows * width * 3 floats). Without: returned on the host as (rows, width, 3) float32."""
        return self._float_plane(self.lib.spt_film_noise_map, se_dev_ptr, stream_ptr)

    def noise_pool_map(self, radius: int, exclude_center: bool = False, se_dev_ptr: int = 0,
                       stream_ptr: int = 0):
        """noise_map with every value's error pooled over the pixel's (2 radius + 1)^2 window (clipped
        to the film, and to the tile of a sharded film); exclude_center: without the pixel itself."""
        flags = POOL_EXCLUDE_CENTER if exclude_center else 0
        return self._float_plane(
            lambda f, dev, stream: self.lib.spt_film_noise_pool_map(f, int(radius), flags, dev, stream),
            se_dev_ptr, stream_ptr)

    def noise_summary(self, stream_ptr: int = 0) -> dict:
        """spt_film_noise_summary(): {"rmse": [r, g, b], "rmse_all", "se_max", "clamped",
        "batches_done"} of the clamped image; waits for the stream."""
        out = spt_noise_summary()
        _check(self.lib.spt_film_noise_summary(self._f, ctypes.byref(out),
                                               ctypes.c_void_p(stream_ptr or None)))
        return out.as_dict()

    # ---- the adaptive film (spt_film_adaptive_*) ----
    def enable_adaptive(self):
        """Per-pixel batch counts from now on (an empty noise film with at most 4096 batches): passes
        must come in window order and render the pixels still active (adaptive_select)."""
        _check(self.lib.spt_film_adaptive_enable(self._f))

    def adaptive_info(self) -> dict:
        i = spt_film_adaptive_info()
        _check(self.lib.spt_film_adaptive_info_get(self._f, ctypes.byref(i)))
        return {k: int(getattr(i, k)) for k in ("enabled", "front", "n_active", "samples_total")}

    def adaptive_select(self, threshold: float, keep=None, stream_ptr: int = 0, pool_radius: int = 0,
                        exclude_center: bool = False) -> int:
        """Retire the active pixels whose every channel has se <= threshold (threshold < 0: none by
        the error) or whose keep entry is 0; -> the pixels still active. keep: None, a device pointer
        (rows * width bytes), or an array (uploaded for this call). pool_radius > 0: se is the error
        pooled over the pixel's (2 pool_radius + 1)^2 window (spt_film_adaptive_select_pooled),
        exclude_center: without the pixel itself."""
        n = ctypes.c_int64(0)
        ptr, hold = None, None
        if keep is not None and not isinstance(keep, int):
            import torch
            k = np.ascontiguousarray(keep, dtype=np.uint8).reshape(-1)
            i = self.info()
            if k.size != i["rows"] * i["width"]:
                raise SptError(1, "keep does not have rows * width bytes")
            hold = torch.from_numpy(k).to(f"cuda:{self.device}")
            torch.cuda.synchronize(self.device)
            ptr = hold.data_ptr()
        elif keep:
            ptr = int(keep)
        if pool_radius:
            _check(self.lib.spt_film_adaptive_select_pooled(
                self._f, float(threshold), int(pool_radius), POOL_EXCLUDE_CENTER if exclude_center else 0,
                ctypes.c_void_p(ptr), ctypes.byref(n), ctypes.c_void_p(stream_ptr or None)))
        else:
            _check(self.lib.spt_film_adaptive_select(self._f, float(threshold), ctypes.c_void_p(ptr),
                                                     ctypes.byref(n), ctypes.c_void_p(stream_ptr or None)))
        del hold
        return int(n.value)

    def counts_to_numpy(self, stream_ptr: int = 0) -> np.ndarray:
        """The counts plane on the host: (rows, width) uint32 (COUNT_MASK, COUNT_RETIRED)."""
        return self._download(self.lib.spt_film_adaptive_download, (), np.uint32, stream_ptr)

    def counts_from_numpy(self, counts: np.ndarray, stream_ptr: int = 0):
        """Replace the counts plane (the last of a checkpoint's three uploads): rebuilds the active
        list and sets the front."""
        self._upload(self.lib.spt_film_adaptive_upload, counts, 1, np.uint32,
                     "counts do not have rows * width elements", stream_ptr)


# ---------------------------------------------------------------------------------------------
# Guide planes: first-hit albedo, normal, depth and coverage (spt_guide_*)
# ---------------------------------------------------------------------------------------------
GUIDE_PLANES = ("albedo", "normal", "depth", "coverage")


def guide_resolve_host(records: np.ndarray, width: int, rows: int, spp_total: int,
                       samples_done: int) -> dict:
    """spt_guide_resolve_host(): the CPU statement of the guide's resolve (no device). records:
    rows * width * 8 int64. -> {"albedo", "normal": (rows, width, 3), "depth", "coverage": (rows,
    width)} float32."""
    a = np.ascontiguousarray(records, dtype=np.int64)
    info = spt_guide_info(int(width), int(rows), int(spp_total), int(samples_done), 0, 0)
    rr, ww = max(info.rows, 0), max(info.width, 0)
    if a.size != GUIDE_SLOTS * rr * ww:
        raise SptError(1, "records do not have rows * width * 8 elements")
    out = {"albedo": np.empty((rr, ww, 3), np.float32), "normal": np.empty((rr, ww, 3), np.float32),
           "depth": np.empty((rr, ww), np.float32), "coverage": np.empty((rr, ww), np.float32)}
    _check(load_library().spt_guide_resolve_host(a.ctypes.data, ctypes.byref(info),
                                                 *[out[k].ctypes.data for k in GUIDE_PLANES]))
    return out


class Guide:
    """spt_guide: per pixel the integer sums of the first hit's colour, oriented normal, ray parameter
    and hit count over the samples added so far, on the device. The rays are the render's own camera
    rays, so passes over disjoint sample windows add up to one object whatever the split.
    through_specular: a guide of the specular chain (spt_guide_create_ex, SPT_GUIDE_THROUGH_SPECULAR):
    every pass follows mirrors and glass to the first DIFF surface; the default holds first hits."""

    def __init__(self, params: spt_params, device: int = 0, through_specular: bool = False):
        self.lib = load_library()
        self._g = ctypes.c_void_p()
        if through_specular:
            _check(self.lib.spt_guide_create_ex(int(device), ctypes.byref(params), GUIDE_THROUGH_SPECULAR,
                                                ctypes.byref(self._g)))
        else:
            _check(self.lib.spt_guide_create(int(device), ctypes.byref(params), ctypes.byref(self._g)))
        self.device = device

    def close(self):
        if self._g:
            self.lib.spt_guide_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def info(self) -> dict:
        i = spt_guide_info()
        _check(self.lib.spt_guide_info_get(self._g, ctypes.byref(i)))
        return {k: int(getattr(i, k)) for k, _ in i._fields_}

    def clear(self, stream_ptr: int = 0):
        _check(self.lib.spt_guide_clear(self._g, ctypes.c_void_p(stream_ptr or None)))

    def render(self, renderer: "Renderer", prims, cam: Camera, params: spt_params, base: int,
               count: int, stream_ptr: int = 0):
        """Enqueue the first hits of samples [base, base + count) of the params.spp-sample image and
        add them. The renderer's statistics and kernel() still describe its last render."""
        renderer._prims = _scene_array(prims)
        _check(self.lib.spt_guide_render_async(renderer._ctx, self._g, renderer._prims, len(prims),
                                               ctypes.byref(cam._c), ctypes.byref(params), int(base),
                                               int(count), ctypes.c_void_p(stream_ptr or None)))

    def to_numpy(self, stream_ptr: int = 0) -> np.ndarray:
        """The records on the host: (rows, width, 8) int64."""
        i = self.info()
        out = np.zeros((i["rows"], i["width"], GUIDE_SLOTS), dtype=np.int64)
        _check(self.lib.spt_guide_download(self._g, out.ctypes.data, ctypes.c_void_p(stream_ptr or None)))
        return out

    def resolve(self, planes=GUIDE_PLANES, stream_ptr: int = 0) -> dict:
        """The device resolve of the planes asked for -> {"albedo", "normal": (rows, width, 3),
        "depth", "coverage": (rows, width)} float32 on the host."""
        import torch
        i = self.info()
        n = i["rows"] * i["width"]
        with torch.cuda.device(self.device):
            bufs = {k: torch.empty(max(1, n * (3 if k in ("albedo", "normal") else 1)),
                                   dtype=torch.float32, device=f"cuda:{self.device}")
                    for k in GUIDE_PLANES if k in planes}
            _check(self.lib.spt_guide_resolve(
                self._g, *[ctypes.c_void_p(bufs[k].data_ptr() if k in bufs else None)
                           for k in GUIDE_PLANES], ctypes.c_void_p(stream_ptr or None)))
            torch.cuda.synchronize(self.device)
        out = {}
        for k, b in bufs.items():
            c = 3 if k in ("albedo", "normal") else 1
            a = b[: n * c].cpu().numpy()
            out[k] = a.reshape(i["rows"], i["width"], 3) if c == 3 else a.reshape(i["rows"], i["width"])
        return out


def render_guides(prims: Sequence[spt_prim], cam: Camera, params: spt_params,
                  through_specular: bool = False) -> dict:
    """The guide planes of the full window [0, params.spp): {"albedo", "normal", "depth",
    "coverage"} as float32 arrays on the host (Guide.resolve). through_specular: of a chain guide."""
    import torch
    r, g = Renderer(params.device), Guide(params, params.device, through_specular)
    try:
        with torch.cuda.device(params.device):
            g.render(r, prims, cam, params, 0, params.spp, torch.cuda.current_stream().cuda_stream)
            return g.resolve(stream_ptr=torch.cuda.current_stream().cuda_stream)
    finally:
        g.close()
        r.close()


# ---------------------------------------------------------------------------------------------
# Light guides: per-pixel light visibility and direct irradiance (spt_light_guide_*, spt_light_shade_*)
# ---------------------------------------------------------------------------------------------
LIGHT_GUIDE_PLANES = ("visibility", "direct", "tested")


def light_guide_resolve_host(records: np.ndarray, width: int, rows: int, spp_total: int,
                             samples_done: int) -> dict:
    """spt_light_guide_resolve_host(): the CPU statement of the light guide's resolve (no device).
    records: rows * width * 4 int64. -> {"visibility", "direct", "tested": (rows, width)} float32."""
    a = np.ascontiguousarray(records, dtype=np.int64)
    info = spt_guide_info(int(width), int(rows), int(spp_total), int(samples_done), 0, 0)
    rr, ww = max(info.rows, 0), max(info.width, 0)
    if a.size != LIGHT_GUIDE_SLOTS * rr * ww:
        raise SptError(1, "records do not have rows * width * 4 elements")
    out = {k: np.empty((rr, ww), np.float32) for k in LIGHT_GUIDE_PLANES}
    _check(load_library().spt_light_guide_resolve_host(a.ctypes.data, ctypes.byref(info),
                                                       *[out[k].ctypes.data for k in LIGHT_GUIDE_PLANES]))
    return out


def _shade_planes(albedo, visibility):
    a = np.ascontiguousarray(albedo, dtype=np.float32)
    v = np.ascontiguousarray(visibility, dtype=np.float32)
    if a.ndim < 1 or a.shape[-1] != 3 or a.size != 3 * v.size:
        raise SptError(1, "light_shade: albedo must hold three floats per visibility value")
    return a, v


def light_shade_host(albedo, visibility, shade_floor: float = 0.25, out=None) -> np.ndarray:
    """spt_light_shade_host(): albedo (.., 3) * (shade_floor + (1 - shade_floor) * visibility), the
    CPU statement (no device). out: a float32 array to write into (albedo itself is allowed)."""
    a, v = _shade_planes(albedo, visibility)
    if out is None:
        out = np.empty_like(a)
    elif out.dtype != np.float32 or not out.flags.c_contiguous or out.size != a.size:
        raise SptError(1, "light_shade_host: out must be a contiguous float32 array of albedo's size")
    _check(load_library().spt_light_shade_host(a.ctypes.data, v.ctypes.data, v.size, float(shade_floor),
                                               out.ctypes.data))
    return out


def light_shade(albedo, visibility, shade_floor: float = 0.25, device: int = 0, in_place: bool = False):
    """spt_light_shade_async() on host arrays (uploaded through torch) -> the shaded albedo on the
    host. in_place: the device call writes over its own albedo plane (out_dev == albedo_dev)."""
    import torch
    a, v = _shade_planes(albedo, visibility)
    with torch.cuda.device(device):
        da = torch.from_numpy(a.reshape(-1)).to(f"cuda:{device}")
        dv = torch.from_numpy(v.reshape(-1)).to(f"cuda:{device}")
        do = da if in_place else torch.empty_like(da)
        V = ctypes.c_void_p
        _check(load_library().spt_light_shade_async(V(da.data_ptr() or None), V(dv.data_ptr() or None), v.size,
                                                    float(shade_floor), V(do.data_ptr() or None),
                                                    V(torch.cuda.current_stream().cuda_stream or None)))
        torch.cuda.synchronize(device)
        return do.cpu().numpy().reshape(a.shape)


class LightGuide:
    """spt_light_guide: per pixel the integer counts of the samples whose guide vertex was tested
    against the light and of those that were lit, and the fixed-point sum of the lit ones' NEE weight, on
    the device. The vertex is the guide's (through_specular: the chain guide's), the shadow ray goes to a
    uniform point of params' light rectangle; passes over disjoint sample windows add up to one object."""

    def __init__(self, params: spt_params, device: int = 0, through_specular: bool = False):
        self.lib = load_library()
        self._g = ctypes.c_void_p()
        _check(self.lib.spt_light_guide_create(int(device), ctypes.byref(params),
                                               GUIDE_THROUGH_SPECULAR if through_specular else 0,
                                               ctypes.byref(self._g)))
        self.device = device

    def close(self):
        if self._g:
            self.lib.spt_light_guide_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def info(self) -> dict:
        i = spt_guide_info()
        _check(self.lib.spt_light_guide_info_get(self._g, ctypes.byref(i)))
        return {k: int(getattr(i, k)) for k, _ in i._fields_}

    def clear(self, stream_ptr: int = 0):
        _check(self.lib.spt_light_guide_clear(self._g, ctypes.c_void_p(stream_ptr or None)))

    def render(self, renderer: "Renderer", prims, cam: Camera, params: spt_params, base: int,
               count: int, stream_ptr: int = 0):
        """Enqueue the light tests of samples [base, base + count) of the params.spp-sample image and
        add them. The renderer's statistics and kernel() still describe its last render."""
        renderer._prims = _scene_array(prims)
        _check(self.lib.spt_light_guide_render_async(renderer._ctx, self._g, renderer._prims, len(prims),
                                                     ctypes.byref(cam._c), ctypes.byref(params), int(base),
                                                     int(count), ctypes.c_void_p(stream_ptr or None)))

    def to_numpy(self, stream_ptr: int = 0) -> np.ndarray:
        """The records on the host: (rows, width, 4) int64."""
        i = self.info()
        out = np.zeros((i["rows"], i["width"], LIGHT_GUIDE_SLOTS), dtype=np.int64)
        _check(self.lib.spt_light_guide_download(self._g, out.ctypes.data,
                                                 ctypes.c_void_p(stream_ptr or None)))
        return out

    def resolve(self, planes=LIGHT_GUIDE_PLANES, stream_ptr: int = 0) -> dict:
        """The device resolve of the planes asked for -> {"visibility", "direct", "tested": (rows,
        width)} float32 on the host."""
        import torch
        i = self.info()
        n = i["rows"] * i["width"]
        with torch.cuda.device(self.device):
            bufs = {k: torch.empty(max(1, n), dtype=torch.float32, device=f"cuda:{self.device}")
                    for k in LIGHT_GUIDE_PLANES if k in planes}
            _check(self.lib.spt_light_guide_resolve(
                self._g, *[ctypes.c_void_p(bufs[k].data_ptr() if k in bufs else None)
                           for k in LIGHT_GUIDE_PLANES], ctypes.c_void_p(stream_ptr or None)))
            torch.cuda.synchronize(self.device)
        return {k: b[:n].cpu().numpy().reshape(i["rows"], i["width"]) for k, b in bufs.items()}


def render_light_guides(prims: Sequence[spt_prim], cam: Camera, params: spt_params,
                        through_specular: bool = False) -> dict:
    """The light guide's planes of the full window [0, params.spp): {"visibility", "direct", "tested"}
    as float32 arrays on the host (LightGuide.resolve). through_specular: at the chain guide's vertex."""
    import torch
    r, g = Renderer(params.device), LightGuide(params, params.device, through_specular)
    try:
        with torch.cuda.device(params.device):
            g.render(r, prims, cam, params, 0, params.spp, torch.cuda.current_stream().cuda_stream)
            return g.resolve(stream_ptr=torch.cuda.current_stream().cuda_stream)
    finally:
        g.close()
        r.close()


def _light_shaded_guides(r: "Renderer", guide: "Guide", prims, cam, params, n_guide: int,
                         through_specular: bool, shade_floor: float, stream) -> dict:
    """The guide's planes with the albedo shaded by a light guide of the same window [0, n_guide):
    {"albedo" (shaded), "normal", "depth", "coverage", "albedo_unshaded", "visibility"} on the host."""
    lg = LightGuide(params, params.device, through_specular)
    try:
        lg.render(r, prims, cam, params, 0, n_guide, stream)
        vis = lg.resolve(("visibility",), stream)["visibility"]
    finally:
        lg.close()
    planes = guide.resolve(stream_ptr=stream)
    planes["albedo_unshaded"] = planes["albedo"]
    planes["visibility"] = vis
    planes["albedo"] = light_shade(planes["albedo"], vis, shade_floor, params.device, in_place=True)
    return planes


def _film_buffer(film: Film):
    """A device float buffer for the film's resolved image (at least one element)."""
    import torch
    i = film.info()
    return torch.empty(max(1, i["rows"] * i["width"] * 3), dtype=torch.float32,
                       device=f"cuda:{film.device}")


def _film_image(film: Film, buf) -> np.ndarray:
    """Wait for the device and return the film's image in `buf` on the host: (rows, width, 3)."""
    import torch
    i = film.info()
    torch.cuda.synchronize(film.device)
    return buf[: i["rows"] * i["width"] * 3].cpu().numpy().reshape(i["rows"], i["width"], 3)


@_contextmanager
def _film_session(params: spt_params, batch: int = 0, adaptive: bool = False):
    """-> (renderer, film, image buffer, stream) on params.device, the film a noise film of `batch`
    (and adaptive) when asked; the renderer and the film are closed on the way out."""
    import torch
    r, film = Renderer(params.device), Film(params, params.device)
    try:
        if batch:
            film.enable_noise(batch)
        if adaptive:
            film.enable_adaptive()
        with torch.cuda.device(params.device):
            yield r, film, _film_buffer(film), torch.cuda.current_stream().cuda_stream
    finally:
        film.close()
        r.close()


def render_progressive(prims: Sequence[spt_prim], cam: Camera, params: spt_params, passes,
                       return_stats=False):
    """params.spp samples rendered as several launches through a Film: `passes` = a number of
    near-equal windows (sample_windows) or a list of (base, count). Returns the host image, equal to
    render()'s bit for bit when the windows cover [0, spp) once; return_stats: also the integer
    spt_stats fields summed over the passes (kernel_ms summed too)."""
    windows = sample_windows(params.spp, passes) if isinstance(passes, int) else list(passes)
    total = dict.fromkeys(STAT_KEYS + ["shadow_proven"], 0)
    total["kernel_ms"] = 0.0
    with _film_session(params) as (r, film, buf, stream):
        for k, (base, count) in enumerate(windows):
            last = k == len(windows) - 1
            film.render(r, prims, cam, params, base, count, buf.data_ptr() if last else 0, stream)
            st = r.stats()
            for key in total:
                total[key] += st[key]
        if not windows:
            film.resolve(buf.data_ptr(), stream)
        out = _film_image(film, buf)
    return (out, total) if return_stats else out


def _render_to_target(who: str, prims, cam, params, target_rmse, batch, min_batches, select, info_of):
    """render_until and render_adaptive: batches in index order until max(rmse) <= target_rmse.
    select(film, stream) -> the pixels still active (None: every batch renders every pixel);
    info_of(film, stream) -> the caller's info, to which "rmse" is added."""
    spp = int(params.spp)
    if batch is None:
        if spp % 8:
            raise ValueError(f"{who}: spp is no multiple of 8, give batch")
        batch = spp // 8
    need = max(2, int(min_batches))
    rmse = None
    with _film_session(params, batch, select is not None) as (r, film, buf, stream):
        for k in range(spp // batch):
            film.render(r, prims, cam, params, k * batch, batch, 0, stream)
            r.stats()  # a pass that hit the runaway guard raises here
            if k + 1 >= need:
                rmse = film.noise_summary(stream)["rmse"]
                if max(rmse) <= target_rmse:
                    break
                if select is not None and k + 1 < spp // batch and select(film, stream) == 0:
                    break
        film.resolve(buf.data_ptr(), stream)
        out = _film_image(film, buf)
        info = dict(info_of(film, stream), rmse=rmse)
    return out, info


def render_until(prims: Sequence[spt_prim], cam: Camera, params: spt_params, target_rmse: float,
                 batch: int | None = None, min_batches: int = 2, return_info=False):
    """Render until the image's estimated RMSE is at most target_rmse: batches of `batch` samples in
    index order into a noise film, params.spp the cap. After each batch from min_batches (>= 2) on the
    film's summary is read, and the render stops once max(rmse) <= target_rmse. Returns the resolved
    image (a preview when it stopped early; render()'s image bit for bit when every batch was
    rendered); return_info: also {"samples_done", "batches_done", "rmse"}.
    batch defaults to spp / 8 when 8 divides spp and must be given otherwise."""
    out, info = _render_to_target(
        "render_until", prims, cam, params, target_rmse, batch, min_batches, None,
        lambda film, stream: {"samples_done": film.info()["samples_done"],
                              "batches_done": film.noise_info()["batches_done"]})
    return (out, info) if return_info else out


def render_adaptive(prims: Sequence[spt_prim], cam: Camera, params: spt_params, target_rmse: float,
                    batch: int | None = None, min_batches: int = 4, threshold_scale: float = 1.0,
                    return_info=False, pool_radius: int = 0, pool_exclude_center: bool = False):
    """render_until with the samples going where the error is. Full batches until min_batches (at
    least 2; pass a small value to retire earlier). After every pass from then on the film's summary
    is read and the render stops once max(rmse) <= target_rmse; otherwise the pixels whose every
    channel has se <= threshold_scale * target_rmse retire (adaptive_select) and the next pass renders
    the rest, until nothing is active or every batch of params.spp is in. A pixel retired on its own
    estimate may look converged by luck: min_batches is the guard.
    pool_radius > 0 retires on the error pooled over the pixel's (2 pool_radius + 1)^2 window
    instead, pool_exclude_center without the pixel itself (the decision then does not depend on the
    pixel's own samples). Measured at C3: pool_radius=2 with
    pool_exclude_center=True keeps the true error at the estimate, which the default does not.
    Returns the resolved image; return_info: also {"front", "samples_total",
    "rmse", "counts", "pool_radius", "pool_exclude_center"}."""
    def info_of(film, stream):
        a = film.adaptive_info()
        return {"front": a["front"], "samples_total": a["samples_total"],
                "counts": film.counts_to_numpy(stream), "pool_radius": int(pool_radius),
                "pool_exclude_center": bool(pool_exclude_center)}

    out, info = _render_to_target(
        "render_adaptive", prims, cam, params, target_rmse, batch, min_batches,
        lambda film, stream: film.adaptive_select(threshold_scale * target_rmse, None, stream,
                                                  pool_radius, pool_exclude_center), info_of)
    return (out, info) if return_info else out


# ---------------------------------------------------------------------------------------------
# Denoising: the edge-stopping a-trous filter over a film's image, its error map and the guide planes
# (spt_denoise_*, spt_film_denoise)
# ---------------------------------------------------------------------------------------------
DenoiseParams = spt_denoise_params


def default_denoise_params(**kw) -> spt_denoise_params:
    """spt_denoise_default_params() with the given fields replaced."""
    p = spt_denoise_params()
    load_library().spt_denoise_default_params(ctypes.byref(p))
    for k, v in kw.items():
        if k not in dict(spt_denoise_params._fields_):
            raise TypeError(f"spt_denoise_params has no field {k!r}")
        setattr(p, k, v)
    return p


def _denoise_planes(rgb, se, albedo, normal, depth):
    """The five planes as contiguous float32 arrays, and (height, width) taken from rgb."""
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise SptError(1, "rgb is not (height, width, 3)")
    h, w = rgb.shape[:2]
    planes = [rgb] + [np.ascontiguousarray(a, dtype=np.float32) for a in (se, albedo, normal, depth)]
    for a, c, name in zip(planes, (3, 3, 3, 3, 1), ("rgb", "se", "albedo", "normal", "depth")):
        if a.size != h * w * c:
            raise SptError(1, f"{name} does not have height * width * {c} elements")
    return planes, h, w


def denoise_host(rgb, se, albedo, normal, depth, params: spt_denoise_params | None = None,
                 return_se=False):
    """spt_denoise_host(): the CPU statement of the filter (no device). Planes as (h, w, 3) float32,
    depth (h, w). -> the denoised image (h, w, 3), with return_se also se_out."""
    planes, h, w = _denoise_planes(rgb, se, albedo, normal, depth)
    p = params if params is not None else default_denoise_params()
    out = np.empty((h, w, 3), np.float32)
    se_out = np.empty((h, w, 3), np.float32) if return_se else None
    _check(load_library().spt_denoise_host(*[a.ctypes.data for a in planes], w, h, ctypes.byref(p),
                                           out.ctypes.data, se_out.ctypes.data if return_se else None))
    return (out, se_out) if return_se else out


def _pair_planes(rgb_a, se_a, rgb_b, se_b, albedo, normal, depth):
    """The seven planes of a pair as contiguous float32 arrays, and (height, width) from rgb_a."""
    planes, h, w = _denoise_planes(rgb_a, se_a, albedo, normal, depth)
    half_b = [np.ascontiguousarray(a, dtype=np.float32) for a in (rgb_b, se_b)]
    for a, name in zip(half_b, ("rgb_b", "se_b")):
        if a.size != h * w * 3:
            raise SptError(1, f"{name} does not have height * width * 3 elements")
    return [planes[0], planes[1], half_b[0], half_b[1]] + planes[2:], h, w


def _pair_flags(own_weights) -> int:
    return DENOISE_PAIR_OWN_WEIGHTS if own_weights is True else int(own_weights)


def denoise_pair_host(rgb_a, se_a, rgb_b, se_b, albedo, normal, depth,
                      params: spt_denoise_params | None = None, own_weights=False, return_se=True,
                      return_diff=True):
    """spt_denoise_pair_host(): the CPU statement of the two-half filter (no device). own_weights: a
    bool, or the pair_flags word itself. -> (out, se_out, diff), each (h, w, 3) float32; a plane that
    was not asked for is None (and NULL in the call)."""
    planes, h, w = _pair_planes(rgb_a, se_a, rgb_b, se_b, albedo, normal, depth)
    p = params if params is not None else default_denoise_params()
    out = np.empty((h, w, 3), np.float32)
    se_out = np.empty((h, w, 3), np.float32) if return_se else None
    diff = np.empty((h, w, 3), np.float32) if return_diff else None
    _check(load_library().spt_denoise_pair_host(
        *[a.ctypes.data for a in planes], w, h, ctypes.byref(p), _pair_flags(own_weights), out.ctypes.data,
        se_out.ctypes.data if return_se else None, diff.ctypes.data if return_diff else None))
    return out, se_out, diff


def pair_summary_host(diff) -> dict:
    """spt_denoise_pair_summary_host(): {"rmse": [r, g, b], "rmse_all", "diff_max"} of a diff plane
    (h, w, 3)."""
    d = np.ascontiguousarray(diff, dtype=np.float32)
    if d.ndim != 3 or d.shape[2] != 3:
        raise SptError(1, "diff is not (height, width, 3)")
    out = spt_pair_summary()
    _check(load_library().spt_denoise_pair_summary_host(d.ctypes.data, d.shape[1], d.shape[0],
                                                        ctypes.byref(out)))
    return out.as_dict()


def default_bank_params(**kw) -> spt_bank_params:
    """spt_denoise_bank_default_params() with the given fields replaced."""
    b = spt_bank_params()
    load_library().spt_denoise_bank_default_params(ctypes.byref(b))
    for k, v in kw.items():
        if k not in ("error_iterations", "pair_flags"):
            raise TypeError(f"spt_bank_params has no settable field {k!r}")
        setattr(b, k, v)
    return b


def _bank_args(cands, bank, own_weights, error_iterations):
    """-> (the candidates as a ctypes array, their count, the spt_bank_params). cands: a sequence of
    spt_denoise_params. bank: an spt_bank_params, or None for the defaults with own_weights and
    error_iterations (None: the default) put in."""
    cands = list(cands)
    arr = (spt_denoise_params * max(len(cands), 1))()
    for k, c in enumerate(cands):
        ctypes.memmove(ctypes.byref(arr, k * ctypes.sizeof(spt_denoise_params)), ctypes.byref(c),
                       ctypes.sizeof(spt_denoise_params))
    if bank is None:
        bank = default_bank_params(pair_flags=_pair_flags(own_weights))
        if error_iterations is not None:
            bank.error_iterations = int(error_iterations)
    return arr, len(cands), bank


def bank_candidates(sigma_colors=(2.0, 4.0, 8.0), denoise: spt_denoise_params | None = None) -> list:
    """One copy of `denoise` (default: the defaults) per sigma_color: the bank's candidates."""
    cands = []
    for sc in sigma_colors:
        c = spt_denoise_params()
        ctypes.memmove(ctypes.byref(c), ctypes.byref(denoise if denoise is not None else default_denoise_params()),
                       ctypes.sizeof(c))
        c.sigma_color = float(sc)
        cands.append(c)
    return cands


def denoise_bank_host(rgb_a, se_a, rgb_b, se_b, albedo, normal, depth, cands, bank: spt_bank_params | None = None,
                      own_weights=True, error_iterations=None, return_mse=True, return_choice=True):
    """spt_denoise_bank_host(): the CPU statement of the filter bank (no device). cands: 1..4
    spt_denoise_params (bank_candidates()). -> (out (h, w, 3) float32, mse (h, w) float32, choice (h, w)
    uint8); a plane that was not asked for is None (and NULL in the call)."""
    planes, h, w = _pair_planes(rgb_a, se_a, rgb_b, se_b, albedo, normal, depth)
    arr, n, b = _bank_args(cands, bank, own_weights, error_iterations)
    out = np.empty((h, w, 3), np.float32)
    mse = np.empty((h, w), np.float32) if return_mse else None
    choice = np.empty((h, w), np.uint8) if return_choice else None
    _check(load_library().spt_denoise_bank_host(
        *[a.ctypes.data for a in planes], w, h, arr, n, ctypes.byref(b), out.ctypes.data,
        mse.ctypes.data if return_mse else None, choice.ctypes.data if return_choice else None))
    return out, mse, choice


def bank_summary_host(mse, choice) -> dict:
    """spt_denoise_bank_summary_host(): {"mse_mean", "rmse_est", "share": [4], "mse_min", "mse_max"} of an
    mse plane (h, w) float32 and a choice plane (h, w) uint8."""
    m = np.ascontiguousarray(mse, dtype=np.float32)
    c = np.ascontiguousarray(choice, dtype=np.uint8)
    if m.ndim != 2 or c.shape != m.shape:
        raise SptError(1, "mse and choice are not two (height, width) planes of one shape")
    out = spt_bank_summary()
    _check(load_library().spt_denoise_bank_summary_host(m.ctypes.data, c.ctypes.data, m.shape[1], m.shape[0],
                                                        ctypes.byref(out)))
    return out.as_dict()


class Denoiser:
    """spt_denoiser: the filter's scratch for width x height images on one device. Calls on one
    denoiser go on one stream."""

    def __init__(self, width: int, height: int, device: int = 0):
        self.lib = load_library()
        self._d = ctypes.c_void_p()
        _check(self.lib.spt_denoiser_create(int(device), int(width), int(height), ctypes.byref(self._d)))
        self.width, self.height, self.device = int(width), int(height), int(device)

    def close(self):
        if self._d:
            self.lib.spt_denoiser_destroy(self._d)
            self._d = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def _outputs(self, return_se: bool):
        import torch
        n = self.width * self.height * 3
        dev = f"cuda:{self.device}"
        return (torch.empty(n, dtype=torch.float32, device=dev),
                torch.empty(n, dtype=torch.float32, device=dev) if return_se else None)

    def _host(self, out, se_out):
        import torch
        torch.cuda.synchronize(self.device)
        shape = (self.height, self.width, 3)
        img = out.cpu().numpy().reshape(shape)
        return (img, se_out.cpu().numpy().reshape(shape)) if se_out is not None else img

    def denoise_async(self, rgb_ptr: int, se_ptr: int, albedo_ptr: int, normal_ptr: int, depth_ptr: int,
                      params: spt_denoise_params, out_ptr: int, se_out_ptr: int = 0, stream_ptr: int = 0):
        """spt_denoise_async() on device pointers."""
        V = ctypes.c_void_p
        _check(self.lib.spt_denoise_async(self._d, V(rgb_ptr or None), V(se_ptr or None),
                                          V(albedo_ptr or None), V(normal_ptr or None),
                                          V(depth_ptr or None), ctypes.byref(params), V(out_ptr or None),
                                          V(se_out_ptr or None), V(stream_ptr or None)))

    def denoise(self, rgb, se, albedo, normal, depth, params: spt_denoise_params | None = None,
                return_se=False):
        """Host arrays in (uploaded through torch), the denoised image out: (h, w, 3) float32, with
        return_se also se_out."""
        import torch
        planes, h, w = _denoise_planes(rgb, se, albedo, normal, depth)
        if (h, w) != (self.height, self.width):
            raise SptError(1, "the planes are not the denoiser's height x width")
        p = params if params is not None else default_denoise_params()
        with torch.cuda.device(self.device):
            dev = [torch.from_numpy(a.reshape(-1)).to(f"cuda:{self.device}") for a in planes]
            out, se_out = self._outputs(return_se)
            self.denoise_async(*[t.data_ptr() for t in dev], p, out.data_ptr(),
                               se_out.data_ptr() if return_se else 0,
                               torch.cuda.current_stream().cuda_stream)
            return self._host(out, se_out)

    def denoise_film_async(self, film: "Film", guide: "Guide", params: spt_denoise_params, out_ptr: int,
                           se_out_ptr: int = 0, stream_ptr: int = 0):
        """spt_film_denoise() into device pointers."""
        V = ctypes.c_void_p
        _check(self.lib.spt_film_denoise(film._f, guide._g, self._d, ctypes.byref(params),
                                         V(out_ptr or None), V(se_out_ptr or None), V(stream_ptr or None)))

    def denoise_film(self, film: "Film", guide: "Guide", params: spt_denoise_params | None = None,
                     return_se=False):
        """The film's image, its error map and the guide's planes resolved and filtered on the device
        in one call -> the denoised image on the host, with return_se also se_out."""
        import torch
        p = params if params is not None else default_denoise_params()
        with torch.cuda.device(self.device):
            out, se_out = self._outputs(return_se)
            self.denoise_film_async(film, guide, p, out.data_ptr(), se_out.data_ptr() if return_se else 0,
                                    torch.cuda.current_stream().cuda_stream)
            return self._host(out, se_out)


    # ---- the two-half filter (spt_denoise_pair_*, spt_film_pair_denoise) ----
    def _pair_outputs(self):
        import torch
        n = self.width * self.height * 3
        return [torch.empty(n, dtype=torch.float32, device=f"cuda:{self.device}") for _ in range(3)]

    def _pair_host(self, bufs):
        import torch
        torch.cuda.synchronize(self.device)
        return tuple(b.cpu().numpy().reshape(self.height, self.width, 3) for b in bufs)

    def denoise_pair_async(self, rgb_a_ptr: int, se_a_ptr: int, rgb_b_ptr: int, se_b_ptr: int,
                           albedo_ptr: int, normal_ptr: int, depth_ptr: int, params: spt_denoise_params,
                           pair_flags: int, out_ptr: int, se_out_ptr: int = 0, diff_ptr: int = 0,
                           stream_ptr: int = 0):
        """spt_denoise_pair_async() on device pointers."""
        V = ctypes.c_void_p
        ins = (rgb_a_ptr, se_a_ptr, rgb_b_ptr, se_b_ptr, albedo_ptr, normal_ptr, depth_ptr)
        _check(self.lib.spt_denoise_pair_async(self._d, *[V(x or None) for x in ins], ctypes.byref(params),
                                               int(pair_flags), V(out_ptr or None), V(se_out_ptr or None),
                                               V(diff_ptr or None), V(stream_ptr or None)))

    def denoise_pair(self, rgb_a, se_a, rgb_b, se_b, albedo, normal, depth,
                     params: spt_denoise_params | None = None, own_weights=False):
        """Host arrays in (uploaded through torch) -> (out, se_out, diff) on the host, (h, w, 3) each."""
        import torch
        planes, h, w = _pair_planes(rgb_a, se_a, rgb_b, se_b, albedo, normal, depth)
        if (h, w) != (self.height, self.width):
            raise SptError(1, "the planes are not the denoiser's height x width")
        p = params if params is not None else default_denoise_params()
        with torch.cuda.device(self.device):
            dev = [torch.from_numpy(a.reshape(-1)).to(f"cuda:{self.device}") for a in planes]
            bufs = self._pair_outputs()
            self.denoise_pair_async(*[t.data_ptr() for t in dev], p, _pair_flags(own_weights),
                                    *[b.data_ptr() for b in bufs], torch.cuda.current_stream().cuda_stream)
            return self._pair_host(bufs)

    def denoise_film_pair_async(self, film_a: "Film", film_b: "Film", guide: "Guide",
                                params: spt_denoise_params, pair_flags: int, out_ptr: int,
                                se_out_ptr: int = 0, diff_ptr: int = 0, stream_ptr: int = 0):
        """spt_film_pair_denoise() into device pointers."""
        V = ctypes.c_void_p
        _check(self.lib.spt_film_pair_denoise(film_a._f, film_b._f, guide._g, self._d, ctypes.byref(params),
                                              int(pair_flags), V(out_ptr or None), V(se_out_ptr or None),
                                              V(diff_ptr or None), V(stream_ptr or None)))

    def denoise_film_pair(self, film_a: "Film", film_b: "Film", guide: "Guide",
                          params: spt_denoise_params | None = None, own_weights=False, return_summary=False):
        """Both films' images and error maps and the guide's planes resolved and pair-filtered on the
        device in one call -> (out, se_out, diff) on the host; return_summary: also pair_summary of diff."""
        import torch
        p = params if params is not None else default_denoise_params()
        with torch.cuda.device(self.device):
            bufs = self._pair_outputs()
            stream = torch.cuda.current_stream().cuda_stream
            self.denoise_film_pair_async(film_a, film_b, guide, p, _pair_flags(own_weights),
                                         *[b.data_ptr() for b in bufs], stream)
            summary = self.pair_summary(bufs[2].data_ptr(), stream) if return_summary else None
            res = self._pair_host(bufs)
            return res + (summary,) if return_summary else res

    def pair_summary(self, diff, stream_ptr: int = 0) -> dict:
        """spt_denoise_pair_summary(): {"rmse": [r, g, b], "rmse_all", "diff_max"} of a diff plane: a
        device pointer (int), or a host array (h, w, 3) that is uploaded first; waits for the stream."""
        import torch
        out = spt_pair_summary()
        with torch.cuda.device(self.device):
            keep = None
            if not isinstance(diff, int):
                d = np.ascontiguousarray(diff, dtype=np.float32)
                if d.size != self.width * self.height * 3:
                    raise SptError(1, "diff does not have height * width * 3 elements")
                keep = torch.from_numpy(d.reshape(-1)).to(f"cuda:{self.device}")
                diff = keep.data_ptr()
                stream_ptr = stream_ptr or torch.cuda.current_stream().cuda_stream
            _check(self.lib.spt_denoise_pair_summary(self._d, ctypes.c_void_p(diff or None), ctypes.byref(out),
                                                     ctypes.c_void_p(stream_ptr or None)))
        return out.as_dict()


    # ---- the filter bank (spt_denoise_bank_*, spt_film_pair_denoise_bank) ----
    def _bank_outputs(self):
        import torch
        n, dev = self.width * self.height, f"cuda:{self.device}"
        return (torch.empty(n * 3, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev),
                torch.empty(n, dtype=torch.uint8, device=dev))

    def _bank_host(self, bufs):
        import torch
        torch.cuda.synchronize(self.device)
        h, w = self.height, self.width
        return (bufs[0].cpu().numpy().reshape(h, w, 3), bufs[1].cpu().numpy().reshape(h, w),
                bufs[2].cpu().numpy().reshape(h, w))

    def denoise_bank_async(self, rgb_a_ptr: int, se_a_ptr: int, rgb_b_ptr: int, se_b_ptr: int, albedo_ptr: int,
                           normal_ptr: int, depth_ptr: int, cands, n_cands: int, bank: spt_bank_params,
                           out_ptr: int, mse_ptr: int = 0, choice_ptr: int = 0, stream_ptr: int = 0):
        """spt_denoise_bank_async() on device pointers; cands: a ctypes array of spt_denoise_params."""
        V = ctypes.c_void_p
        ins = (rgb_a_ptr, se_a_ptr, rgb_b_ptr, se_b_ptr, albedo_ptr, normal_ptr, depth_ptr)
        _check(self.lib.spt_denoise_bank_async(self._d, *[V(x or None) for x in ins], cands, int(n_cands),
                                               ctypes.byref(bank), V(out_ptr or None), V(mse_ptr or None),
                                               V(choice_ptr or None), V(stream_ptr or None)))

    def denoise_bank(self, rgb_a, se_a, rgb_b, se_b, albedo, normal, depth, cands,
                     bank: spt_bank_params | None = None, own_weights=True, error_iterations=None):
        """Host arrays in (uploaded through torch) -> (out (h, w, 3), mse (h, w), choice (h, w) uint8) on
        the host."""
        import torch
        planes, h, w = _pair_planes(rgb_a, se_a, rgb_b, se_b, albedo, normal, depth)
        if (h, w) != (self.height, self.width):
            raise SptError(1, "the planes are not the denoiser's height x width")
        arr, n, b = _bank_args(cands, bank, own_weights, error_iterations)
        with torch.cuda.device(self.device):
            dev = [torch.from_numpy(a.reshape(-1)).to(f"cuda:{self.device}") for a in planes]
            bufs = self._bank_outputs()
            self.denoise_bank_async(*[t.data_ptr() for t in dev], arr, n, b, *[x.data_ptr() for x in bufs],
                                    torch.cuda.current_stream().cuda_stream)
            return self._bank_host(bufs)

    def denoise_film_bank_async(self, film_a: "Film", film_b: "Film", guide: "Guide", cands, n_cands: int,
                                bank: spt_bank_params, out_ptr: int, mse_ptr: int = 0, choice_ptr: int = 0,
                                stream_ptr: int = 0):
        """spt_film_pair_denoise_bank() into device pointers."""
        V = ctypes.c_void_p
        _check(self.lib.spt_film_pair_denoise_bank(film_a._f, film_b._f, guide._g, self._d, cands, int(n_cands),
                                                   ctypes.byref(bank), V(out_ptr or None), V(mse_ptr or None),
                                                   V(choice_ptr or None), V(stream_ptr or None)))

    def denoise_film_bank(self, film_a: "Film", film_b: "Film", guide: "Guide", cands,
                          bank: spt_bank_params | None = None, own_weights=True, error_iterations=None,
                          return_summary=False):
        """Both films and the guide resolved and run through the filter bank on the device in one call ->
        (out, mse, choice) on the host; return_summary: also bank_summary of mse and choice."""
        import torch
        arr, n, b = _bank_args(cands, bank, own_weights, error_iterations)
        with torch.cuda.device(self.device):
            bufs = self._bank_outputs()
            stream = torch.cuda.current_stream().cuda_stream
            self.denoise_film_bank_async(film_a, film_b, guide, arr, n, b, *[x.data_ptr() for x in bufs], stream)
            summary = self.bank_summary(bufs[1].data_ptr(), bufs[2].data_ptr(), stream) if return_summary else None
            res = self._bank_host(bufs)
            return res + (summary,) if return_summary else res

    def bank_summary(self, mse, choice, stream_ptr: int = 0) -> dict:
        """spt_denoise_bank_summary(): {"mse_mean", "rmse_est", "share", "mse_min", "mse_max"} of an mse and
        a choice plane: two device pointers (int), or two host arrays (h, w) that are uploaded first; waits
        for the stream."""
        import torch
        out = spt_bank_summary()
        with torch.cuda.device(self.device):
            keep = None
            if not isinstance(mse, int):
                m = np.ascontiguousarray(mse, dtype=np.float32)
                c = np.ascontiguousarray(choice, dtype=np.uint8)
                if m.size != self.width * self.height or c.size != m.size:
                    raise SptError(1, "mse or choice does not have height * width elements")
                keep = [torch.from_numpy(a.reshape(-1)).to(f"cuda:{self.device}") for a in (m, c)]
                mse, choice = keep[0].data_ptr(), keep[1].data_ptr()
                stream_ptr = stream_ptr or torch.cuda.current_stream().cuda_stream
            _check(self.lib.spt_denoise_bank_summary(self._d, ctypes.c_void_p(mse or None),
                                                     ctypes.c_void_p(choice or None), ctypes.byref(out),
                                                     ctypes.c_void_p(stream_ptr or None)))
        return out.as_dict()


def render_denoised(prims: Sequence[spt_prim], cam: Camera, params: spt_params, batch: int | None = None,
                    guide_spp: int | None = None, denoise: spt_denoise_params | None = None,
                    return_info=False, through_specular: bool = False, light_guide: bool = False,
                    shade_floor: float = 0.25):
    """Render all params.spp samples into a noise film (batches of `batch`, default spp / 8 as in
    render_until), fill a guide (through_specular: a chain guide, see Guide) with the sample window
    [0, min(spp, guide_spp or 64)), and return the
    film's image denoised (Denoiser.denoise_film). One device. return_info: also {"noisy": the film's
    own image, "noise": the film's noise_summary, "guides": the guide planes, "se": se_out}.
    light_guide: a light guide (LightGuide, the same window and kind as the guide) shades the albedo
    plane, albedo * (shade_floor + (1 - shade_floor) * visibility), before the filter takes it as its
    demodulation divisor and as the input of its albedo weight, so a shadow edge becomes an albedo
    edge. The planes are then resolved one by one (film resolve, error map, guide resolve) and filtered
    by Denoiser.denoise; "guides" also holds "visibility" and "albedo_unshaded". Off (the default), the
    calls are spt_film_denoise's as ever."""
    spp = int(params.spp)
    if params.shard_count > 1:
        raise SptError(1, "render_denoised: a shard's rows are not image neighbours; gather the planes")
    if batch is None:
        if spp % 8:
            raise SptError(1, "render_denoised: spp is no multiple of 8, give batch")
        batch = spp // 8
    if batch < 1 or spp % batch:
        raise SptError(1, "render_denoised: batch must divide spp (every sample is rendered)")
    n_guide = min(spp, int(guide_spp or 64))
    guide = Guide(params, params.device, through_specular)
    dn = None
    try:
        dn = Denoiser(params.width, params.height, params.device)
        with _film_session(params, batch) as (r, film, buf, stream):
            for k in range(spp // batch):
                film.render(r, prims, cam, params, k * batch, batch, 0, stream)
                r.stats()  # a pass that hit the runaway guard raises here
            guide.render(r, prims, cam, params, 0, n_guide, stream)
            if light_guide:
                planes = _light_shaded_guides(r, guide, prims, cam, params, n_guide, through_specular,
                                              shade_floor, stream)
                film.resolve(buf.data_ptr(), stream)
                noisy = _film_image(film, buf)
                out = dn.denoise(noisy, film.noise_map(stream_ptr=stream), planes["albedo"], planes["normal"],
                                 planes["depth"], denoise, return_se=return_info)
                if not return_info:
                    return out
                return out[0], {"noisy": noisy, "noise": film.noise_summary(stream), "guides": planes,
                                "se": out[1]}
            out = dn.denoise_film(film, guide, denoise, return_se=return_info)
            if not return_info:
                return out
            film.resolve(buf.data_ptr(), stream)
            info = {"noisy": _film_image(film, buf), "noise": film.noise_summary(stream),
                    "guides": guide.resolve(stream_ptr=stream), "se": out[1]}
            return out[0], info
    finally:
        if dn is not None:
            dn.close()
        guide.close()


# ---------------------------------------------------------------------------------------------
# Temporal accumulation (include/spt.h, SPT_HAS_TEMPORAL)
# ---------------------------------------------------------------------------------------------
def default_temporal_params(**kw) -> spt_temporal_params:
    """spt_temporal_default_params() with the given fields replaced."""
    p = spt_temporal_params()
    load_library().spt_temporal_default_params(ctypes.byref(p))
    for k, v in kw.items():
        if k not in dict(spt_temporal_params._fields_):
            raise TypeError(f"spt_temporal_params has no field {k!r}")
        setattr(p, k, v)
    return p


def _camera_struct(cam) -> spt_camera:
    return cam._c if isinstance(cam, Camera) else cam


def _temporal_state(h: int, w: int):
    """An empty state: its planes as a dict and the spt_temporal_state that points at them."""
    planes = {k: np.empty((h, w, c) if c > 1 else (h, w), np.float32) for k, c in TEMPORAL_STATE_PLANES}
    return planes, spt_temporal_state(*[planes[k].ctypes.data for k, _ in TEMPORAL_STATE_PLANES])


def temporal_accumulate_host(rgb, se, albedo, normal, depth, cam, params: spt_temporal_params | None = None,
                             prev: dict | None = None, prev_cam=None) -> dict:
    """spt_temporal_accumulate_host(): the CPU statement of one frame (no device). Planes as (h, w, 3)
    float32, depth (h, w); cam a Camera or an spt_camera; prev the "state" of the previous frame's result
    and prev_cam its camera (both None on a first frame). -> {"rgb", "se", "n", "hist", "state": {"c", "v",
    "n", "X", "N"}}."""
    planes, h, w = _denoise_planes(rgb, se, albedo, normal, depth)
    p = params if params is not None else default_temporal_params()
    out = {"rgb": np.empty((h, w, 3), np.float32), "se": np.empty((h, w, 3), np.float32),
           "n": np.empty((h, w), np.float32), "hist": np.empty((h, w, 3), np.float32)}
    state, nxt = _temporal_state(h, w)
    old, keep = None, []
    if prev is not None:
        for k, c in TEMPORAL_STATE_PLANES:
            a = np.ascontiguousarray(prev[k], dtype=np.float32)
            if a.size != h * w * c:
                raise SptError(1, f"the previous state's {k} does not have height * width * {c} elements")
            keep.append(a)
        old = spt_temporal_state(*[a.ctypes.data for a in keep])
    _check(load_library().spt_temporal_accumulate_host(
        *[a.ctypes.data for a in planes], w, h, ctypes.byref(_camera_struct(cam)), ctypes.byref(p),
        ctypes.byref(old) if old is not None else None,
        ctypes.byref(_camera_struct(prev_cam)) if prev_cam is not None else None,
        out["rgb"].ctypes.data, out["se"].ctypes.data, out["n"].ctypes.data, out["hist"].ctypes.data,
        ctypes.byref(nxt)))
    out["state"] = state
    return out


class TemporalAccumulator:
    """spt_temporal: the accumulated film of width x height frames on one device, reprojected into every
    new frame's camera. Calls on one accumulator go on one stream."""

    def __init__(self, width: int, height: int, device: int = 0):
        self.lib = load_library()
        self._t = ctypes.c_void_p()
        _check(self.lib.spt_temporal_create(int(device), int(width), int(height), ctypes.byref(self._t)))
        self.width, self.height, self.device = int(width), int(height), int(device)

    def close(self):
        if self._t:
            self.lib.spt_temporal_destroy(self._t)
            self._t = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def reset(self):
        """Drop the history: the next frame is a first frame."""
        _check(self.lib.spt_temporal_reset(self._t))

    def info(self) -> dict:
        i = spt_temporal_info()
        _check(self.lib.spt_temporal_info_get(self._t, ctypes.byref(i)))
        return {"frames": int(i.frames), "width": int(i.width), "height": int(i.height),
                "has_history": bool(i.has_history)}

    def state_to_numpy(self, stream_ptr: int = 0, return_camera=False):
        """The last frame's state on the host: {"c", "v", "n", "X", "N"}; return_camera: also its spt_camera."""
        state, st = _temporal_state(self.height, self.width)
        cam = spt_camera()
        _check(self.lib.spt_temporal_state_download(self._t, ctypes.byref(st), ctypes.byref(cam),
                                                    ctypes.c_void_p(stream_ptr or None)))
        return (state, cam) if return_camera else state

    def accumulate_async(self, rgb_ptr: int, se_ptr: int, albedo_ptr: int, normal_ptr: int, depth_ptr: int, cam,
                         params: spt_temporal_params, rgb_out_ptr: int, se_out_ptr: int, n_out_ptr: int = 0,
                         hist_ptr: int = 0, stream_ptr: int = 0):
        """spt_temporal_accumulate_async() on device pointers."""
        V = ctypes.c_void_p
        _check(self.lib.spt_temporal_accumulate_async(
            self._t, V(rgb_ptr or None), V(se_ptr or None), V(albedo_ptr or None), V(normal_ptr or None),
            V(depth_ptr or None), ctypes.byref(_camera_struct(cam)), ctypes.byref(params), V(rgb_out_ptr or None),
            V(se_out_ptr or None), V(n_out_ptr or None), V(hist_ptr or None), V(stream_ptr or None)))

    def accumulate_film_async(self, film: "Film", guide: "Guide", cam, params: spt_temporal_params,
                              rgb_out_ptr: int, se_out_ptr: int, n_out_ptr: int = 0, hist_ptr: int = 0,
                              albedo_ptr: int = 0, normal_ptr: int = 0, depth_ptr: int = 0, stream_ptr: int = 0):
        """spt_film_temporal_accumulate() into device pointers; albedo_ptr, normal_ptr, depth_ptr: where
        the guide's resolved planes go when the caller wants them (for a denoise call that follows)."""
        V = ctypes.c_void_p
        _check(self.lib.spt_film_temporal_accumulate(
            film._f, guide._g, self._t, ctypes.byref(_camera_struct(cam)), ctypes.byref(params),
            V(rgb_out_ptr or None), V(se_out_ptr or None), V(n_out_ptr or None), V(hist_ptr or None),
            V(albedo_ptr or None), V(normal_ptr or None), V(depth_ptr or None), V(stream_ptr or None)))

    def _outputs(self):
        import torch
        n, dev = self.width * self.height, f"cuda:{self.device}"
        return {k: torch.empty(n * c, dtype=torch.float32, device=dev)
                for k, c in (("rgb", 3), ("se", 3), ("n", 1), ("hist", 3))}

    def _host(self, bufs) -> dict:
        import torch
        torch.cuda.synchronize(self.device)
        return {k: t.cpu().numpy().reshape((self.height, self.width, 3) if k != "n" else (self.height, self.width))
                for k, t in bufs.items()}

    def accumulate(self, rgb, se, albedo, normal, depth, cam, params: spt_temporal_params | None = None) -> dict:
        """Host arrays in (uploaded through torch) -> {"rgb", "se", "n", "hist"} on the host."""
        import torch
        planes, h, w = _denoise_planes(rgb, se, albedo, normal, depth)
        if (h, w) != (self.height, self.width):
            raise SptError(1, "the planes are not the accumulator's height x width")
        p = params if params is not None else default_temporal_params()
        with torch.cuda.device(self.device):
            dev = [torch.from_numpy(a.reshape(-1)).to(f"cuda:{self.device}") for a in planes]
            o = self._outputs()
            self.accumulate_async(*[t.data_ptr() for t in dev], cam, p, o["rgb"].data_ptr(), o["se"].data_ptr(),
                                  o["n"].data_ptr(), o["hist"].data_ptr(), torch.cuda.current_stream().cuda_stream)
            return self._host(o)

    def accumulate_film(self, film: "Film", guide: "Guide", cam, params: spt_temporal_params | None = None) -> dict:
        """The film's image, its error map and the guide's planes resolved and accumulated on the device in
        one call -> {"rgb", "se", "n", "hist"} on the host."""
        import torch
        p = params if params is not None else default_temporal_params()
        with torch.cuda.device(self.device):
            o = self._outputs()
            self.accumulate_film_async(film, guide, cam, p, o["rgb"].data_ptr(), o["se"].data_ptr(),
                                       o["n"].data_ptr(), o["hist"].data_ptr(),
                                       stream_ptr=torch.cuda.current_stream().cuda_stream)
            return self._host(o)


def orbit_cameras(frames: int, degrees: float, lookfrom=LOOKFROM, lookat=(50, 40, 5), **camera_kw) -> list:
    """`frames` cameras: camera k has lookfrom rotated about the vertical axis through lookat by k * degrees
    (camera 0 is Camera(lookfrom, lookat, **camera_kw) itself)."""
    f, a = _v3(lookfrom), _v3(lookat)
    dx, dz = f[0] - a[0], f[2] - a[2]
    cams = []
    for k in range(int(frames)):
        if k == 0:
            cams.append(Camera(f, a, **camera_kw))
            continue
        t = math.radians(k * float(degrees))
        c, s = math.cos(t), math.sin(t)
        cams.append(Camera((a[0] + c * dx + s * dz, f[1], a[2] - s * dx + c * dz), a, **camera_kw))
    return cams


def render_sequence(prims: Sequence[spt_prim], cams, params: spt_params, batch: int | None = None,
                    temporal: bool = True, denoise: bool = True, denoise_params: spt_denoise_params | None = None,
                    temporal_params: spt_temporal_params | None = None, guide_spp: int | None = None) -> list:
    """One frame per camera of `cams`, frame k with the seed params.seed + k: a noise film of params.spp
    samples (batches of `batch`, default spp / 8) and a first-hit guide (the window [0, min(spp, guide_spp
    or 64))), accumulated over the frames before it (TemporalAccumulator.accumulate_film) and then filtered
    (Denoiser.denoise_async on the accumulated planes). -> the list of images, (h, w, 3) float32 each.
    temporal=False: every frame on its own, render_denoised() of that camera and seed bit for bit
    (denoise=False: the film's image). The scene must not change between the frames (spt.h)."""
    import torch
    spp = int(params.spp)
    if params.shard_count > 1:
        raise SptError(1, "render_sequence: a shard's rows are not image neighbours; gather the planes")
    if batch is None:
        if spp % 8:
            raise SptError(1, "render_sequence: spp is no multiple of 8, give batch")
        batch = spp // 8
    if batch < 1 or spp % batch or spp // batch < 2:
        raise SptError(1, "render_sequence: batch must divide spp into at least two batches")
    n_guide = min(spp, int(guide_spp or 64))
    frames = []

    def frame_params(k):
        p = spt_params.from_buffer_copy(params)
        p.seed = (int(params.seed) + k) & 0xFFFFFFFF
        return p

    if not temporal:
        for k, cam in enumerate(cams):
            p = frame_params(k)
            if denoise:
                frames.append(render_denoised(prims, cam, p, batch, guide_spp, denoise_params))
            else:
                with _film_session(p, batch) as (r, film, buf, stream):
                    for b in range(spp // batch):
                        film.render(r, prims, cam, p, b * batch, batch, 0, stream)
                        r.stats()
                    film.resolve(buf.data_ptr(), stream)
                    frames.append(_film_image(film, buf))
        return frames
    tp_params = temporal_params if temporal_params is not None else default_temporal_params()
    dn_params = denoise_params if denoise_params is not None else default_denoise_params()
    w, h, dev = int(params.width), int(params.height), f"cuda:{params.device}"
    acc = TemporalAccumulator(w, h, params.device)
    dn = Denoiser(w, h, params.device) if denoise else None
    r = Renderer(params.device)
    try:
        with torch.cuda.device(params.device):
            stream = torch.cuda.current_stream().cuda_stream
            new = lambda c: torch.empty(w * h * c, dtype=torch.float32, device=dev)  # noqa: E731
            rgb, se, albedo, normal, depth, out = new(3), new(3), new(3), new(3), new(1), new(3)
            for k, cam in enumerate(cams):
                p = frame_params(k)
                film, guide = Film(p, p.device), Guide(p, p.device)
                try:
                    film.enable_noise(batch)
                    for b in range(spp // batch):
                        film.render(r, prims, cam, p, b * batch, batch, 0, stream)
                        r.stats()  # a pass that hit the runaway guard raises here
                    guide.render(r, prims, cam, p, 0, n_guide, stream)
                    acc.accumulate_film_async(film, guide, cam, tp_params, rgb.data_ptr(), se.data_ptr(),
                                              albedo_ptr=albedo.data_ptr(), normal_ptr=normal.data_ptr(),
                                              depth_ptr=depth.data_ptr(), stream_ptr=stream)
                    img = rgb
                    if denoise:
                        dn.denoise_async(rgb.data_ptr(), se.data_ptr(), albedo.data_ptr(), normal.data_ptr(),
                                         depth.data_ptr(), dn_params, out.data_ptr(), 0, stream)
                        img = out
                    torch.cuda.synchronize(params.device)
                    frames.append(img.cpu().numpy().reshape(h, w, 3))
                finally:
                    guide.close()
                    film.close()
    finally:
        r.close()
        if dn is not None:
            dn.close()
        acc.close()
    return frames


def _pair_batch(who: str, params: spt_params, batch):
    """The batch size of a pair render: spp / batch even and at least 4 (two batches per half)."""
    spp = int(params.spp)
    if params.shard_count > 1:
        raise SptError(1, f"{who}: a shard's rows are not image neighbours; gather the planes")
    if batch is None:
        if spp % 8:
            raise SptError(1, f"{who}: spp is no multiple of 8, give batch")
        batch = spp // 8
    if batch < 1 or spp % batch or (spp // batch) % 2 or spp // batch < 4:
        raise SptError(1, f"{who}: batch must divide spp into an even number of batches, at least 4")
    return int(batch)


@_contextmanager
def _pair_session(params: spt_params, batch: int, through_specular: bool):
    """-> (renderer, film A, film B, guide, denoiser, stream) on params.device; everything is closed
    on the way out. The films are noise films of `batch`."""
    import torch
    made = []
    try:
        r = Renderer(params.device)
        made.append(r)
        films = []
        for _ in range(2):
            f = Film(params, params.device)
            made.append(f)
            f.enable_noise(batch)
            films.append(f)
        guide = Guide(params, params.device, through_specular)
        made.append(guide)
        dn = Denoiser(params.width, params.height, params.device)
        made.append(dn)
        with torch.cuda.device(params.device):
            yield r, films[0], films[1], guide, dn, torch.cuda.current_stream().cuda_stream
    finally:
        for o in reversed(made):
            o.close()


def render_denoised_pair(prims: Sequence[spt_prim], cam: Camera, params: spt_params,
                         batch: int | None = None, guide_spp: int | None = None,
                         denoise: spt_denoise_params | None = None, own_weights: bool = False,
                         through_specular: bool = False, return_info=False, light_guide: bool = False,
                         shade_floor: float = 0.25):
    """Render all params.spp samples into TWO noise films (batch k of `batch` samples, default spp / 8,
    into film A when k is even and into film B when it is odd; spp / batch must be even and at least
    4), fill a guide as render_denoised does, and return the two-half filter's image
    (Denoiser.denoise_film_pair). The default is cross weights: they give the better image (README);
    own_weights=True gives the error estimate that means what it says. One device. return_info: also
    {"diff": half the difference of the halves' results, "se": the propagated se_out, "pair": the
    summary of diff, "guides": the guide planes, "noisy": the resolve of A merged with B in a third
    film, which is render()'s image bit for bit}. light_guide, shade_floor: as render_denoised's -- the
    halves' images and error maps and the guide's planes are resolved one by one, the albedo shaded, and
    Denoiser.denoise_pair filters them."""
    spp = int(params.spp)
    batch = _pair_batch("render_denoised_pair", params, batch)
    n_guide = min(spp, int(guide_spp or 64))
    with _pair_session(params, batch, through_specular) as (r, fa, fb, guide, dn, stream):
        for k in range(spp // batch):
            (fb if k & 1 else fa).render(r, prims, cam, params, k * batch, batch, 0, stream)
            r.stats()  # a pass that hit the runaway guard raises here
        guide.render(r, prims, cam, params, 0, n_guide, stream)
        planes = None
        if light_guide:
            planes = _light_shaded_guides(r, guide, prims, cam, params, n_guide, through_specular, shade_floor,
                                          stream)
            out, se, diff = dn.denoise_pair(fa.resolve(stream_ptr=stream), fa.noise_map(stream_ptr=stream),
                                            fb.resolve(stream_ptr=stream), fb.noise_map(stream_ptr=stream),
                                            planes["albedo"], planes["normal"], planes["depth"], denoise,
                                            own_weights)
            pair = dn.pair_summary(diff, stream)
        else:
            out, se, diff, pair = dn.denoise_film_pair(fa, fb, guide, denoise, own_weights, return_summary=True)
        if not return_info:
            return out
        merged = Film(params, params.device)
        try:
            merged.enable_noise(batch)
            merged.merge(fa, stream)
            merged.merge(fb, stream)
            buf = _film_buffer(merged)
            merged.resolve(buf.data_ptr(), stream)
            noisy = _film_image(merged, buf)
        finally:
            merged.close()
        return out, {"diff": diff, "se": se, "pair": pair,
                     "guides": planes if planes is not None else guide.resolve(stream_ptr=stream),
                     "noisy": noisy}


def render_denoised_bank(prims: Sequence[spt_prim], cam: Camera, params: spt_params,
                         sigma_colors=(2.0, 4.0, 8.0), batch: int | None = None, guide_spp: int | None = None,
                         denoise: spt_denoise_params | None = None, own_weights: bool = True,
                         error_iterations: int | None = 3, through_specular: bool = False,
                         return_info=False):
    """render_denoised_pair's render (two noise films, a guide) through the filter bank
    (Denoiser.denoise_film_bank): one candidate per sigma_color (1..4 of them), the other filter
    parameters `denoise`'s (default: the defaults), per pixel the candidate of least cross-validated
    error, blended. One device. The defaults come from measurements (HEAD and mirror_glass, 256x192, 16
    seeds, 64 / 256 / 1024 spp): own weights, because with cross weights the estimate that picks
    the filter is not merely low but negative on renders (-1.0 to -1.4 times the true squared error), and
    three smoothing passes (error_iterations=None: the library's two), because the choice among noisy
    estimates is the weak point: RMSE over the film's 0.257 / 0.273 / 0.329 on HEAD with three passes,
    0.300 / 0.311 / 0.358 with two, beside 0.246 / 0.276 / 0.343 for sigma_color 8 alone and 0.239 / 0.258 /
    0.318 for render_denoised_pair's cross weights, which remain the better image where no error plane is
    wanted. The bank wins where the candidates fail in different places (the balls' silhouette band on
    mirror_glass: 0.583 / 0.599 / 0.620 against 0.585-0.765 for its candidates alone).
    return_info: also {"mse": the blended estimate of the squared
    error, "choice": the candidate each pixel chose, "bank": the summary of the two, "guides": the guide
    planes}."""
    spp = int(params.spp)
    batch = _pair_batch("render_denoised_bank", params, batch)
    n_guide = min(spp, int(guide_spp or 64))
    cands = bank_candidates(sigma_colors, denoise)
    with _pair_session(params, batch, through_specular) as (r, fa, fb, guide, dn, stream):
        for k in range(spp // batch):
            (fb if k & 1 else fa).render(r, prims, cam, params, k * batch, batch, 0, stream)
            r.stats()  # a pass that hit the runaway guard raises here
        guide.render(r, prims, cam, params, 0, n_guide, stream)
        out, mse, choice, summary = dn.denoise_film_bank(fa, fb, guide, cands, None, own_weights,
                                                         error_iterations, return_summary=True)
        if not return_info:
            return out
        return out, {"mse": mse, "choice": choice, "bank": summary, "guides": guide.resolve(stream_ptr=stream)}


def render_denoised_until(prims: Sequence[spt_prim], cam: Camera, params: spt_params, target_rmse: float,
                          batch: int | None = None, min_batches: int = 4, own_weights: bool = True,
                          guide_spp: int | None = None, denoise: spt_denoise_params | None = None,
                          through_specular: bool = False, estimate: str = "diff",
                          sigma_colors=(2.0, 4.0, 8.0)):
    """Render until the DENOISED image's measured error is at most target_rmse. The guide is rendered
    first; batches of `batch` samples go in index order alternately into film A (even k) and film B
    (odd k), params.spp the cap. After every second batch from min_batches on (rounded up to an even
    number, at least 4) the two-half filter runs and the summary of diff is read; the render stops once
    max(rmse) <= target_rmse. -> (the denoised image, {"samples_done", "batches_done", "rmse"}).
    The default is own weights, because the stopping number must mean what it says. Measured on
    renders (HEAD and mirror_glass, 256x192, 16 seeds, 64 / 256 / 1024 spp): the
    mean diff^2 over the variance of the result across seeds is 0.99-1.00 with own weights (the halves
    are independent, so this is exact in expectation) and 0.81 / 0.68 / 0.55 (HEAD), 0.72 / 0.55 / 0.42
    (mirror_glass) with cross weights, where the halves' results correlate. Over the true squared error
    against a 65536-spp render: 0.76-0.88 with own weights (the true RMSE is 1.06-1.15x the figure this
    call stops on), 0.26-0.46 with cross weights. Both read variance only: the filter's bias is not in
    diff (include/spt.h).
    estimate="bank" (opt-in): the filter bank runs instead (one candidate per sigma_colors, three
    smoothing passes, as render_denoised_bank) and the render stops once the bank summary's rmse_est,
    which sees bias, is at most target_rmse; "rmse" in the result is then that one figure and "bank" the
    whole summary. NOT recommended with several candidates: the least of several noisy estimates reads low
    by selection, and on the renders above mean mse over the true squared error is 0.37-0.69 (0.14-0.49
    with two passes), worse than diff's 0.76-0.88. With ONE sigma_color there is no selection and the
    figure does see bias: 0.74 / 0.85 / 0.86 at sigma_color 4 (diff: 0.80 / 0.85 / 0.76) and 0.52 / 0.69 /
    0.78 at 8 (diff: 0.50 / 0.49 / 0.39) on HEAD at 64 / 256 / 1024 spp; at 64 spp, four batches per half,
    it still reads low."""
    if estimate not in ("diff", "bank"):
        raise SptError(1, "render_denoised_until: estimate is 'diff' or 'bank'")
    spp = int(params.spp)
    batch = _pair_batch("render_denoised_until", params, batch)
    need = max(4, int(min_batches) + (int(min_batches) & 1))
    n_guide = min(spp, int(guide_spp or 64))
    with _pair_session(params, batch, through_specular) as (r, fa, fb, guide, dn, stream):
        guide.render(r, prims, cam, params, 0, n_guide, stream)
        out = rmse = None
        done = 0
        for k in range(spp // batch):
            (fb if k & 1 else fa).render(r, prims, cam, params, k * batch, batch, 0, stream)
            r.stats()  # a pass that hit the runaway guard raises here
            done = k + 1
            if done >= need and done % 2 == 0 and estimate == "bank":
                out, _mse, _choice, bank = dn.denoise_film_bank(fa, fb, guide,
                                                                bank_candidates(sigma_colors, denoise), None,
                                                                own_weights, 3, return_summary=True)
                rmse = bank["rmse_est"]
                if rmse <= target_rmse:
                    return out, {"samples_done": done * batch, "batches_done": done, "rmse": rmse, "bank": bank}
            elif done >= need and done % 2 == 0:
                out, _se, _diff, pair = dn.denoise_film_pair(fa, fb, guide, denoise, own_weights,
                                                             return_summary=True)
                rmse = pair["rmse"]
                if max(rmse) <= target_rmse:
                    break
        return out, {"samples_done": done * batch, "batches_done": done, "rmse": rmse}


def render_multi(prims: Sequence[spt_prim], cam: Camera, params: spt_params, devices,
                 return_stats=False):
    """One process, len(devices) GPUs (spt_render_multi): shard k on devices[k], one RCCL gather to
    devices[0]. Returns the full (h, w, 3) image, bit-identical to render() on one GPU."""
    lib = load_library()
    devs = (ctypes.c_int32 * len(devices))(*[int(d) for d in devices])
    out = np.empty((params.height, params.width, 3), dtype=np.float32)
    st = spt_stats()
    _check(lib.spt_render_multi(_scene_array(prims), len(prims), ctypes.byref(cam._c),
                                ctypes.byref(params), devs, len(devices),
                                out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                ctypes.byref(st)))
    return (out, st.as_dict()) if return_stats else out


COMM_ID_BYTES = 128


def comm_unique_id() -> bytes:
    """spt_comm_unique_id(): the RCCL unique id rank 0 hands to every rank."""
    buf = (ctypes.c_uint8 * COMM_ID_BYTES)()
    _check(load_library().spt_comm_unique_id(buf))
    return bytes(buf)


class Comm:
    """One rank of the framebuffer gather (spt_comm_*): RCCL over xGMI, rank 0 receives."""

    def __init__(self, unique_id: bytes, nranks: int, rank: int, device: int):
        self.lib = load_library()
        self._c = ctypes.c_void_p()
        idb = (ctypes.c_uint8 * COMM_ID_BYTES)(*unique_id)
        _check(self.lib.spt_comm_create(idb, int(nranks), int(rank), int(device),
                                        ctypes.byref(self._c)))
        self.nranks, self.rank, self.device = nranks, rank, device

    def close(self):
        if self._c:
            self.lib.spt_comm_destroy(self._c)
            self._c = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def reserve(self, params: spt_params):
        _check(self.lib.spt_comm_reserve(self._c, ctypes.byref(params)))

    def gather(self, params: spt_params, shard_dev_ptr: int, image_dev_ptr: int, stream_ptr: int = 0):
        """Enqueue the gather of this rank's shard (rank 0: into image_dev_ptr) on the stream."""
        _check(self.lib.spt_gather_framebuffer(self._c, ctypes.byref(params),
                                               ctypes.c_void_p(shard_dev_ptr),
                                               ctypes.c_void_p(image_dev_ptr or None),
                                               ctypes.c_void_p(stream_ptr or None)))


def gather_plan(params: spt_params, nranks: int, rank: int) -> list:
    """spt_gather_plan(): the (kind, peer, count, offset) transfers `rank` posts in one framebuffer
    gather (pure host function, no device)."""
    ops = (spt_gather_op * 64)()
    n = load_library().spt_gather_plan(ctypes.byref(params), int(nranks), int(rank), ops, 64)
    if n < 0:
        raise SptError(1, "spt_gather_plan: bad arguments")
    return [(ops[i].kind, ops[i].peer, int(ops[i].count), int(ops[i].offset)) for i in range(n)]


def gather_staging_floats(params: spt_params, nranks: int) -> int:
    return int(load_library().spt_gather_staging_floats(ctypes.byref(params), int(nranks)))


def deinterleave_source(params: spt_params, nranks: int, row: int) -> tuple:
    """(rank, compact row) the de-interleave kernel reads image row `row` from."""
    k, j = ctypes.c_int32(), ctypes.c_int32()
    _check(load_library().spt_deinterleave_source(ctypes.byref(params), int(nranks), int(row),
                                                  ctypes.byref(k), ctypes.byref(j)))
    return k.value, j.value


def shutdown() -> None:
    """spt_shutdown(): release spt_render's cached per-device contexts."""
    _check(load_library().spt_shutdown())


def deinterleave_rows(params: spt_params, shard_dev_ptrs, image_dev_ptr: int, stream_ptr: int = 0):
    """spt_deinterleave_rows(): shard k's compact rows (device pointers) -> the image."""
    arr = (ctypes.c_void_p * len(shard_dev_ptrs))(*[ctypes.c_void_p(int(x)) for x in shard_dev_ptrs])
    _check(load_library().spt_deinterleave_rows(ctypes.byref(params), len(shard_dev_ptrs), arr,
                                                ctypes.c_void_p(image_dev_ptr),
                                                ctypes.c_void_p(stream_ptr or None)))


# ---------------------------------------------------------------------------------------------
# Output (:313-321 toInt/clamp, :548-551 the P3 writer): encoded on the GPU (spt_image.hip)
# ---------------------------------------------------------------------------------------------
def _format(fmt) -> int:
    return IMAGE_FORMATS[fmt] if isinstance(fmt, str) else int(fmt)


def write_image(path: str, rgb: np.ndarray, fmt="p3", device: int = 0) -> None:
    """Write an (h, w, 3) float32 framebuffer as P3 (byte-identical to :548-551), P6 or PFM."""
    a = np.ascontiguousarray(rgb, dtype=np.float32)
    h, w, _ = a.shape
    _check(load_library().spt_write_image(device, a.ctypes.data, w, h, _format(fmt),
                                          path.encode()))


def write_ppm(path: str, rgb: np.ndarray, device: int = 0) -> None:
    """The reference's writer (:548-551): ASCII P3, '%d %d %d ' per pixel."""
    write_image(path, rgb, "p3", device)


class Encoder:
    """spt_encoder: device framebuffer -> file bytes in a device buffer (spt_encode_image)."""

    def __init__(self, device: int = 0):
        self._e = ctypes.c_void_p()
        _check(load_library().spt_encoder_create(device, ctypes.byref(self._e)))

    def close(self):
        if self._e:
            load_library().spt_encoder_destroy(self._e)
            self._e = None

    @staticmethod
    def bound(w: int, h: int, fmt="p3") -> int:
        return int(load_library().spt_image_bound(w, h, _format(fmt)))

    def encode(self, rgb_dev_ptr: int, w: int, h: int, fmt, out_dev_ptr: int, cap: int,
               stream: int = 0) -> int:
        n = ctypes.c_uint64()
        _check(load_library().spt_encode_image(self._e, rgb_dev_ptr, w, h, _format(fmt),
                                               out_dev_ptr, cap, ctypes.byref(n), stream or None))
        return int(n.value)


def flop_model(stats: dict, prims: Iterable[spt_prim], executed: bool = False) -> float:
    """include/spt_flops.h model (same as the C side): `flop`, or with executed=True
    `flop_executed` (only the traced shadow rays charged a scene test)."""
    scene = sum(19 if p.kind == SPHERE else 6 for p in prims)
    shadow = (stats["shadow_traced"] - stats.get("shadow_proven", 0)) if executed else stats["shadow_rays"]
    return (stats["samples"] * 40 + (stats["path_rays"] + shadow) * scene
            + stats["vertices"] * 11 + stats["sphere_vertices"] * 13
            + (stats["vertices"] - stats["samples"]) * 12
            + stats["cosine_samples"] * 65 + stats["nee_events"] * 19
            + stats["nee_light_hits"] * 14)


__all__ = [n for n in dir() if not n.startswith("_")]

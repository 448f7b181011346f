// spt_probe.hip — TEST INFRASTRUCTURE ONLY: the device building blocks of spt_device.h, each mapped
// over a device array by a kernel of its own, so tests/test_gpu_primitives.py can compare them with
// the oracle's spt_oracle_map word for word. Built by tests/probe/Makefile with the render kernel's
// HIPFLAGS (the contraction and division flags are what the comparison is about).
//
// Every launcher: int spt_probe_<name>(const uint32_t* in, uint32_t* out, long long n, void* stream)
// with device pointers, floats as their bits, element i at in + i * WI and out + i * WO (the widths
// of spt_oracle_map_width). Returns the hipError_t of the launch and the stream's synchronise.
#include "../../small-pathtracer_amd/csrc/spt_device.h"

namespace {

using namespace spt;

__device__ __forceinline__ float f(uint32_t u) { return __uint_as_float(u); }
__device__ __forceinline__ uint32_t u(float x) { return __float_as_uint(x); }
__device__ __forceinline__ void put3(uint32_t* o, f3 v) { o[0] = u(v.x); o[1] = u(v.y); o[2] = u(v.z); }
__device__ __forceinline__ void put4(uint32_t* o, u4 v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; }

struct RcpNr { static constexpr int WI = 1, WO = 1;
  __device__ static void run(const uint32_t* a, uint32_t* o) { o[0] = u(rcp_nr(f(a[0]))); } };
struct RsqNr { static constexpr int WI = 1, WO = 1;
  __device__ static void run(const uint32_t* a, uint32_t* o) { o[0] = u(rsq_nr(f(a[0]))); } };
struct RsqNr1 { static constexpr int WI = 1, WO = 1;
  __device__ static void run(const uint32_t* a, uint32_t* o) { o[0] = u(rsq_nr1(f(a[0]))); } };
struct RsqNr2 { static constexpr int WI = 1, WO = 1;
  __device__ static void run(const uint32_t* a, uint32_t* o) { o[0] = u(rsq_nr2(f(a[0]))); } };
struct U01 { static constexpr int WI = 1, WO = 1;
  __device__ static void run(const uint32_t* a, uint32_t* o) { o[0] = u(u01(a[0])); } };
struct U16i { static constexpr int WI = 2, WO = 1;
  __device__ static void run(const uint32_t* a, uint32_t* o) { o[0] = u16i(a[0], a[1]); } };
struct U16 { static constexpr int WI = 2, WO = 1;
  __device__ static void run(const uint32_t* a, uint32_t* o) { o[0] = u(u16(a[0], a[1])); } };
struct JitterF { static constexpr int WI = 2, WO = 1;
  __device__ static void run(const uint32_t* a, uint32_t* o) { o[0] = u(jitter_f(a[0], a[1])); } };
struct DiskDir { static constexpr int WI = 1, WO = 2;
  __device__ static void run(const uint32_t* a, uint32_t* o) {
    float c, s;
    disk_dir(a[0], c, s);
    o[0] = u(c); o[1] = u(s);
  } };
// (nl, ra, rb, mode): cosine_vec and the normalize the kernel applies to it (oracle c_cosine);
// mode bit 0 = uniform, bit 1 = unit
template <bool AXIS>
struct Cosine { static constexpr int WI = 6, WO = 3;
  __device__ static void run(const uint32_t* a, uint32_t* o) {
    const bool uniform = (a[5] & 1u) != 0u, unit = (a[5] & 2u) != 0u;
    put3(o, normalize_dir(cosine_vec<AXIS>(mk(f(a[0]), f(a[1]), f(a[2])), a[3], a[4], uniform, unit), unit));
  } };
// (L, inv_spp): scale = inv_spp * 2^31 as the host computes it (exact)
struct Fix31 { static constexpr int WI = 2, WO = 1;
  __device__ static void run(const uint32_t* a, uint32_t* o) { o[0] = fix31(f(a[0]), f(a[1]) * 2147483648.0f); } };
struct Philox { static constexpr int WI = 4, WO = 4;
  __device__ static void run(const uint32_t* a, uint32_t* o) { put4(o, philox4x32(a[0], a[1], a[2], a[3])); } };
// the same counter (pixel, c1, c2, seed) through the per-unit key
struct PhiloxPx { static constexpr int WI = 4, WO = 4;
  __device__ static void run(const uint32_t* a, uint32_t* o) {
    put4(o, philox_px(philox_pixel_key(a[0], a[3]), a[1], a[2]));
  } };
struct Normalize3 { static constexpr int WI = 3, WO = 3;
  __device__ static void run(const uint32_t* a, uint32_t* o) { put3(o, normalize3(mk(f(a[0]), f(a[1]), f(a[2])))); } };
struct Normalize3Free { static constexpr int WI = 3, WO = 3;
  __device__ static void run(const uint32_t* a, uint32_t* o) { put3(o, normalize3_free(mk(f(a[0]), f(a[1]), f(a[2])))); } };

template <typename OP>
__global__ void map_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) OP::run(in + i * OP::WI, out + i * OP::WO);
}

template <typename OP>
int launch(const uint32_t* in, uint32_t* out, long long n, void* stream) {
  if (n <= 0) return 0;
  if (in == nullptr || out == nullptr || n > (1ll << 28)) return (int)hipErrorInvalidValue;
  const hipStream_t s = (hipStream_t)stream;
  const unsigned blocks = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(map_kernel<OP>, dim3(blocks), dim3(256), 0, s, in, out, n);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  return (int)hipStreamSynchronize(s);
}

}  // namespace

#define SPT_PROBE(name, OP)                                                                      \
  extern "C" int spt_probe_##name(const uint32_t* in, uint32_t* out, long long n, void* stream) { \
    return launch<OP>(in, out, n, stream);                                                       \
  }

SPT_PROBE(rcp_nr, RcpNr)
SPT_PROBE(rsq_nr, RsqNr)
SPT_PROBE(rsq_nr1, RsqNr1)
SPT_PROBE(rsq_nr2, RsqNr2)
SPT_PROBE(u01, U01)
SPT_PROBE(u16i, U16i)
SPT_PROBE(u16, U16)
SPT_PROBE(jitter_f, JitterF)
SPT_PROBE(disk_dir, DiskDir)
SPT_PROBE(cosine_axis, Cosine<true>)
SPT_PROBE(cosine_general, Cosine<false>)
SPT_PROBE(fix31, Fix31)
SPT_PROBE(philox4x32, Philox)
SPT_PROBE(philox_px, PhiloxPx)
SPT_PROBE(normalize3, Normalize3)
SPT_PROBE(normalize3_free, Normalize3Free)

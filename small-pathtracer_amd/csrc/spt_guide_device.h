// spt_guide_device.h — the device functions the guide kernel (spt_guide.hip) and the light-guide
// kernel (spt_guide_light.hip) share: the 64-bit cross-lane move of their reductions, the vertex frame
// of a hit and the specular chain's step. Moved here from spt_guide.hip as they stood; the four guide
// kernels' listings did not move (tools/isa_same.py, profiles/r29_guide_light_isa.txt).
//
// The functions below restate blocks of render_kernel (spt_kernel.hip) operation for operation, and
// those blocks cite them back. They are not one function with the render's: every attempt to share
// one moved render_kernel's listings (the sphere variants by up to 17 lines, the generic and wide ones
// by 15 to 17, the wide one sitting at its 80-VGPR limit), and a pull request that leaves the render
// kernels' machine code alone cannot afford that. tools/isa_same.py is the check that it stayed so.
#pragma once
#include <hip/hip_runtime.h>

#include "spt_trace.h"

namespace spt {

__device__ __forceinline__ long long shfl_xor64(long long v, int m) {
  const int lo = __shfl_xor((int)(uint32_t)(unsigned long long)v, m, 64);
  const int hi = __shfl_xor((int)(uint32_t)((unsigned long long)v >> 32), m, 64);
  return (long long)(((unsigned long long)(uint32_t)hi << 32) | (unsigned long long)(uint32_t)lo);
}

// The vertex frame of a hit on H at the trace's t along (o, d): the hit point x, the geometric normal
// gn and the normal nl oriented against the ray. render_kernel's generic shading branch ("plane
// distance as the reference derives it" and "Hitable::normal, oriented against the ray"): a
// rectangle's t corrected (hit_plane_t) for x, a sphere's gn as (x - p) * (1/r).
// POINT: the caller goes on from x (the chain, the light guide's shadow ray). Without it only a
// sphere's normal reads x, and x is formed there alone, from the sphere's own t: the same bits, and a
// rectangle's hit point is not formed at all (formed for every kind, the first-hit pass took 3 to 4 %
// longer than the two-branch kernel's: profiles/r25_guide_bench.json).
struct GuideVertex { f3 x, gn, nl; };
template <bool POINT>
__device__ __forceinline__ GuideVertex guide_vertex(const DevPrim& H, f3 o, f3 d, float ia, float t) {
  GuideVertex V;
  V.x = mk(0, 0, 0);
  if constexpr (POINT) {
    float tr = t;
    if (H.kind == SPT_RECT_XY) tr = hit_plane_t(H.w1 - o.z, d.z, ia, t);
    else if (H.kind == SPT_RECT_XZ) tr = hit_plane_t(H.w1 - o.y, d.y, ia, t);
    else if (H.kind == SPT_RECT_YZ) tr = hit_plane_t(H.w1 - o.x, d.x, ia, t);
    V.x = mk(o.x + d.x * tr, o.y + d.y * tr, o.z + d.z * tr);
  }
  if (H.kind == SPT_RECT_XY) {
    V.nl = d.z < 0.0f ? mk(0, 0, 1) : mk(0, 0, -1);
    V.gn = mk(0, 0, 1);
  } else if (H.kind == SPT_RECT_XZ) {
    V.nl = d.y < 0.0f ? mk(0, 1, 0) : mk(0, -1, 0);
    V.gn = mk(0, 1, 0);
  } else if (H.kind == SPT_RECT_YZ) {
    V.nl = d.x < 0.0f ? mk(1, 0, 0) : mk(-1, 0, 0);
    V.gn = mk(1, 0, 0);
  } else {
    if constexpr (!POINT) V.x = mk(o.x + d.x * t, o.y + d.y * t, o.z + d.z * t);
    V.gn = mk((V.x.x - H.w1) * H.w5, (V.x.y - H.w2) * H.w5, (V.x.z - H.w3) * H.w5);
    V.nl = dot3(V.gn, d) < 0.0f ? V.gn : mk(-V.gn.x, -V.gn.y, -V.gn.z);
  }
  return V;
}

// The chain's step at a SPEC or REFR hit (include/spt.h, SPT_HAS_GUIDE_CHAIN): the throughput
// takes the primitive's colour, the length the segment's t, and (o, d) become the ray the render's path
// takes from here -- render_kernel's block "SPEC :481-482 and REFR :484-495" (oracle c_path), with the
// refraction wherever there is one (no Fresnel draw) and the reflection on total internal reflection.
__device__ __forceinline__ void guide_chain_step(const DevPrim& H, bool unit, f3 x, f3 gn, f3 nl, float t,
                                                 f3& A, float& D, f3& o, f3& d) {
  A = mk(A.x * H.cx, A.y * H.cy, A.z * H.cz);
  D = D + t;
  const float k2 = 2.0f * dot3(gn, d);
  f3 nd = mk(d.x - gn.x * k2, d.y - gn.y * k2, d.z - gn.z * k2);  // reflRay
  if (unit) nd = normalize3(nd);
  if (H.refl == SPT_REFR) {
    const bool into = dot3(gn, nl) > 0.0f;
    const float nnt = into ? 1.0f / 1.5f : 1.5f / 1.0f;
    const float ddn = dot3(d, nl);
    const float cos2t = 1.0f - nnt * nnt * (1.0f - ddn * ddn);
    if (!(cos2t < 0.0f)) {  // else total internal reflection: the reflection above
      const float kk = (into ? 1.0f : -1.0f) * (ddn * nnt + sqrtf(cos2t));
      nd = normalize3(mk(d.x * nnt - gn.x * kk, d.y * nnt - gn.y * kk, d.z * nnt - gn.z * kk));
    }
  }
  o = x;
  d = nd;
}

}  // namespace spt

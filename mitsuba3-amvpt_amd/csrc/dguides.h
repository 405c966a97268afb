/*
 * dguides.h -- the per-element functions of the depth planes (include/amvpt_guides.h).  The kernels of
 * amvpt_guides.hip and its host-only entries call these same functions; everything is unfused float32
 * (-ffp-contract=off, correctly rounded division) and no library function beyond rintf is called, so host and
 * device agree bit for bit.
 *
 * Depth here is PLANAR: the camera-space z of the hit point in the pixel's own view, what a display or a
 * compositor wants.  It is deliberately not the `depth` of the reference's aov integrator
 * (src/integrators/aov.cpp:245-300), which is si.t: a ray parameter measured from the near plane along the
 * ray, which no oracle output pins.
 */
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace amvpt {

#define DHD __host__ __device__ __forceinline__

DHD uint32_t gbits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
DHD float gfloat(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
DHD bool gfinite(float f) { return (gbits(f) & 0x7f800000u) != 0x7f800000u; }
DHD float ginf() { return gfloat(0x7f800000u); }

/* a guide record's hit flag and view index; the view is n_views (out of range) for anything but 0 .. n_views - 1,
 * so that no integer is ever formed from a float outside its range */
DHD bool guide_hit(const float *rec) { return rec[0] >= 0.f; }
DHD uint32_t guide_view(const float *rec, uint32_t n_views) {
    const float v = rec[7];
    return (v >= 0.f && v < (float) n_views) ? (uint32_t) v : n_views;
}

/* z of the record's hit point under row 2 of the view's to_world_inv (m[8 .. 11]), every operation rounded */
DHD float guide_depth_value(const float *rec, const float *row) {
    return ((row[0] * rec[4] + row[1] * rec[5]) + row[2] * rec[6]) + row[3];
}

/* float -> unsigned key with the floats' order (finite values; -0 below +0), and back */
DHD uint32_t depth_key(float f) {
    const uint32_t u = gbits(f);
    return (u & 0x80000000u) ? ~u : u | 0x80000000u;
}
DHD float depth_unkey(uint32_t k) { return gfloat((k & 0x80000000u) ? k & 0x7fffffffu : ~k); }
/* the keys no finite value has: the running minimum and maximum start from them */
constexpr uint32_t kDepthKeyMin0 = 0xffffffffu, kDepthKeyMax0 = 0u;

/* what depth8_value needs of (near, far) */
struct Depth8Params { float far_, span; };   /* span = far - near */

/* nearer is brighter: t = (far - z) / (far - near) clamped to [0, 1], code = rint(255 t), half to even;
 * a z that is not finite (a miss is +inf) gives 0; far == near gives 255 for every finite z */
DHD uint8_t depth8_value(float z, const Depth8Params &P) {
    if (!gfinite(z)) return 0;
    if (P.span == 0.f) return 255;
    float t = (P.far_ - z) / P.span;
    t = t > 0.f ? (t < 1.f ? t : 1.f) : 0.f;   /* a NaN (inf / inf) gives 0 */
    return (uint8_t) rintf(255.f * t);
}

#undef DHD

} // namespace amvpt

/*
 * dpost.h -- the per-pixel primitives the post-process stages share (ddenoise.h, dtemporal.h, dvariance.h, dsynth.h):
 * the finite test, the dot product, the luminance, the a-trous kernel, the two kinds of guide stop, the guide planes
 * in memory and the bilinear footprint of a reprojection.  Host and device: everything is unfused float32
 * (-ffp-contract=off) built from +, -, *, / alone, so both sides agree bit for bit.
 *
 * A helper that reads a plane takes the source object and fetches where its callers always did: a tap stopped by its
 * shape or view fetches nothing else, whichever source serves it.
 */
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace amvpt {

#define PP_HD __host__ __device__ __forceinline__

PP_HD bool pp_finite(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return (u & 0x7f800000u) != 0x7f800000u;
}
PP_HD bool pp_finite3(const float *c) { return pp_finite(c[0]) && pp_finite(c[1]) && pp_finite(c[2]); }
PP_HD float pp_dot(const float *a, const float *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
PP_HD float pp_lum(const float *c) { return (0.2126f * c[0] + 0.7152f * c[1]) + 0.0722f * c[2]; }
/* hk = {1/16, 1/4, 3/8, 1/4, 1/16} at i = -2 .. 2, as selects: no indexed table in registers */
PP_HD float pp_hk(int i) { return i == 0 ? 0.375f : ((i == 1 || i == -1) ? 0.25f : 0.0625f); }
/* floor of a float in [-1, 2^24) by truncation and a correction */
PP_HD int32_t pp_floor(float s) {
    const int32_t i = (int32_t) s;
    return (float) i > s ? i - 1 : i;
}

/* the soft stops: wn * wp of amvpt_denoise between a centre (head g0, normal g0 + 1, hit point p0) and the tap at
 * (qx, qy) with the head g.  The tap's point is fetched here, before wn or after it: kPointFirst says where the caller
 * always fetched it, because the compiler keeps that order and the kernel's registers hang on it */
template <bool kPointFirst, class Src>
PP_HD float pp_guide_weight(const Src &S, int qx, int qy, const float *g0, const float *p0, const float *g, float inv_sp,
                            uint32_t squarings) {
    float pq[3];
    if (kPointFirst) S.point(qx, qy, pq);
    float wn = pp_dot(g0 + 1, g + 1);
    wn = wn > 0.f ? wn : 0.f;
    for (uint32_t i = 0; i < squarings; ++i) wn = wn * wn;
    if (!kPointFirst) S.point(qx, qy, pq);
    const float e[3] = {pq[0] - p0[0], pq[1] - p0[1], pq[2] - p0[2]};
    float t = pp_dot(g0 + 1, e);
    t = (t < 0.f ? -t : t) * inv_sp;
    const float wp = 1.f / (1.f + t * t);
    return wn * wp;
}

/* the hard stops: the normal cosine and the plane distance of a tap with the record q against the pixel's record g */
PP_HD bool pp_same_surface(const float *g, const float *q, float normal_cos, float plane_tol) {
    if (pp_dot(g + 1, q + 1) < normal_cos) return false;
    const float e[3] = {q[4] - g[4], q[5] - g[5], q[6] - g[6]};
    const float t = pp_dot(g + 1, e);
    return !((t < 0.f ? -t : t) > plane_tol);
}

/* the guide records in memory, row-major h x w x 8: what every source in memory starts from */
struct GuidePlanes {
    const float *guides;
    uint32_t w;
    PP_HD size_t at(int x, int y) const { return (size_t) y * w + (size_t) x; }
    PP_HD void head(int x, int y, float g[4]) const {
        const float *r = guides + 8 * at(x, y);
        g[0] = r[0], g[1] = r[1], g[2] = r[2], g[3] = r[3];
    }
    PP_HD float view(int x, int y) const { return guides[8 * at(x, y) + 7]; }
    PP_HD void point(int x, int y, float p[3]) const {
        const float *r = guides + 8 * at(x, y) + 4;
        p[0] = r[0], p[1] = r[1], p[2] = r[2];
    }
    PP_HD float shape(int x, int y) const { return guides[8 * at(x, y)]; }
};

/* the bilinear footprint of a reprojection: the four pixels (x0 + i, y0 + j), i, j = 0, 1, and their weights */
struct Footprint {
    int32_t x0, y0;
    float ax, ay;
    PP_HD float weight(int i, int j) const { return (i ? ax : 1.f - ax) * (j ? ay : 1.f - ay); }
};
/* of the film position (uvx, uvy) inside the tile of tw x th pixels whose first pixel is (tx0, ty0); false when no
 * pixel of the tile is among the four */
PP_HD bool pp_footprint(int32_t tx0, int32_t ty0, int32_t tw, int32_t th, float uvx, float uvy, Footprint &F) {
    const float ftx = (float) tx0, fty = (float) ty0;
    const float fx = ftx + uvx, fy = fty + uvy;
    const float sx = fx - .5f, sy = fy - .5f;
    if (!(sx >= ftx - 1.f && sx < ftx + (float) tw && sy >= fty - 1.f && sy < fty + (float) th)) return false;
    F.x0 = pp_floor(sx), F.y0 = pp_floor(sy);
    F.ax = sx - (float) F.x0, F.ay = sy - (float) F.y0;
    return true;
}

} // namespace amvpt

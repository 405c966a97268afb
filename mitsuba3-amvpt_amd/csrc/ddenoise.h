/*
 * ddenoise.h -- the per-pixel function of the a-trous denoiser (include/amvpt_denoise.h, which holds the normative
 * definition).  The kernels of amvpt_denoise.hip and its host-only entry call this same function; everything is
 * unfused float32 (-ffp-contract=off, correctly rounded division) built from +, -, *, / alone, so host and device
 * agree bit for bit.
 *
 * denoise_pixel reads its planes through a source object, so that one body serves the three places the data can
 * lie: host memory, device memory (DenoisePlanes for both) and the LDS tile of the small-step kernel.  A source has
 *   head(x, y, g)   elements 0..3 of the guide record: shape, normal
 *   view(x, y)      element 7
 *   point(x, y, p)  elements 4..6
 *   color(x, y, c)  RGB of the iteration's input plane
 * and a tap asks for them in this order, so that a tap stopped by its shape or view fetches no colour and no point.
 */
#pragma once
#include "dpost.h"

namespace amvpt {

/* what one iteration needs beyond its planes; the floats are computed once on the host (amvpt_denoise.hip) */
struct DenoiseStep {
    float inv_s2;        /* 1 / sigma_color^2 of this iteration: 4^i / sigma_color^2 */
    float floor2;        /* color_floor * color_floor */
    float inv_sp;        /* 1 / sigma_plane */
    uint32_t squarings;  /* normal_squarings */
    int32_t step;        /* 2^i */
};

/* planes in memory, row-major: image h x w x channels, guides h x w x 8 */
struct DenoisePlanes : GuidePlanes {
    const float *image;
    uint32_t channels;
    PP_HD void color(int x, int y, float c[3]) const {
        const float *r = image + channels * at(x, y);
        c[0] = r[0], c[1] = r[1], c[2] = r[2];
    }
};

/* out = the filtered RGB of pixel (x, y) of a w x h image: one iteration of the definition */
template <class Src>
PP_HD void denoise_pixel(const Src &S, int x, int y, int w, int h, const DenoiseStep &K, float out[3]) {
    float g0[4], c[3], p0[3] = {0.f, 0.f, 0.f};
    S.head(x, y, g0);
    const float v0 = S.view(x, y);
    S.color(x, y, c);
    const bool hit = g0[0] >= 0.f;
    if (hit) S.point(x, y, p0);
    const float m = pp_dot(c, c) + K.floor2;
    const float k = K.inv_s2 / m;
    float sum[3] = {0.f, 0.f, 0.f}, sum_w = 0.f;
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * K.step;
        if (qy < 0 || qy >= h) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * K.step;
            if (qx < 0 || qx >= w) continue;
            float g[4];
            S.head(qx, qy, g);
            if (g[0] != g0[0] || S.view(qx, qy) != v0) continue;   /* another shape (or hit against miss), another view */
            float cq[3];
            S.color(qx, qy, cq);
            if (!pp_finite3(cq)) continue;
            const float d[3] = {cq[0] - c[0], cq[1] - c[1], cq[2] - c[2]};
            const float wc = 1.f / (1.f + pp_dot(d, d) * k);
            float wgt = (pp_hk(dy) * pp_hk(dx)) * wc;
            if (hit) wgt = wgt * pp_guide_weight<false>(S, qx, qy, g0, p0, g, K.inv_sp, K.squarings);
            sum[0] = sum[0] + wgt * cq[0];
            sum[1] = sum[1] + wgt * cq[1];
            sum[2] = sum[2] + wgt * cq[2];
            sum_w = sum_w + wgt;
        }
    }
    const bool ok = sum_w > 0.f;   /* false for the NaN a centre that is not finite leaves */
    out[0] = ok ? sum[0] / sum_w : c[0];
    out[1] = ok ? sum[1] / sum_w : c[1];
    out[2] = ok ? sum[2] / sum_w : c[2];
}

} // namespace amvpt

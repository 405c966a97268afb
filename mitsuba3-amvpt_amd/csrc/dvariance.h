/*
 * dvariance.h -- the per-pixel functions of stages 2 and 3 of the variance-guided denoiser (include/amvpt_variance.h,
 * which holds the normative definition; stage 1 is dtemporal.h's moments instance).  The kernels of
 * amvpt_variance.hip and its host-only entries call these same functions; everything is unfused float32
 * (-ffp-contract=off, correctly rounded division) built from +, -, *, / alone, so host and device agree bit for bit.
 *
 * As in ddenoise.h the functions read their planes through a source object, so that one body serves host memory,
 * device memory (VariancePlanes for both) and the LDS tile of the small-step kernel.  A source has ddenoise.h's
 *   head(x, y, g)   elements 0..3 of the guide record: shape, normal
 *   view(x, y)      element 7
 *   point(x, y, p)  elements 4..6
 *   color(x, y, c)  RGB of the iteration's input plane
 * and, for stage 3,
 *   var(x, y)       the iteration's input variance
 * and a tap asks for them in this order, so that a tap stopped by its shape or view fetches nothing else.  The 3 x 3
 * prefilter of stage 3 reads through a source of its own, which needs no more than
 *   shape(x, y)     element 0
 *   view(x, y)
 *   var(x, y)
 * so that the kernel whose taps go to memory can still keep the prefilter's nine in LDS.
 */
#pragma once
#include "dpost.h"

namespace amvpt {

PP_HD float vr_max0(float x) { return x > 0.f ? x : 0.f; }

/* ---- stage 2 ------------------------------------------------------------------------------------------------------ */

/* what the stage needs beyond its planes; the floats are computed once on the host (amvpt_variance.hip) */
struct VarianceConst {
    float inv_sp;        /* 1 / sigma_plane */
    float min_history;   /* (float) min_history */
    uint32_t squarings;  /* normal_squarings */
};

/* planes in memory, row-major: moments h x w x 2, count h x w, guides h x w x 8.  A source of stage 2 has head, view
 * and point as above, and
 *   count(x, y)        the history count
 *   moments(x, y, m)   the two moments */
struct MomentPlanes : GuidePlanes {
    const float *mom, *cnt;
    PP_HD float count(int x, int y) const { return cnt[at(x, y)]; }
    PP_HD void moments(int x, int y, float m[2]) const {
        const float *r = mom + 2 * at(x, y);
        m[0] = r[0], m[1] = r[1];
    }
};

/* whether pixel (x, y) takes the 7 x 7 window: a usable pixel whose history is shorter than min_history */
template <class Src> PP_HD bool variance_takes_window(const Src &S, int x, int y, const VarianceConst &K) {
    const float n = S.count(x, y);
    float m[2];
    S.moments(x, y, m);
    return n >= 1.f && pp_finite(m[0]) && pp_finite(m[1]) && !(n >= K.min_history);
}

/* the variance of the accumulated luminance of pixel (x, y) of a w x h image */
template <class Src> PP_HD float variance_pixel(const Src &S, int x, int y, int w, int h, const VarianceConst &K) {
    const float n = S.count(x, y);
    float m[2];
    S.moments(x, y, m);
    if (!(n >= 1.f) || !pp_finite(m[0]) || !pp_finite(m[1])) return 0.f;
    const float tv = vr_max0(m[1] - m[0] * m[0]);
    float v = tv;
    if (!(n >= K.min_history)) {
        float g0[4], p0[3] = {0.f, 0.f, 0.f};
        S.head(x, y, g0);
        const float v0 = S.view(x, y);
        const bool hit = g0[0] >= 0.f;
        if (hit) S.point(x, y, p0);
        float s1 = 0.f, s2 = 0.f, sw = 0.f;
        for (int dy = -3; dy <= 3; ++dy) {
            const int qy = y + dy;
            if (qy < 0 || qy >= h) continue;
            for (int dx = -3; dx <= 3; ++dx) {
                const int qx = x + dx;
                if (qx < 0 || qx >= w) continue;
                float g[4];
                S.head(qx, qy, g);
                if (g[0] != g0[0] || S.view(qx, qy) != v0) continue;
                if (!(S.count(qx, qy) >= 1.f)) continue;
                float mq[2];
                S.moments(qx, qy, mq);
                if (!pp_finite(mq[0]) || !pp_finite(mq[1])) continue;
                float wgt = 1.f;
                if (hit) wgt = pp_guide_weight<true>(S, qx, qy, g0, p0, g, K.inv_sp, K.squarings);
                s1 = s1 + wgt * mq[0];
                s2 = s2 + wgt * mq[1];
                sw = sw + wgt;
            }
        }
        const float r = K.min_history / n;
        if (sw > 0.f) {
            const float e1 = s1 / sw, e2 = s2 / sw;
            v = vr_max0(e2 - e1 * e1) * r;
        } else {
            v = tv * r;
        }
    }
    return v / n;
}

/* ---- stage 3 ------------------------------------------------------------------------------------------------------ */

/* what one iteration needs beyond its planes; the floats are computed once on the host (amvpt_variance.hip) */
struct VarianceStep {
    float sl2;           /* sigma_lum * sigma_lum */
    float var_floor;
    float inv_sp;        /* 1 / sigma_plane */
    uint32_t squarings;  /* normal_squarings */
    int32_t step;        /* 2^i */
};

/* planes in memory, row-major: image h x w x channels, variance h x w, guides h x w x 8 */
struct VariancePlanes : GuidePlanes {
    const float *image, *variance;
    uint32_t channels;
    PP_HD void color(int x, int y, float c[3]) const {
        const float *r = image + channels * at(x, y);
        c[0] = r[0], c[1] = r[1], c[2] = r[2];
    }
    PP_HD float var(int x, int y) const { return variance[at(x, y)]; }
};

/* gk = {1/4, 1/2, 1/4} at i = -1 .. 1 */
PP_HD float vr_gk(int i) { return i == 0 ? 0.5f : 0.25f; }

/* gv of pixel (x, y), whose shape and view are shape0 and v0: the 3 x 3 prefilter of the input variance at step 1 */
template <class Pre> PP_HD float variance_prefilter(const Pre &S, int x, int y, int w, int h, float shape0, float v0) {
    float sg = 0.f, sk = 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int qy = y + dy;
        if (qy < 0 || qy >= h) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx;
            if (qx < 0 || qx >= w) continue;
            if (S.shape(qx, qy) != shape0 || S.view(qx, qy) != v0) continue;
            const float vq = S.var(qx, qy);
            if (!pp_finite(vq)) continue;
            const float kw = vr_gk(dy) * vr_gk(dx);
            sg = sg + kw * vq;
            sk = sk + kw;
        }
    }
    return sk > 0.f ? sg / sk : 0.f;
}

/* out = the filtered RGB of pixel (x, y) of a w x h image and vout its filtered variance: one iteration.  S serves the
 * 25 taps, P the prefilter */
template <class Src, class Pre>
PP_HD void denoise_variance_pixel(const Src &S, const Pre &P, int x, int y, int w, int h, const VarianceStep &K, float out[3],
                                float &vout) {
    float g0[4], c[3], p0[3] = {0.f, 0.f, 0.f};
    S.head(x, y, g0);
    const float v0 = S.view(x, y);
    S.color(x, y, c);
    const bool hit = g0[0] >= 0.f;
    if (hit) S.point(x, y, p0);
    const float gv = variance_prefilter(P, x, y, w, h, g0[0], v0);
    const float lp = pp_lum(c);
    const float kl = 1.f / (K.sl2 * gv + K.var_floor);
    float sum[3] = {0.f, 0.f, 0.f}, sum_w = 0.f, sum_v = 0.f;
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
            if (!pp_finite(cq[0]) || !pp_finite(cq[1]) || !pp_finite(cq[2])) continue;
            const float vq = S.var(qx, qy);
            if (!pp_finite(vq)) continue;
            const float dl = pp_lum(cq) - lp;
            const float wl = 1.f / (1.f + (dl * dl) * kl);
            float wgt = (pp_hk(dy) * pp_hk(dx)) * wl;
            if (hit) wgt = wgt * pp_guide_weight<true>(S, qx, qy, g0, p0, g, K.inv_sp, K.squarings);
            sum[0] = sum[0] + wgt * cq[0];
            sum[1] = sum[1] + wgt * cq[1];
            sum[2] = sum[2] + wgt * cq[2];
            sum_w = sum_w + wgt;
            sum_v = sum_v + (wgt * wgt) * vq;
        }
    }
    const bool ok = sum_w > 0.f;   /* false for the NaN a centre that is not finite leaves */
    out[0] = ok ? sum[0] / sum_w : c[0];
    out[1] = ok ? sum[1] / sum_w : c[1];
    out[2] = ok ? sum[2] / sum_w : c[2];
    vout = ok ? sum_v / (sum_w * sum_w) : S.var(x, y);
}

} // namespace amvpt

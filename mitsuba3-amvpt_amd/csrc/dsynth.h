/*
 * dsynth.h -- the per-pixel functions of the view synthesis (include/amvpt_synth.h, which holds the normative
 * definition): synth_pixel is stage 1, the cross-view gather, and synth_fill_pixel one iteration of stage 2, the hole
 * fill.  The kernels of amvpt_synth.hip and its host-only entries call these same functions.  Weights, sums and stops
 * are unfused float32 (-ffp-contract=off, correctly rounded division and square root); the projection and the tile layout
 * are dtemporal.h's, the hard stops and the bilinear footprint dpost.h's.  Host and device agree bit for bit.
 *
 * A tap fetches its fields in the order of the stops: the guide record (two 16-byte halves), then the colour -- a tap
 * stopped by its view or shape fetches no colour.  The loop over the source views is uniform across a wave, and the
 * device reads src_views[s] through the constant address space: once per wave with scalar loads, not once per lane.
 */
#pragma once
#include "dtemporal.h"

namespace amvpt {

struct SynthArgs {
    const float *src_image, *src_guides, *dst_guides;
    const amvpt_view_desc *src_views;   /* ns views: host memory for the host entry, the upload for the kernel */
    const float *dst_origins;           /* three floats per target view: (m[3], m[7], m[11]) of its to_world */
    float *dst_image, *dst_cover;
    uint32_t channels;
    TemporalLayout S, D;                /* S: the whole source quilt; D: the target quilt and the rectangle */
    float plane_tol, normal_cos, view_falloff;
    uint32_t tiles_x;                   /* blocks per row of the launch */
};

struct SynthFillArgs {
    const float *in, *cover_in, *guides;
    float *out, *cover_out;
    uint32_t channels, w, h, tiles_x;
    int32_t step;
    float plane_tol, normal_cos;
};

/* source view s, the same for every lane of the wave: what the projection reads and the camera's origin */
PP_HD TemporalView sy_fetch_view(const amvpt_view_desc *views, uint32_t s, float O[3]) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(4))) const amvpt_view_desc uniform_view;
    const uint32_t s0 = (uint32_t) __builtin_amdgcn_readfirstlane((int) s);
    uniform_view &U = *(uniform_view *) (uintptr_t) (views + s0);
#else
    const amvpt_view_desc &U = views[s];
#endif
    O[0] = U.to_world[3], O[1] = U.to_world[7], O[2] = U.to_world[11];
    return tp_view(U);
}

PP_HD bool sy_finite(const float *c, uint32_t channels) {
    return pp_finite(c[0]) && pp_finite(c[1]) && pp_finite(c[2]) && (channels != 4u || pp_finite(c[3]));
}

/* stage 1, pixel (lx, ly) of the target rectangle: colour and cover */
PP_HD void synth_pixel(const SynthArgs &A, int32_t lx, int32_t ly) {
    const TemporalLayout &S = A.S, &D = A.D;
    const uint32_t C = A.channels;
    const size_t at = (size_t) ly * (size_t) D.rw + (size_t) lx;
    const float *r = A.dst_guides + 8 * at;
    const float g[8] = {r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]};
    float *o = A.dst_image + C * at;
    const uint32_t nd = D.multisensor ? D.n_views : 1u, ns = S.multisensor ? S.n_views : 1u;
    float sw = 0.f, sc[4] = {0.f, 0.f, 0.f, 0.f};
    bool ok = g[7] >= 0.f && g[7] < (float) nd;
    uint32_t t = 0;
    int32_t px = 0, py = 0;   /* the pixel's position inside target tile t */
    if (ok) {
        t = (uint32_t) g[7];
        int32_t dx0, dy0;
        tp_tile(D, t, dx0, dy0);
        px = lx + D.rx0 - dx0, py = ly + D.ry0 - dy0;
        ok = px >= 0 && px < D.tw && py >= 0 && py < D.th;
    }
    if (ok && g[0] >= 0.f) {
        const float *Ot = A.dst_origins + 3 * (size_t) t;
        const float dt[3] = {Ot[0] - g[4], Ot[1] - g[5], Ot[2] - g[6]};
        const float lt = __builtin_sqrtf(pp_dot(dt, dt));
        for (uint32_t s = 0; s < ns; ++s) {
            float Os[3], uvx, uvy;
            const TemporalView V = sy_fetch_view(A.src_views, s, Os);
            if (!tp_project(V, g + 4, uvx, uvy)) continue;
            const float ds[3] = {Os[0] - g[4], Os[1] - g[5], Os[2] - g[6]};
            const float ls = __builtin_sqrtf(pp_dot(ds, ds));
            const float d = lt * ls;
            float wv = 1.f;
            if (d > 0.f) {
                const float c = pp_dot(dt, ds) / d;
                float a = 1.f - c;
                a = a > 0.f ? a : 0.f;
                wv = 1.f / (1.f + a * A.view_falloff);
            }
            int32_t tx0, ty0;
            tp_tile(S, s, tx0, ty0);
            Footprint F;
            if (!pp_footprint(tx0, ty0, S.tw, S.th, uvx, uvy, F)) continue;
            const float fs = (float) s;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int32_t qy = F.y0 + j;
                if (qy < ty0 || qy >= ty0 + S.th) continue;
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int32_t qx = F.x0 + i;
                    if (qx < tx0 || qx >= tx0 + S.tw) continue;
                    const size_t qa = (size_t) qy * (size_t) S.rw + (size_t) qx;
                    const float *rq = A.src_guides + 8 * qa;
                    const float q[8] = {rq[0], rq[1], rq[2], rq[3], rq[4], rq[5], rq[6], rq[7]};
                    if (q[7] != fs || q[0] != g[0]) continue;
                    const float *cq = A.src_image + C * qa;
                    const float col[4] = {cq[0], cq[1], cq[2], C == 4u ? cq[3] : 0.f};
                    if (!sy_finite(col, C)) continue;
                    if (!pp_same_surface(g, q, A.normal_cos, A.plane_tol)) continue;
                    const float w = F.weight(i, j) * wv;
                    sw = sw + w;
                    sc[0] = sc[0] + w * col[0];
                    sc[1] = sc[1] + w * col[1];
                    sc[2] = sc[2] + w * col[2];
                    sc[3] = sc[3] + w * col[3];
                }
            }
        }
    } else if (ok && g[0] < 0.f) {
        const int32_t mx = (int32_t) (((int64_t) px * S.tw) / D.tw), my = (int32_t) (((int64_t) py * S.th) / D.th);
        const int32_t ox = mx < S.tw - 1 ? mx : S.tw - 1, oy = my < S.th - 1 ? my : S.th - 1;
        for (uint32_t s = 0; s < ns; ++s) {
            int32_t tx0, ty0;
            tp_tile(S, s, tx0, ty0);
            const size_t qa = (size_t) (ty0 + oy) * (size_t) S.rw + (size_t) (tx0 + ox);
            const float *rq = A.src_guides + 8 * qa;
            if (!(rq[0] < 0.f) || rq[7] != (float) s) continue;
            const float *cq = A.src_image + C * qa;
            const float col[4] = {cq[0], cq[1], cq[2], C == 4u ? cq[3] : 0.f};
            if (!sy_finite(col, C)) continue;
            sw = sw + 1.f;
            sc[0] = sc[0] + 1.f * col[0];
            sc[1] = sc[1] + 1.f * col[1];
            sc[2] = sc[2] + 1.f * col[2];
            sc[3] = sc[3] + 1.f * col[3];
        }
    }
    if (sw > 0.f) {
        o[0] = sc[0] / sw, o[1] = sc[1] / sw, o[2] = sc[2] / sw;
        if (C == 4u) o[3] = sc[3] / sw;
        A.dst_cover[at] = sw;
    } else {
        o[0] = 0.f, o[1] = 0.f, o[2] = 0.f;
        if (C == 4u) o[3] = 0.f;
        A.dst_cover[at] = 0.f;
    }
}

/* stage 2, one iteration at pixel (x, y) */
PP_HD void synth_fill_pixel(const SynthFillArgs &A, int32_t x, int32_t y) {
    const uint32_t C = A.channels;
    const size_t at = (size_t) y * (size_t) A.w + (size_t) x;
    float *o = A.out + C * at;
    const float c = A.cover_in[at];
    if (!(c == 0.f)) {
        const float *ci = A.in + C * at;
        o[0] = ci[0], o[1] = ci[1], o[2] = ci[2];
        if (C == 4u) o[3] = ci[3];
        A.cover_out[at] = c;
        return;
    }
    const float *r = A.guides + 8 * at;
    const float g[8] = {r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]};
    const bool hit = g[0] >= 0.f;
    float sw = 0.f, sc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int dy = -2; dy <= 2; ++dy) {
        const int32_t qy = y + dy * A.step;
        if (qy < 0 || qy >= (int32_t) A.h) continue;
        for (int dx = -2; dx <= 2; ++dx) {
            const int32_t qx = x + dx * A.step;
            if (qx < 0 || qx >= (int32_t) A.w) continue;
            const size_t qa = (size_t) qy * (size_t) A.w + (size_t) qx;
            const float *rq = A.guides + 8 * qa;
            const float q7 = rq[7], q0 = rq[0];
            if (q7 != g[7] || q0 != g[0]) continue;
            if (!(A.cover_in[qa] > 0.f)) continue;
            const float *cq = A.in + C * qa;
            const float col[4] = {cq[0], cq[1], cq[2], C == 4u ? cq[3] : 0.f};
            if (!sy_finite(col, C)) continue;
            if (hit) {
                const float q[8] = {q0, rq[1], rq[2], rq[3], rq[4], rq[5], rq[6], q7};
                if (!pp_same_surface(g, q, A.normal_cos, A.plane_tol)) continue;
            }
            const float w = pp_hk(dy) * pp_hk(dx);
            sw = sw + w;
            sc[0] = sc[0] + w * col[0];
            sc[1] = sc[1] + w * col[1];
            sc[2] = sc[2] + w * col[2];
            sc[3] = sc[3] + w * col[3];
        }
    }
    if (sw > 0.f) {
        o[0] = sc[0] / sw, o[1] = sc[1] / sw, o[2] = sc[2] / sw;
        if (C == 4u) o[3] = sc[3] / sw;
        A.cover_out[at] = -1.f;
    } else {
        o[0] = 0.f, o[1] = 0.f, o[2] = 0.f;
        if (C == 4u) o[3] = 0.f;
        A.cover_out[at] = 0.f;
    }
}

} // namespace amvpt

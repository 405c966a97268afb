/*
 * dtemporal.h -- the per-pixel function of the temporal accumulation (include/amvpt_temporal.h, which holds the
 * normative definition).  The kernel of amvpt_temporal.hip and its host-only entry call this same function.  The
 * blend, the weights and the stops are unfused float32 (-ffp-contract=off, correctly rounded division and square
 * root); the projection restates camera_uv of amvpt_render.hip operation by operation, with the explicit fused
 * multiply-adds of xf_point / xf_point_affine (dmath.h), so that a hit point projected into the view it was traced
 * from lands in its own pixel.  Host and device agree bit for bit.
 *
 * A tap fetches its fields in the order of the stops: the guide record (two 16-byte halves), then the count, then
 * the colour -- a tap stopped by its view or shape fetches neither count nor colour.
 *
 * The function has two instances, chosen by the type of its arguments: TemporalArgs is amvpt_temporal, and
 * TemporalMomentsArgs is amvpt_temporal_moments (include/amvpt_variance.h), which carries the two luminance moments
 * through the same accepted taps and fetches a tap's moments last, once every stop has passed.  Everything the
 * moments add sits behind `if constexpr`, so the first instance compiles to what it was without them.
 */
#pragma once
#include "../../include/amvpt.h"
#include "dpost.h"

namespace amvpt {

/* the quilt's tiles (amvpt_temporal.h "Layout") and the rectangle the planes hold */
struct TemporalLayout {
    uint32_t multisensor, batch, n_views, gx, gy, rev_x, rev_y;
    int32_t tw, th;
    int32_t rx0, ry0, rw, rh;
};

struct TemporalArgs {
    const float *image, *guides, *hist_image, *hist_guides, *hist_count;
    const amvpt_view_desc *views;   /* the previous views: host memory for the host entry, the upload for the kernel */
    float *out_image, *out_count;
    uint32_t channels;
    TemporalLayout L;
    float max_history, plane_tol, normal_cos;
    uint32_t tiles_x;               /* blocks per row of the launch */
};

/* amvpt_temporal_moments: the same, with the h x w x 2 planes of the luminance moments */
struct TemporalMomentsArgs : TemporalArgs {
    const float *hist_moments;
    float *out_moments;
};
template <class Args> struct tp_moments { static constexpr bool value = false; };
template <> struct tp_moments<TemporalMomentsArgs> { static constexpr bool value = true; };

PP_HD float tp_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
/* row r of a Transform4f applied to the point q: the terms of xf_point / xf_point_affine */
PP_HD float tp_row(const float *m, int r, const float *q) {
    return tp_fma(m[4 * r + 2], q[2], tp_fma(m[4 * r + 1], q[1], tp_fma(m[4 * r], q[0], m[4 * r + 3])));
}

/* the fields of a view the projection reads */
struct TemporalView {
    float to_world_inv[12], camera_to_sample[16];
    float near_clip, far_clip, resolution[2], pp_offset[2], aperture_radius, focus_distance;
    uint32_t type;
};
template <class VT> PP_HD TemporalView tp_view(const VT &V) {
    TemporalView T;
    for (int i = 0; i < 12; ++i) T.to_world_inv[i] = V.to_world_inv[i];
    for (int i = 0; i < 16; ++i) T.camera_to_sample[i] = V.camera_to_sample[i];
    T.near_clip = V.near_clip, T.far_clip = V.far_clip;
    T.resolution[0] = V.resolution[0], T.resolution[1] = V.resolution[1];
    T.pp_offset[0] = V.pp_offset[0], T.pp_offset[1] = V.pp_offset[1];
    T.aperture_radius = V.aperture_radius, T.focus_distance = V.focus_distance;
    T.type = V.type;
    return T;
}

/* camera_uv(V, P, .5, .5): false when the camera-space z is outside the clip range or not above 0 */
PP_HD bool tp_project(const TemporalView &V, const float *P, float &uvx, float &uvy) {
    const float ref[3] = {tp_row(V.to_world_inv, 0, P), tp_row(V.to_world_inv, 1, P), tp_row(V.to_world_inv, 2, P)};
    if (!(ref[2] >= V.near_clip && ref[2] <= V.far_clip && ref[2] > 0.f)) return false;
    const float *s = V.camera_to_sample;
    if (V.type == AMVPT_CAMERA_THINLENS) {
        /* thin_uv: disk_concentric(.5, .5) is (0, 0) */
        const float a[3] = {0.f * V.aperture_radius, 0.f * V.aperture_radius, 0.f};
        float l[3] = {ref[0] - a[0], ref[1] - a[1], ref[2] - a[2]};
        const float dist = __builtin_sqrtf(tp_fma(l[2], l[2], tp_fma(l[1], l[1], l[0] * l[0])));
        const float inv_dist = 1.0f / dist;
        l[0] = l[0] * inv_dist, l[1] = l[1] * inv_dist, l[2] = l[2] * inv_dist;
        const float inv_f = 1.f / V.focus_distance;
        const float f[3] = {a[0] * inv_f + l[0] / l[2], a[1] * inv_f + l[1] / l[2], a[2] * inv_f + l[2] / l[2]};
        uvx = tp_row(s, 0, f) * V.resolution[0];
        uvy = tp_row(s, 1, f) * V.resolution[1];
    } else {
        /* persp_uv: xf_point divides by the fourth row */
        const float d = tp_row(s, 3, ref);
        uvx = (tp_row(s, 0, ref) / d - V.pp_offset[0]) * V.resolution[0];
        uvy = (tp_row(s, 1, ref) / d - V.pp_offset[1]) * V.resolution[1];
    }
    return true;
}

/* view v of the table.  On the device a wave whose lanes all ask for one view (a wave is two rows of 32 pixels: every
 * wave of a quilt whose tile width is a multiple of 32) fetches it once with scalar loads instead of once per lane */
PP_HD TemporalView tp_fetch_view(const amvpt_view_desc *views, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t v0 = (uint32_t) __builtin_amdgcn_readfirstlane((int) v);
    if (__ballot(v != v0) == 0ull) {
        typedef __attribute__((address_space(4))) const amvpt_view_desc uniform_view;
        return tp_view(*(uniform_view *) (uintptr_t) (views + v0));
    }
#endif
    return tp_view(views[v]);
}

/* the first pixel of view v's tile, in quilt pixels */
PP_HD void tp_tile(const TemporalLayout &L, uint32_t v, int32_t &tx0, int32_t &ty0) {
    uint32_t col = 0, row = 0;
    if (L.multisensor) {
        if (L.batch) col = L.rev_x ? L.n_views - 1u - v : v;
        else {
            col = v % L.gx, row = v / L.gx;
            if (L.rev_x) col = L.gx - 1u - col;
            if (L.rev_y) row = L.gy - 1u - row;
        }
    }
    tx0 = (int32_t) col * L.tw, ty0 = (int32_t) row * L.th;
}

/* the history of a hit pixel: the four taps around its reprojection; n_prev = 0 when nothing is accepted.  hm: the
 * history of the moments (the moments instance alone) */
template <class Args> PP_HD float tp_gather(const Args &A, const float *g, float h[3], float hm[2]) {
    constexpr bool kMoments = tp_moments<Args>::value;
    const TemporalLayout &L = A.L;
    const uint32_t nv = L.multisensor ? L.n_views : 1u;
    if (!(g[7] >= 0.f && g[7] < (float) nv)) return 0.f;
    const uint32_t v = (uint32_t) g[7];
    float uvx, uvy;
    const TemporalView V = tp_fetch_view(A.views, v);
    if (!tp_project(V, g + 4, uvx, uvy)) return 0.f;
    int32_t tx0, ty0;
    tp_tile(L, v, tx0, ty0);
    Footprint F;
    if (!pp_footprint(tx0, ty0, L.tw, L.th, uvx, uvy, F)) return 0.f;
    float sw = 0.f, sn = 0.f, sc[3] = {0.f, 0.f, 0.f};
    float n_lo = __builtin_huge_valf(), n_hi = 0.f;   /* the range of the accepted counts */
    float sm[2] = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int32_t qy = F.y0 + j;
        if (qy < ty0 || qy >= ty0 + L.th || qy < L.ry0 || qy >= L.ry0 + L.rh) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int32_t qx = F.x0 + i;
            if (qx < tx0 || qx >= tx0 + L.tw || qx < L.rx0 || qx >= L.rx0 + L.rw) continue;
            const size_t at = (size_t) (qy - L.ry0) * (size_t) L.rw + (size_t) (qx - L.rx0);
            const float *r = A.hist_guides + 8 * at;
            const float q[8] = {r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]};
            if (q[7] != g[7] || q[0] != g[0]) continue;
            const float cnt = A.hist_count[at];
            if (!(cnt >= 1.f)) continue;
            const float *hc = A.hist_image + A.channels * at;
            const float col[3] = {hc[0], hc[1], hc[2]};
            if (!pp_finite3(col)) continue;
            if (!pp_same_surface(g, q, A.normal_cos, A.plane_tol)) continue;
            const float w = F.weight(i, j);
            sw = sw + w;
            sc[0] = sc[0] + w * col[0];
            sc[1] = sc[1] + w * col[1];
            sc[2] = sc[2] + w * col[2];
            sn = sn + w * cnt;
            if constexpr (kMoments) {
                const float *mq = A.hist_moments + 2 * at;
                sm[0] = sm[0] + w * mq[0];
                sm[1] = sm[1] + w * mq[1];
            }
            n_lo = cnt < n_lo ? cnt : n_lo;
            n_hi = cnt > n_hi ? cnt : n_hi;
        }
    }
    if (!(sw > 0.f)) return 0.f;
    h[0] = sc[0] / sw, h[1] = sc[1] / sw, h[2] = sc[2] / sw;
    if constexpr (kMoments) hm[0] = sm[0] / sw, hm[1] = sm[1] / sw;
    /* a weighted mean lies in the range of its terms; rounding alone can take the quotient out of it */
    const float n = sn / sw;
    return n < n_lo ? n_lo : (n > n_hi ? n_hi : n);
}

/* pixel (lx, ly) of the rectangle: both outputs, and with the moments instance the third */
template <class Args> PP_HD void temporal_pixel(const Args &A, int32_t lx, int32_t ly) {
    constexpr bool kMoments = tp_moments<Args>::value;
    const size_t at = (size_t) ly * (size_t) A.L.rw + (size_t) lx;
    const float *cp = A.image + A.channels * at;
    const float c[3] = {cp[0], cp[1], cp[2]};
    float *o = A.out_image + A.channels * at;
    if (A.channels == 4u) o[3] = cp[3];
    if (!pp_finite3(c)) {
        o[0] = c[0], o[1] = c[1], o[2] = c[2];
        A.out_count[at] = 0.f;
        if constexpr (kMoments) A.out_moments[2 * at] = 0.f, A.out_moments[2 * at + 1] = 0.f;
        return;
    }
    float m[2] = {0.f, 0.f}, hm[2] = {0.f, 0.f};
    if constexpr (kMoments) {
        const float l = pp_lum(c);
        m[0] = l, m[1] = l * l;
    }
    const float *r = A.guides + 8 * at;
    const float g[8] = {r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]};
    float h[3] = {0.f, 0.f, 0.f}, n_prev = 0.f;
    if (g[0] < 0.f) {
        const float *hg = A.hist_guides + 8 * at;
        if (hg[0] < 0.f && hg[7] == g[7]) {
            const float cnt = A.hist_count[at];
            if (cnt >= 1.f) {
                const float *hc = A.hist_image + A.channels * at;
                const float col[3] = {hc[0], hc[1], hc[2]};
                if (pp_finite3(col)) {
                    h[0] = col[0], h[1] = col[1], h[2] = col[2], n_prev = cnt;
                    if constexpr (kMoments) hm[0] = A.hist_moments[2 * at], hm[1] = A.hist_moments[2 * at + 1];
                }
            }
        }
    } else {
        n_prev = tp_gather(A, g, h, hm);
    }
    if (n_prev > 0.f) {
        float n = n_prev + 1.f;
        n = n < A.max_history ? n : A.max_history;
        const float a = 1.f / n;
        o[0] = h[0] + a * (c[0] - h[0]);
        o[1] = h[1] + a * (c[1] - h[1]);
        o[2] = h[2] + a * (c[2] - h[2]);
        A.out_count[at] = n;
        if constexpr (kMoments) {
            A.out_moments[2 * at] = hm[0] + a * (m[0] - hm[0]);
            A.out_moments[2 * at + 1] = hm[1] + a * (m[1] - hm[1]);
        }
    } else {
        o[0] = c[0], o[1] = c[1], o[2] = c[2];
        A.out_count[at] = 1.f;
        if constexpr (kMoments) A.out_moments[2 * at] = m[0], A.out_moments[2 * at + 1] = m[1];
    }
}

} // namespace amvpt

/*
 * amvpt_variance.h -- the variance-guided denoiser of libamvpt_hip.so, in three stages: temporal accumulation that
 * also carries the first and second moment of luminance through the history (amvpt_temporal_moments), the variance
 * of the accumulated luminance from those moments (amvpt_variance), and an a-trous filter whose luminance stop is
 * as wide as that variance says the noise is (amvpt_denoise_variance).  amvpt_denoise weighs colour differences
 * against the centre pixel's magnitude and smooths a converged image as hard as a 1-spp one; this filter converges
 * to its input as the variance falls.
 *
 * The reference has none of this.  The scheme is that of Schied et al., "Spatiotemporal Variance-Guided Filtering"
 * (HPG 2017): temporal luminance moments, a spatial estimate where the history is short, a 3 x 3 prefilter of the
 * variance, and the variance filtered along with the colour.  The stops are those of amvpt_denoise.h and
 * amvpt_temporal.h (shape, normal, plane, view).  All weights are rational, 1 / (1 + x): no transcendental function.
 *
 * These are new entry points only: no struct of amvpt.h changes, AMVPT_ABI_VERSION stays as it is, amvpt_temporal
 * and amvpt_denoise keep their definitions, and this header carries a version of its own.  Status codes and
 * amvpt_last_error() are amvpt.h's.
 *
 * THE DEFINITION (normative).  Every operation is rounded on its own in float32 (no fused multiply-add, correctly
 * rounded division), except inside the projection of stage 1, which is amvpt_temporal's.  Dot products are formed
 * as (a.x*b.x + a.y*b.y) + a.z*b.z, and lum(c) = (0.2126f*c.r + 0.7152f*c.g) + 0.0722f*c.b.  max(0, x) is
 * x > 0 ? x : 0 (a NaN gives 0).  "finite" is neither NaN nor an infinity.  Device entry and host entry of each stage
 * are compiled from the same per-pixel code and agree bit for bit.  Guide records have amvpt_guides' layout
 * ([0] shape or -1, [1..3] normal n, [4..6] hit point pos, [7] view).
 *
 * STAGE 1, amvpt_temporal_moments: amvpt_temporal (amvpt_temporal.h) with two more planes, hist_moments in and
 * out_moments out, both h x w x 2 float32 over the same rectangle.  out_image and out_count are amvpt_temporal's,
 * bit for bit, for every input: the tap selection, the weights w, sw, h, n_prev, n and a below are its own, and the
 * moments change none of them.  With c the current colour of pixel p:
 *
 *   current       l = lum(c), m = (l, l*l)
 *   centre not finite   (any RGB of c) out_moments = (0, 0); out_count is 0 there
 *   miss          where amvpt_temporal accepts the history pixel: hm = hist_moments[p]
 *   hit           sm from (0, 0), in tap order over the accepted taps q: sm.k = sm.k + w * hist_moments[q].k for
 *                 k = 0, 1; a tap's moments are not examined: one that is not finite makes hm not finite.
 *                 If sw > 0: hm = sm / sw per component
 *   blend         n_prev > 0:  out_moments.k = hm.k + a * (m.k - hm.k)
 *                 otherwise:   out_moments = m
 *
 * STAGE 2, amvpt_variance: moments (h x w x 2), count (h x w) and guide records (h x w x 8) of a plain rectangle
 * to one float per pixel, the variance of the ACCUMULATED luminance (the variance of one frame's luminance over the
 * history length).  It needs no layout: the view of a pixel is guides[..][7].  With (M1, M2) = moments[p]:
 *
 *   n = count[p].  If n >= 1 does not hold (a NaN too), or M1 or M2 is not finite: var = 0.
 *   tv = max(0, M2 - M1*M1)
 *   n >= (float) min_history:  v = tv
 *   otherwise     the 7 x 7 window q = p + (dx, dy), dy = -3..3 the outer loop and dx = -3..3 the inner one (the
 *                 summation order).  A tap is skipped when q is outside the image, or guides[q][7] != guides[p][7],
 *                 or guides[q][0] != guides[p][0], or count[q] >= 1 does not hold, or a moment of q is not finite.
 *                 Its weight w is 1 on a miss (guides[p][0] < 0) and wn*wp on a hit, with amvpt_denoise's
 *                   wn = max(0, n_p.n_q) squared normal_squarings times;  e = pos_q - pos_p;
 *                   t = |n_p.e| * inv_sp;  wp = 1.f / (1.f + t*t);  inv_sp = 1.f / sigma_plane (host, once)
 *                 sums from 0: s1 = s1 + w*M1_q, s2 = s2 + w*M2_q, sw = sw + w.
 *                 r = (float) min_history / n.
 *                 If sw > 0:  e1 = s1/sw, e2 = s2/sw, v = max(0, e2 - e1*e1) * r.
 *                 Otherwise (the centre's own weight is 0 or NaN: a degenerate normal or hit point):  v = tv * r.
 *   var = v / n
 *
 * STAGE 3, amvpt_denoise_variance: a developed image (h x w x C, C = 3 or 4), a variance plane (h x w) and guide
 * records to the filtered image and, where asked for, the filtered variance.  Iteration i = 0 .. iterations-1 uses
 * the step s = 2^i, reads a colour plane `in` and a variance plane `vin` (the inputs for i = 0, the previous
 * iteration's outputs after it) and writes `out` and `vout`:
 *
 *   constants   inv_sp = 1.f / sigma_plane;  sl2 = sigma_lum*sigma_lum  (host, once)
 *   prefilter   over the 3 x 3 q = p + (dx, dy) at step 1 in every iteration, dy = -1..1 outer, dx = -1..1 inner,
 *               gk = {1/4, 1/2, 1/4}: a tap is skipped when q is outside the image, or of another view or shape
 *               (guides[q][7] != guides[p][7] or guides[q][0] != guides[p][0]), or vin[q] is not finite;
 *               from 0: sg = sg + (gk[dy]*gk[dx]) * vin[q], sk = sk + gk[dy]*gk[dx];  gv = sk > 0 ? sg / sk : 0
 *   centre      l_p = lum(in[p]);  kl = 1.f / (sl2 * gv + var_floor)
 *   taps        the 25 taps q = p + s*(dx, dy) of amvpt_denoise in its order (dy = -2..2 outer, dx = -2..2 inner),
 *               hk = {1/16, 1/4, 3/8, 1/4, 1/16}, with its skip rules (outside the image, another view, another
 *               shape, an RGB of in[q] not finite) and its wn and wp (stage 2 restates them); a tap whose vin[q]
 *               is not finite is skipped too
 *   weight      dl = lum(in[q]) - l_p;  wl = 1.f / (1.f + (dl*dl)*kl);  w = (hk[dy]*hk[dx]) * wl;
 *               on a hit (guides[p][0] >= 0)  w = ((hk[dy]*hk[dx]) * wl) * (wn*wp)
 *   sums        from 0: sum_c = sum_c + w*in[q] per channel, sum_w = sum_w + w, sum_v = sum_v + (w*w)*vin[q]
 *   output      where sum_w > 0:  out[p] = sum_c / sum_w per channel, vout[p] = sum_v / (sum_w*sum_w);
 *               else out[p] = in[p], vout[p] = vin[p].  With C = 4 alpha is the input image's, unchanged, in every
 *               iteration.
 *
 * The variance plane is expected to be at least 0 wherever it is finite, as stage 2 writes it and as every iteration
 * keeps it; with a negative variance kl can be infinite or negative, and nothing below is promised.
 *
 * What follows: inputs are only read; a pixel whose centre colour is not finite passes through unchanged, colour and
 * variance, and contaminates nothing.  A pixel whose own variance is not finite contaminates nothing either, but does
 * not pass through: its own tap is skipped like any other, so its colour and its variance are filtered from its
 * accepted neighbours (both finite), and only where sum_w > 0 does not hold -- no neighbour accepted -- do in[p] and the
 * vin[p] that is not finite come out.  An image holding one power-of-two value per (view, shape) region comes out
 * exactly equal, whatever a variance plane of values that are at least 0 or not finite holds (dl = 0 makes wl = 1, kl
 * being finite); with an all-zero variance plane the luminance stop is as narrow as var_floor, and the filter returns
 * its input to within that.  No tap of any stage crosses a view, so a rectangle of whole tiles gives that part of
 * the whole result.
 */
#ifndef AMVPT_VARIANCE_H
#define AMVPT_VARIANCE_H

#include "amvpt.h"
#include "amvpt_temporal.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AMVPT_VARIANCE_VERSION 1

typedef struct amvpt_variance_params {
    uint32_t iterations;        /* 1 .. 8; iteration i of stage 3 uses step s = 2^i */
    float    sigma_lum;         /* > 0: the luminance stop, in standard deviations of the accumulated luminance */
    float    var_floor;         /* > 0: added to the scaled variance, in squared luminance */
    float    sigma_plane;       /* > 0, world units, as amvpt_denoise's */
    uint32_t normal_squarings;  /* 0 .. 7: the normal weight is max(0, n.n')^(2^k) */
    uint32_t min_history;       /* 1 .. 65535: below it stage 2 estimates the variance from the 7 x 7 window */
} amvpt_variance_params;

uint32_t amvpt_variance_version(void);

/* {4, 2.0, 1e-8, 0.05, 5, 4}; sigma_plane is in world units: scale it to the scene, as for amvpt_denoise. */
amvpt_variance_params amvpt_variance_default_params(void);

/*
 * Stage 1 over device pointers.  Everything amvpt_temporal.h says of amvpt_temporal holds: one kernel launch ordered
 * on `stream`, `params` for the layout, `rect`, the view table's upload pair, the refusals.  It adds: a null
 * hist_moments or out_moments; out_moments overlapping any input or another output; out_image or out_count
 * overlapping hist_moments.
 */
amvpt_status amvpt_temporal_moments(const float *image_device, uint32_t channels, const float *guides_device,
                                    const float *hist_image_device, const float *hist_guides_device,
                                    const float *hist_count_device, const float *hist_moments_device,
                                    const amvpt_view_desc *prev_views, const amvpt_params *params, const uint32_t rect[4],
                                    const amvpt_temporal_params *tp, float *out_image_device, float *out_count_device,
                                    float *out_moments_device, void *stream);

amvpt_status amvpt_temporal_moments_host(const float *image, uint32_t channels, const float *guides, const float *hist_image,
                                         const float *hist_guides, const float *hist_count, const float *hist_moments,
                                         const amvpt_view_desc *prev_views, const amvpt_params *params, const uint32_t rect[4],
                                         const amvpt_temporal_params *tp, float *out_image, float *out_count,
                                         float *out_moments);

/*
 * Stage 2 over device pointers: one kernel launch ordered on `stream`; nothing allocated, no device-wide
 * synchronisation.  Of `params` it reads sigma_plane, normal_squarings and min_history, and checks all of them.
 * AMVPT_ERR_INVALID, naming the argument: a null pointer; a dimension of 0 or above 2^31 - 256, or more than 2^31
 * tiles of 32 x 8 pixels; a parameter outside the ranges above or not finite; out overlapping an input.
 */
amvpt_status amvpt_variance(const float *moments_device, const float *count_device, const float *guides_device,
                            uint32_t width, uint32_t height, const amvpt_variance_params *params, float *out_device,
                            void *stream);

amvpt_status amvpt_variance_host(const float *moments, const float *count, const float *guides, uint32_t width,
                                 uint32_t height, const amvpt_variance_params *params, float *out);

/*
 * Stage 3 over device pointers, one kernel launch per iteration, ordered on `stream`; nothing allocated, no
 * device-wide synchronisation.  out and scratch (the image's size) take turns so that the last iteration lands in
 * out, and so do var_out and var_scratch (height x width float32) for the variance.  scratch and var_scratch may be
 * NULL when iterations == 1; var_out may be NULL when iterations <= 2, and then the last iteration's variance is not
 * written.
 * AMVPT_ERR_INVALID, naming the argument: a null pointer; channels not 3 or 4; a dimension as for stage 2; a parameter
 * outside the ranges above or not finite; out, scratch, var_out or var_scratch overlapping the image, the variance, the
 * guides or each other.
 */
amvpt_status amvpt_denoise_variance(const float *image_device, uint32_t channels, uint32_t width, uint32_t height,
                                    const float *variance_device, const float *guides_device,
                                    const amvpt_variance_params *params, float *out_device, float *scratch_device,
                                    float *var_out_device, float *var_scratch_device, void *stream);

/* The host entries run the same functions over host pointers, compiled for the host from the same per-pixel code:
 * they need no device and never return AMVPT_ERR_NO_DEVICE. */
amvpt_status amvpt_denoise_variance_host(const float *image, uint32_t channels, uint32_t width, uint32_t height,
                                         const float *variance, const float *guides, const amvpt_variance_params *params,
                                         float *out, float *scratch, float *var_out, float *var_scratch);

#ifdef __cplusplus
}
#endif

#endif /* AMVPT_VARIANCE_H */

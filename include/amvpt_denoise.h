/*
 * amvpt_denoise.h -- the denoiser of libamvpt_hip.so: an edge-avoiding a-trous wavelet filter over a developed
 * quilt, stopped by the guide buffers of amvpt_guides.h (shape, geometric normal, hit point, view).
 *
 * The reference has no denoiser and no guide buffers for mvpath (see amvpt_guides.h); the filter is the a-trous
 * scheme of Dammertz et al., "Edge-Avoiding A-Trous Wavelet Transform for fast Global Illumination Filtering"
 * (HPG 2010), with the stops this project's structure gives it: reflectance is constant per shape (no textures),
 * so a hard stop on the shape index does what albedo demodulation does elsewhere, and the view index is an exact
 * stop at quilt tile borders: the filter never mixes two views.  A view-group rank may therefore filter the
 * rectangle of its own whole tiles and gets the single-process result.
 *
 * These are new entry points only: no struct of amvpt.h changes, AMVPT_ABI_VERSION stays as it is and this header
 * carries a version of its own.  Status codes and amvpt_last_error() are amvpt.h's.
 *
 * THE DEFINITION (normative).  Every operation is rounded on its own in float32 (no fused multiply-add, correctly
 * rounded division); dot products are formed as (a.x*b.x + a.y*b.y) + a.z*b.z.  Device entry and host entry are
 * compiled from the same per-pixel code and agree bit for bit.
 *
 * Inputs: a developed image, h x w x C float32 with C = 3 or 4 (what amvpt_develop writes); the guide records of
 * the same rectangle, h x w x 8 float32 in amvpt_guides' layout ([0] shape or -1, [1..3] normal n, [4..6] hit
 * point pos, [7] view); the parameters below.  Iteration i = 0 .. iterations-1 uses the step s = 2^i, reads a
 * colour plane `in` (the image for i = 0, the previous iteration's output after it) and writes `out`:
 *
 *   constants   inv_s2_0 = 1.f / (sigma_color*sigma_color), inv_s2_i = 4 * inv_s2_(i-1) (the colour sigma halves
 *               per iteration), inv_sp = 1.f / sigma_plane, computed once on the host
 *   centre p    c = RGB of in at p;  m = ((c.r*c.r + c.g*c.g) + c.b*c.b) + color_floor*color_floor;  k = inv_s2_i / m
 *   taps        q = p + s*(dx, dy), dy = -2..2 the outer loop and dx = -2..2 the inner one (the summation order),
 *               hk = {1/16, 1/4, 3/8, 1/4, 1/16}
 *   skipped     (weight 0) when q is outside the image, or any RGB of in at q is not finite, or
 *               guides[q][7] != guides[p][7] (another view), or guides[q][0] != guides[p][0] (another shape, or
 *               hit against miss)
 *   weight      d = in[q] - c per channel;  d2 = (d.r*d.r + d.g*d.g) + d.b*d.b;  wc = 1.f / (1.f + d2*k);
 *               w = (hk[dy]*hk[dx]) * wc
 *   on a hit    (guides[p][0] >= 0)  wn = max(0, n_p.n_q) squared normal_squarings times;  e = pos_q - pos_p;
 *               t = |n_p.e| * inv_sp;  wp = 1.f / (1.f + t*t);  w = ((hk[dy]*hk[dx]) * wc) * (wn*wp)
 *   sums        sum_c += w * in[q] per channel, sum_w += w
 *   output      out[p] = sum_c / sum_w per channel where sum_w > 0, else in[p] unchanged (a centre that is not
 *               finite); with C = 4 alpha is the input image's, unchanged, in every iteration
 *
 * What follows: the image and the guides are only read; a pixel whose centre colour is not finite passes through
 * unchanged and contaminates nothing; an image holding one power-of-two value per (view, shape) region comes out
 * exactly equal.  Image edges are handled by the "outside the image" rule, not by clamping.
 */
#ifndef AMVPT_DENOISE_H
#define AMVPT_DENOISE_H

#include "amvpt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AMVPT_DENOISE_VERSION 1

typedef struct amvpt_denoise_params {
    uint32_t iterations;        /* 1 .. 8; iteration i uses step s = 2^i */
    float    sigma_color;       /* > 0, relative to the centre pixel's magnitude */
    float    color_floor;       /* > 0 */
    float    sigma_plane;       /* > 0, world units */
    uint32_t normal_squarings;  /* 0 .. 7: the normal weight is max(0, n.n')^(2^k) */
} amvpt_denoise_params;

uint32_t amvpt_denoise_version(void);

/* {3, 1.0, 0.01, 0.05, 5}; 0.05 is 1/40 of the Cornell box's width.  sigma_plane is in world units: scale it to
 * the scene (the Python layer takes 1/40 of the largest side of the hit points' bounding box). */
amvpt_denoise_params amvpt_denoise_default_params(void);

/*
 * The filter over device pointers, one kernel launch per iteration, ordered on `stream`.  out and scratch (both of
 * the image's size, height x width x channels float32) take turns so that the last iteration lands in out; scratch
 * may be NULL when iterations == 1.  The call allocates nothing and uses no device-wide synchronisation.
 * AMVPT_ERR_INVALID, naming the argument: a null pointer; channels not 3 or 4; a dimension of 0; a parameter
 * outside the ranges above or not finite; out or scratch overlapping the image, the guides or each other.
 */
amvpt_status amvpt_denoise(const float *image_device, uint32_t channels, uint32_t width, uint32_t height,
                           const float *guides_device, const amvpt_denoise_params *params, float *out_device,
                           float *scratch_device, void *stream);

/* The same function over host pointers, compiled for the host from the same per-pixel code: it needs no device and
 * never returns AMVPT_ERR_NO_DEVICE. */
amvpt_status amvpt_denoise_host(const float *image, uint32_t channels, uint32_t width, uint32_t height,
                                const float *guides, const amvpt_denoise_params *params, float *out, float *scratch);

#ifdef __cplusplus
}
#endif

#endif /* AMVPT_DENOISE_H */

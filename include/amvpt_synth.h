/*
 * amvpt_synth.h -- view synthesis of libamvpt_hip.so: the views of a dense quilt made from the rendered views of a
 * sparse one, without tracing a path.  A lenticular preset wants several dozen views and a path-traced view is by far
 * the most expensive step of the pipeline; the surface point behind every pixel of any view, on the other hand, costs
 * one primary-hit pass (amvpt_guides.h), and a diffuse surface point has the same radiance from every camera.  A stage
 * of its own between the denoiser and the sRGB quilt of amvpt_display.h.
 *
 * The reference has no view synthesis and no guide buffers for mvpath (see amvpt_guides.h).  The scheme is the backward
 * (gather) form of depth-image-based rendering: where McMillan's forward warp ("An Image-Based Approach to Three-
 * Dimensional Computer Graphics", 1997) scatters source pixels and needs a depth test, here the target view's own
 * guide record gives the surface point of every target pixel, the point is projected into every source view with the
 * projection of amvpt_temporal.h, and that header's stops (view, shape, normal, plane) decide whether a source pixel
 * sees the same point: they are the occlusion test.  The blend over the source views is the angular weight of
 * Buehler et al., "Unstructured Lumigraph Rendering" (SIGGRAPH 2001), reduced to one falloff.  Holes, points no source
 * view sees, are filled from covered pixels of the same view and shape with the a-trous taps of amvpt_denoise.h.
 *
 * Both stages are pure gathers: no forward warp, no scatter, no atomics and no summation order that varies.  These are
 * new entry points only: no struct of amvpt.h changes, AMVPT_ABI_VERSION stays as it is and this header carries a
 * version of its own.  Status codes and amvpt_last_error() are amvpt.h's.
 *
 * THE DEFINITION (normative).  Every operation is rounded on its own in float32 (no fused multiply-add, correctly
 * rounded division and square root), except inside the projection, which is amvpt_temporal.h's "projection" unchanged.
 * Dots are (a.x*b.x + a.y*b.y) + a.z*b.z.  "finite" means an exponent field that is not all ones.  Guide records have
 * amvpt_guides' layout: [0] shape or -1, [1..3] normal, [4..6] hit point, [7] view.  Device entry and host entry are
 * compiled from the same per-pixel code and agree bit for bit.
 *
 * STAGE 1, amvpt_synth.  The source quilt is src_image (Hs x Ws x C, C = 3 or 4), src_guides (Hs x Ws x 8) and the
 * ns views src_views; the target quilt is dst_guides (h x w x 8 over `rect`) and the nd views dst_views.  Each quilt
 * has the layout of amvpt_temporal.h "Layout", from src_params and dst_params (tw_s x th_s and tw_d x th_d tiles); ns
 * and nd count as 1 when the quilt's multisensor is 0.  The source planes always hold the whole source quilt; the
 * target planes hold `rect` alone.  Alpha is gathered like a colour channel.
 *
 * Target pixel p = (x, y) of the target quilt has the record g.
 *
 *   bad view            unless 0 <= g[7] < nd every channel is 0 and the cover is 0.  Otherwise t = (uint32_t) g[7];
 *                       (lx, ly) = (x - tile_x0(t), y - tile_y0(t)) in the target layout, and unless 0 <= lx < tw_d and
 *                       0 <= ly < th_d (a record that does not belong to this layout) the outputs are 0 as well.
 *   sums                sw = 0 and sc[k] = 0 for k < C.
 *   hit (g[0] >= 0)     P = g[4..6], n_p = g[1..3].  With m = dst_views[t].to_world, O_t = (m[3], m[7], m[11]);
 *                       dt = O_t - P, lt = sqrt(dot(dt, dt)).
 *                       For s = 0 .. ns-1 (the outer loop and the summation order), V = src_views[s]:
 *     projection        amvpt_temporal.h "projection" of P through V -> (uvx, uvy); rejected: the next s.
 *     view weight       O_s from V.to_world as above, ds = O_s - P, ls = sqrt(dot(ds, ds)), d = lt * ls.  If d > 0:
 *                       c = dot(dt, ds) / d, a = 1.f - c, a = a > 0 ? a : 0, wv = 1.f / (1.f + a * view_falloff).
 *                       Otherwise wv = 1.
 *     position, taps    amvpt_temporal.h "position" and "taps" in the tile of view s of the SOURCE layout: fx, fy, sx,
 *                       sy, the reject test, x0, y0, ax, ay; q = (x0+i, y0+j), j outer and i inner, bilinear weight
 *                       w_b = (i ? ax : 1-ax) * (j ? ay : 1-ay).
 *     skipped           when q is outside the tile of s, or src_guides[q][7] != (float) s, or src_guides[q][0] != g[0],
 *                       or one of the C channels of src_image[q] is not finite, or dot(n_p, n_q) < normal_cos, or
 *                       |dot(n_p, pos_q - P)| > plane_tol.
 *     accepted          w = w_b * wv, sw = sw + w, sc[k] = sc[k] + w * src_image[q][k].
 *   miss (g[0] < 0)     the only environment emitter is `constant`: a miss has the same radiance from any camera.  For
 *                       s = 0 .. ns-1 the source pixel is q = (tile_x0(s) + min(tw_s - 1, (lx * tw_s) / tw_d),
 *                       tile_y0(s) + min(th_s - 1, (ly * th_s) / th_d)) in integer arithmetic.  It is accepted when
 *                       src_guides[q][0] < 0, src_guides[q][7] == (float) s and all C channels are finite; then
 *                       sw = sw + 1.f, sc[k] = sc[k] + 1.f * src_image[q][k].
 *   output              sw > 0: dst_image[p][k] = sc[k] / sw, dst_cover[p] = sw.  Otherwise every channel and the cover
 *                       are 0: a hole.
 *
 * What follows: the inputs are only read; a source pixel that is not finite contaminates nothing; no target pixel
 * depends on another, so the stage over a rectangle of whole target tiles gives that part of the whole result; the
 * result depends on the source quilt only through the taps named above; weights are never negative, so where the
 * source image holds one power of two per shape, every covered target pixel comes out within 1 ulp of that colour
 * (the quotient sc / sw of two rounded sums).
 *
 * STAGE 2, amvpt_synth_fill, over the planes of a plain h x w rectangle of the TARGET quilt; the view of a pixel is
 * guides[..][7].  Iteration i = 0 .. fill_iterations-1 has the step s = 2^i; out / scratch and cover_out /
 * cover_scratch take turns so that the last iteration lands in out and cover_out (iteration i writes the scratch pair
 * when fill_iterations-1-i is odd).  With fill_iterations == 0, out and cover_out are copies of the inputs.
 * Per iteration and pixel p with the record g and c = cover_in[p]:
 *
 *   covered or filled   unless c == 0 holds, colour and cover pass through unchanged (a NaN cover too).
 *   hole                the 25 taps q = p + s * (dx, dy), dy = -2 .. 2 the outer loop and dx = -2 .. 2 the inner one
 *                       (amvpt_denoise.h's order), hk = {1/16, 1/4, 3/8, 1/4, 1/16}.
 *     skipped           when q is outside the image, or guides[q][7] != g[7], or guides[q][0] != g[0], or
 *                       cover_in[q] > 0 does not hold (a filled pixel carries -1: it is never a source, errors do not
 *                       spread), or one of the C channels of in[q] is not finite, or, where g[0] >= 0,
 *                       dot(n_p, n_q) < normal_cos or |dot(n_p, pos_q - pos_p)| > plane_tol.
 *     accepted          w = hk[dy] * hk[dx], sw = sw + w, sc[k] = sc[k] + w * in[q][k], sums from 0.
 *     output            sw > 0: out[p][k] = sc[k] / sw, cover_out[p] = -1.f.  Otherwise every channel and the cover are 0.
 *
 * After the stage a cover above 0 means gathered, -1 filled, 0 still a hole.  A pixel whose cover is not 0 is never
 * changed, and a filled pixel is never read as a source.
 */
#ifndef AMVPT_SYNTH_H
#define AMVPT_SYNTH_H

#include "amvpt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AMVPT_SYNTH_VERSION 1

typedef struct amvpt_synth_params {
    float    plane_tol;       /* > 0, world units: as amvpt_temporal_params */
    float    normal_cos;      /* -1 .. 1: as amvpt_temporal_params */
    float    view_falloff;    /* >= 0, finite: a source view whose direction to the hit point differs from the target's by
                                 1 - cos = 1 / view_falloff weighs half; 0: all views alike */
    uint32_t fill_iterations; /* 0 .. 8: iterations of amvpt_synth_fill; amvpt_synth does not read it beyond its range */
} amvpt_synth_params;

uint32_t amvpt_synth_version(void);

/* {0.02, 0.9, 1e5, 4}; plane_tol is in world units (1/100 of the Cornell box's width): scale it to the scene.
 * view_falloff: of 0, 1000 and 1e5 the last is the best on rough conductors and no worse on diffuse walls (DESIGN.md,
 * "View synthesis"): the nearest source views carry nearly all the weight. */
amvpt_synth_params amvpt_synth_default_params(void);

/*
 * Stage 1 over device pointers: one kernel launch, ordered on `stream`.  src_params and dst_params give the two layouts
 * only (film size, grid, reverse, batch, multisensor, n_views).  rect = {x0, y0, w, h} in pixels of the target quilt,
 * made of whole target tiles; NULL: all of it.  dst_guides, dst_image (h x w x channels) and dst_cover (h x w) hold the
 * rectangle alone; src_image and src_guides hold the whole source quilt.  src_views and dst_views are HOST pointers to
 * the ns and nd views of the two quilts.
 *
 * The call allocates nothing beyond the upload of the view tables: the ns source views and the nd target origins
 * (three floats each) travel in one block of ns x sizeof(amvpt_view_desc) + 12 nd bytes, through a device buffer with a
 * pinned host block beside it that the library keeps for reuse, exactly as amvpt_temporal.h describes for its own
 * upload (the same code over a pool of this entry's own: an event behind each launch, polled, never waited for; both
 * tables are copied out of the caller's memory before the call returns; no device-wide synchronisation; the kept pairs
 * are never freed, and a call that has to allocate cannot be captured into a graph).
 *
 * AMVPT_ERR_INVALID, naming the argument: a null pointer; channels not 3 or 4; a film dimension of 0 or above 2^24; a
 * parameter outside the ranges above or not finite; more than 64 source views; a rectangle of zero area, outside the
 * target film or not made of whole target tiles; an output overlapping any input or the other output.
 * AMVPT_ERR_UNSUPPORTED, for either layout: a crop window (crop_offset_* nonzero, or full_* set and different from the
 * film); a film size the grid does not divide; a grid with n_views != grid_x * grid_y.
 * A refused call writes nothing.
 */
amvpt_status amvpt_synth(const float *src_image_device, uint32_t channels, const float *src_guides_device,
                         const amvpt_view_desc *src_views, const amvpt_params *src_params,
                         const float *dst_guides_device, const amvpt_view_desc *dst_views,
                         const amvpt_params *dst_params, const uint32_t rect[4], const amvpt_synth_params *sp,
                         float *dst_image_device, float *dst_cover_device, void *stream);

/* The same function over host pointers, compiled for the host from the same per-pixel code: it needs no device and
 * never returns AMVPT_ERR_NO_DEVICE. */
amvpt_status amvpt_synth_host(const float *src_image, uint32_t channels, const float *src_guides,
                              const amvpt_view_desc *src_views, const amvpt_params *src_params, const float *dst_guides,
                              const amvpt_view_desc *dst_views, const amvpt_params *dst_params, const uint32_t rect[4],
                              const amvpt_synth_params *sp, float *dst_image, float *dst_cover);

/*
 * Stage 2 over device pointers: sp->fill_iterations launches (or, with 0, two copies) ordered on `stream`; nothing is
 * allocated.  image and out are height x width x channels, cover and cover_out height x width, guides height x width
 * x 8.  scratch (the image's size) and cover_scratch (the cover's) may be NULL only when fill_iterations is at most 1;
 * out and cover_out never.
 *
 * AMVPT_ERR_INVALID, naming the argument: a null pointer; channels not 3 or 4; a width or height of 0 or above
 * 2^31 - 256; a parameter outside the ranges above; an output or scratch plane overlapping an input or another of them.
 */
amvpt_status amvpt_synth_fill(const float *image_device, uint32_t channels, uint32_t width, uint32_t height,
                              const float *cover_device, const float *guides_device, const amvpt_synth_params *sp,
                              float *out_device, float *scratch_device, float *cover_out_device,
                              float *cover_scratch_device, void *stream);

amvpt_status amvpt_synth_fill_host(const float *image, uint32_t channels, uint32_t width, uint32_t height,
                                   const float *cover, const float *guides, const amvpt_synth_params *sp, float *out,
                                   float *scratch, float *cover_out, float *cover_scratch);

#ifdef __cplusplus
}
#endif

#endif /* AMVPT_SYNTH_H */

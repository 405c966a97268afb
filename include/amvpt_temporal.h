/*
 * amvpt_temporal.h -- temporal accumulation of libamvpt_hip.so: the previous frame's accumulated quilt, reprojected
 * through the guide buffers of amvpt_guides.h into the current frame and blended with it.  A stage of its own between
 * amvpt_develop and amvpt_denoise: at the sample counts an interactive quilt affords the previous frame is the
 * cheapest source of samples, and the camera of a light-field viewer moves little from frame to frame.
 *
 * The reference has no temporal stage and no guide buffers for mvpath (see amvpt_guides.h).  The scheme is the
 * backward reprojection of Nehab et al., "Accelerating Real-Time Shading with Reverse Reprojection Caching" (Graphics
 * Hardware 2007), with the history length of Schied et al., "Spatiotemporal Variance-Guided Filtering" (HPG 2017), and
 * the stops this project's structure gives it: the shape index (reflectance is constant per shape), the geometric
 * normal, the plane through the hit point, and the view index, an exact stop at quilt tile borders: no tap crosses a
 * view.  Scenes are static; only the camera moves.
 *
 * It is a pure gather: each output pixel reads at most four history pixels.  No scatter, no atomics and no summation
 * order that varies.  The caller keeps three planes from one frame to the next and swaps them itself: the accumulated
 * image, the guide records it was accumulated with, and the per-pixel history count (one float).
 *
 * These are new entry points only: no struct of amvpt.h changes, AMVPT_ABI_VERSION stays as it is and this header
 * carries a version of its own.  Status codes and amvpt_last_error() are amvpt.h's.
 *
 * THE DEFINITION (normative).  Every operation is rounded on its own in float32 (no fused multiply-add, correctly
 * rounded division and square root), except inside the projection, which repeats the render's camera_uv and with it
 * the fused multiply-adds of its transforms, named below.  Device entry and host entry are compiled from the same
 * per-pixel code and agree bit for bit.
 *
 * Layout, from `params` (the inverse of the render's sensor index):
 *   multisensor == 0   one tile, the whole film: tw = film_width, th = film_height, n_views counts as 1
 *   batch              tw = film_width / n_views, th = film_height; the tile column of view v is
 *                      reverse_x ? n_views-1-v : v, its row 0
 *   grid               tw = film_width / grid_x, th = film_height / grid_y; view v sits at column
 *                      reverse_x ? grid_x-1-(v % grid_x) : v % grid_x and at row reverse_y ? grid_y-1-(v / grid_x) : v / grid_x
 *   tile_x0 = column * tw, tile_y0 = row * th
 *
 * Pixel p = (x, y) has the current record g (amvpt_guides' layout: [0] shape or -1, [1..3] normal n_p, [4..6] hit
 * point P, [7] view) and the current colour c.
 *
 *   centre not finite   any RGB of c not finite: out = c, count = 0.  Such a pixel contaminates nothing.
 *   miss (g[0] < 0)     the history pixel is the same (x, y).  It is accepted when hist_guides[p][0] < 0 and
 *                       hist_guides[p][7] == g[7] (a miss of the same view), hist_count[p] >= 1 and the RGB of
 *                       hist_image[p] is finite; then h = hist_image[p], n_prev = hist_count[p].  Otherwise n_prev = 0.
 *                       (The only environment emitter is `constant`: a miss has the same radiance from any camera.)
 *   hit                 n_prev = 0 unless 0 <= g[7] < n_views; v = (uint32_t) g[7], V = prev_views[v].
 *     projection        the render's camera_uv at the aperture sample (.5, .5), with fma(a, b, c) = a*b + c rounded once:
 *                         row(m, r, q)  = fma(m[4r+2], q.z, fma(m[4r+1], q.y, fma(m[4r], q.x, m[4r+3])))
 *                         ref           = (row(V.to_world_inv, 0, P), row(.., 1, P), row(.., 2, P))
 *                         rejected (n_prev = 0) unless ref.z >= V.near_clip, ref.z <= V.far_clip and ref.z > 0
 *                         perspective   s = V.camera_to_sample;  d = row(s, 3, ref);
 *                                       uvx = (row(s, 0, ref) / d - V.pp_offset[0]) * V.resolution[0], uvy alike from row 1
 *                         thin lens     the aperture point is a = (0 * aperture_radius, 0 * aperture_radius, 0);
 *                                       l = ref - a;  dist = sqrt(fma(l.z, l.z, fma(l.y, l.y, l.x*l.x)));
 *                                       l = l * (1 / dist);  inv_f = 1 / focus_distance;
 *                                       f = (a.x*inv_f + l.x/l.z, a.y*inv_f + l.y/l.z, a.z*inv_f + l.z/l.z);
 *                                       uvx = row(s, 0, f) * V.resolution[0], uvy = row(s, 1, f) * V.resolution[1]
 *     position          fx = tile_x0 + uvx, fy = tile_y0 + uvy, sx = fx - .5f, sy = fy - .5f.  Rejected unless
 *                       sx >= tile_x0 - 1 && sx < tile_x0 + tw && sy >= tile_y0 - 1 && sy < tile_y0 + th (float
 *                       comparisons before any conversion: a NaN rejects).  x0 = floor(sx), y0 = floor(sy), formed by
 *                       truncation and a correction; ax = sx - x0, ay = sy - y0.
 *     taps              q = (x0+i, y0+j), j = 0, 1 the outer loop and i = 0, 1 the inner one (the summation order);
 *                       w = (i ? ax : 1-ax) * (j ? ay : 1-ay)
 *     skipped           when q is outside the tile of v (which also keeps it inside the image) or outside `rect`, or
 *                       hist_guides[q][7] != g[7], or hist_guides[q][0] != g[0], or hist_count[q] >= 1 does not hold
 *                       (a NaN count is skipped), or an RGB of hist_image[q] is not finite, or
 *                       dot(n_p, n_q) < normal_cos, or |dot(n_p, pos_q - P)| > plane_tol, with dots formed as
 *                       (a.x*b.x + a.y*b.y) + a.z*b.z
 *     sums              from 0, in tap order: sw += w, sc += w * hist_image[q] per channel, sn += w * hist_count[q].
 *                       If sw > 0: h = sc / sw per channel and n_prev = sn / sw, clamped to [lo, hi], the least and the
 *                       greatest accepted hist_count[q] (n < lo ? lo : n > hi ? hi : n; a weighted mean lies there,
 *                       and rounding alone can take the quotient out: with equal counts n_prev is that count, so a
 *                       static camera counts its frames in whole numbers).  Otherwise n_prev = 0.
 *   blend               n = min(n_prev + 1, (float) max_history), a = 1.f / n.
 *                       n_prev > 0:  out = h + a * (c - h) per RGB channel, out_count = n.
 *                       otherwise:   out = c, out_count = 1.
 *                       With C = 4, alpha is the current image's, unchanged.
 *
 * What follows: with an all-zero history count the output is the current image, bit for bit, with count 1
 * everywhere; the inputs are only read; no tap crosses a view, so a view-group rank may run the stage over the
 * rectangle of its own whole tiles (`rect`) and gets that part of the single-process result.
 */
#ifndef AMVPT_TEMPORAL_H
#define AMVPT_TEMPORAL_H

#include "amvpt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AMVPT_TEMPORAL_VERSION 1

typedef struct amvpt_temporal_params {
    uint32_t max_history;   /* 1 .. 65535: the weight of a new frame never falls below 1/max_history */
    float    plane_tol;     /* > 0, world units: |n_p . (pos_q - pos_p)| above it rejects a tap */
    float    normal_cos;    /* -1 .. 1: n_p . n_q below it rejects a tap */
} amvpt_temporal_params;

uint32_t amvpt_temporal_version(void);

/* {32, 0.02, 0.9}; 0.02 is 1/100 of the Cornell box's width.  plane_tol is in world units: scale it to the scene. */
amvpt_temporal_params amvpt_temporal_default_params(void);

/*
 * The stage over device pointers: one kernel launch, ordered on `stream`.  `params` gives the layout only (film size,
 * grid, reverse, batch, multisensor, n_views).  rect = {x0, y0, w, h} in pixels of the quilt, made of whole tiles;
 * NULL: all of it.  Every plane holds the rectangle alone, row-major: the current developed image and the outputs of
 * the previous call (h x w x C with C = 3 or 4, h x w x 8 guide records, h x w x 1 counts).  prev_views is a HOST
 * pointer to the n_views views the history was rendered with.
 *
 * The call allocates nothing beyond the upload of that view table, n_views x sizeof(amvpt_view_desc) bytes.  The upload
 * lives in a device buffer with a pinned host block beside it, which the library keeps for reuse: allocated (hipMalloc
 * and hipHostMalloc, whole 4 KiB) when the device has no kept pair that is large enough and whose earlier call has
 * finished -- an event behind each launch tells, polled, never waited for.  The table is copied out of prev_views into
 * the pinned block before the call returns, whatever memory prev_views is in; from there it goes to the device in
 * stream order.  There is no device-wide synchronisation.
 * Limits: the kept pairs are never freed, and there are as many as calls were ever enqueued at once (a caller that
 * queues many frames without synchronising grows them by 8 KiB and one event a frame); a call that has to allocate
 * cannot be captured into a graph.
 *
 * AMVPT_ERR_INVALID, naming the argument: a null pointer; channels not 3 or 4; a film dimension of 0 or above 2^24;
 * a parameter outside the ranges above or not finite; a rectangle of zero area, outside the film or not made of whole
 * tiles; an output overlapping any input or the other output.
 * AMVPT_ERR_UNSUPPORTED: a crop window (crop_offset_* nonzero, or full_* set and different from the film); a film size
 * the grid does not divide; a grid with n_views != grid_x * grid_y.
 */
amvpt_status amvpt_temporal(const float *image_device, uint32_t channels, const float *guides_device,
                            const float *hist_image_device, const float *hist_guides_device,
                            const float *hist_count_device, const amvpt_view_desc *prev_views,
                            const amvpt_params *params, const uint32_t rect[4], const amvpt_temporal_params *tp,
                            float *out_image_device, float *out_count_device, void *stream);

/* The same function over host pointers, compiled for the host from the same per-pixel code: it needs no device and
 * never returns AMVPT_ERR_NO_DEVICE. */
amvpt_status amvpt_temporal_host(const float *image, uint32_t channels, const float *guides, const float *hist_image,
                                 const float *hist_guides, const float *hist_count, const amvpt_view_desc *prev_views,
                                 const amvpt_params *params, const uint32_t rect[4], const amvpt_temporal_params *tp,
                                 float *out_image, float *out_count);

#ifdef __cplusplus
}
#endif

#endif /* AMVPT_TEMPORAL_H */

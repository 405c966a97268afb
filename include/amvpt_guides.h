/*
 * amvpt_guides.h -- guide buffers of libamvpt_hip.so: what every quilt pixel sees (surface, normal, position,
 * view), the planar depth of it, and that depth as an 8-bit quilt for RGB-D displays.
 *
 * Reference interfaces replaced (file:line in xacond00/mitsuba3-amvpt):
 *   amvpt_guides <- the aov integrator's `shape_index`, `geo_normal`, `position` (src/integrators/aov.cpp:245-300),
 *                   which cannot be combined with mvpath (mvpath.cpp:45-46): a multi-view user of the reference has
 *                   no guide buffers at all.
 *
 * How the record differs from the aov integrator's: it is taken at the PIXEL CENTRE with the aperture sample
 * (.5, .5) (a thin lens traces from its centre), one ray per pixel, unjittered and unfiltered; it depends on
 * neither spp, seed, integrator nor group size; emitter shapes are geometry like any other (hide_emitters does
 * not apply); and the depth plane is the camera-space z of the hit in the pixel's own view, not si.t (a ray
 * parameter measured from the near plane).
 *
 * These are new entry points only: no struct of amvpt.h changes, AMVPT_ABI_VERSION stays as it is and this header
 * carries a version of its own.  Status codes and amvpt_last_error() are amvpt.h's.
 *
 * Numerics.  amvpt_guides evaluates the render's own raygen, closest-hit walk and surface interaction on the
 * render's own constants, so its records are bit-identical to what the render's primary vertex would see through
 * the pixel centre.  The depth entries are unfused float32 built from +, -, *, / and rint alone: device entry and
 * host entry agree bit for bit.
 */
#ifndef AMVPT_GUIDES_H
#define AMVPT_GUIDES_H

#include "amvpt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AMVPT_GUIDES_VERSION 1

uint32_t amvpt_guides_version(void);

/*
 * The guide record of every pixel of a rectangle of the quilt crop: out_device receives h x w x 8 float32,
 *   [0]    shape index, 0-based in amvpt_scene_desc::shapes, -1 on a miss
 *   [1..3] geometric normal of the hit   (0 on a miss)
 *   [4..6] hit point, world space         (0 on a miss)
 *   [7]    view index of the pixel (sample_ray_idx's, after reverse_x / reverse_y and the clamp)
 * rect = {x0, y0, w, h} in pixels of the quilt crop (film_width x film_height); NULL: all of it.  A view-group
 * rank asks for its own tiles.  out_device must be 16-byte aligned.  Ordered on `stream`.
 *
 * amvpt_params is validated as amvpt_render_ex validates it.  The traversal mode is amvpt_set_traversal's.
 * The call needs the view table on the device: it takes the device's lane arena under its lock, as a render
 * does, and so serialises with renders on that device; it allocates nothing else (and nothing when a render
 * has run before).
 * AMVPT_ERR_INVALID, naming the argument: a null pointer, a rectangle outside the quilt crop or of zero area,
 * an output that is not 16-byte aligned.
 */
amvpt_status amvpt_guides(amvpt_scene *scene, const amvpt_view_desc *views, const amvpt_params *params,
                          const uint32_t rect[4], float *out_device, void *stream);

/*
 * Guide records -> one float per pixel: z = ((m[8] p.x + m[9] p.y) + m[10] p.z) + m[11] with p the record's hit
 * point and m = views[(uint32_t) record[7]].to_world_inv; +inf on a miss.  `views` is a host pointer.  A record
 * whose view index is not in [0, n_views): the host entry refuses the call, the device entry treats the pixel
 * as a miss.
 */
amvpt_status amvpt_guide_depth(const float *guides_device, const amvpt_view_desc *views, uint32_t n_views,
                               uint64_t n_pixels, float *depth_device, void *stream);

/* {min, max} over the finite values of a depth plane, exact (integer atomics: no summation order); {0, 0} when
 * there is none.  Synchronises `stream`; near_far_host is a host pointer. */
amvpt_status amvpt_guide_depth_range(const float *depth_device, uint64_t n, float near_far_host[2], void *stream);

/*
 * Depth plane -> h x w x 3 uint8 with the same byte in the three channels (feeds amvpt_interlace and a PNG
 * writer unchanged).  Nearer is brighter: t = (far - z) / (far - near) clamped to [0, 1], code = rint(255 t) in
 * float32, half to even.  A z that is not finite (a miss) gives 0; far == near gives 255 for every hit.
 * AMVPT_ERR_INVALID: near or far not finite, far < near, a null pointer, a dimension of 0.
 */
amvpt_status amvpt_depth8(const float *depth_device, uint32_t w, uint32_t h, float near, float far,
                          uint8_t *out_device, void *stream);

/* The same functions over host pointers, compiled for the host from the same per-element code: they need no
 * device and never return AMVPT_ERR_NO_DEVICE. */
amvpt_status amvpt_guide_depth_host(const float *guides, const amvpt_view_desc *views, uint32_t n_views,
                                    uint64_t n_pixels, float *depth);
amvpt_status amvpt_guide_depth_range_host(const float *depth, uint64_t n, float near_far[2]);
amvpt_status amvpt_depth8_host(const float *depth, uint32_t w, uint32_t h, float near, float far, uint8_t *out);

#ifdef __cplusplus
}
#endif

#endif /* AMVPT_GUIDES_H */

/*
 * amvpt_temporal.hip -- the entries of include/amvpt_temporal.h: the previous frame's accumulated quilt reprojected
 * through the guide records and blended with the current one.  One launch on the caller's stream, one thread per
 * pixel, blocks of 32 x 8 pixels in a flat grid; a pure gather with no LDS, no atomics and no device-wide
 * synchronisation.  The previous views travel to the device once per call, into a buffer the library keeps for reuse
 * (ViewBuf of viewbuf.h).  The per-pixel function is dtemporal.h's, shared with the host-only entry below.
 *
 * amvpt_temporal_moments of include/amvpt_variance.h lives here too: k_temporal_moments is the second instance of that
 * per-pixel function, and its entries share the checks, the view table's upload and the launch with amvpt_temporal's.
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/amvpt_temporal.h"
#include "../../include/amvpt_variance.h"
#include "dtemporal.h"
#include "dtile.h"
#include "internal.h"
#include "post_host.h"
#include "viewbuf.h"

namespace amvpt {

__global__ void __launch_bounds__(kTileBlock) k_temporal(TemporalArgs A) {
    const TilePixel t = tile_pixel(A.tiles_x);
    if (t.x >= A.L.rw || t.y >= A.L.rh) return;
    temporal_pixel(A, t.x, t.y);
}

/* amvpt_temporal_moments (include/amvpt_variance.h): the moments instance of the same per-pixel function */
__global__ void __launch_bounds__(kTileBlock) k_temporal_moments(TemporalMomentsArgs A) {
    const TilePixel t = tile_pixel(A.tiles_x);
    if (t.x >= A.L.rw || t.y >= A.L.rh) return;
    temporal_pixel(A, t.x, t.y);
}

/* the refusals of all four entries (hist_moments and out_moments are null for amvpt_temporal's two); on success A
 * holds everything but the view table and the launch geometry */
static amvpt_status temporal_check(const Refusal &R, const float *image, uint32_t channels, const float *guides,
                                   const float *hist_image, const float *hist_guides, const float *hist_count,
                                   const float *hist_moments, const amvpt_view_desc *prev_views, const amvpt_params *p,
                                   const uint32_t *rect, const amvpt_temporal_params *tp, float *out_image, float *out_count,
                                   float *out_moments, TemporalArgs &A) {
    if (!image) return R.bad("null image");
    if (!guides) return R.bad("null guides");
    if (!hist_image) return R.bad("null hist_image");
    if (!hist_guides) return R.bad("null hist_guides");
    if (!hist_count) return R.bad("null hist_count");
    if (!prev_views) return R.bad("null prev_views");
    if (!p) return R.bad("null params");
    if (!tp) return R.bad("null tp");
    if (!out_image) return R.bad("null out_image");
    if (!out_count) return R.bad("null out_count");
    if (amvpt_status st = check_channels(R, channels)) return st;
    if (tp->max_history < 1u || tp->max_history > 65535u)
        return R.bad("tp: max_history must be 1 .. 65535, not " + std::to_string(tp->max_history));
    if (!pp_finite(tp->plane_tol) || !(tp->plane_tol > 0.f)) return R.bad("tp: plane_tol must be finite and above 0");
    if (!(tp->normal_cos >= -1.f && tp->normal_cos <= 1.f)) return R.bad("tp: normal_cos must be -1 .. 1");
    if (amvpt_status st = check_layout(R, "params", p, A.L)) return st;
    if (amvpt_status st = check_rect(R, rect, A.L)) return st;
    const size_t ncnt = (size_t) A.L.rw * (size_t) A.L.rh * sizeof(float), nimg = ncnt * channels, ngd = ncnt * 8, nmom = ncnt * 2;
    if (amvpt_status st = check_disjoint(
            R, {{out_count, ncnt, "out_count"}, {out_image, nimg, "out_image"}, {out_moments, nmom, "out_moments"}},
            {{image, nimg, "the image"}, {guides, ngd, "the guides"}, {hist_image, nimg, "hist_image"},
             {hist_guides, ngd, "hist_guides"}, {hist_count, ncnt, "hist_count"}, {hist_moments, nmom, "hist_moments"}}))
        return st;
    A.image = image, A.guides = guides, A.hist_image = hist_image, A.hist_guides = hist_guides, A.hist_count = hist_count;
    A.views = prev_views;
    A.out_image = out_image, A.out_count = out_count;
    A.channels = channels;
    A.max_history = (float) tp->max_history, A.plane_tol = tp->plane_tol, A.normal_cos = tp->normal_cos;
    A.tiles_x = 0;
    return AMVPT_OK;
}

/* amvpt_temporal_moments': its two planes, h x w x 2 over the same rectangle, and then the above */
static amvpt_status temporal_moments_check(const Refusal &R, const float *image, uint32_t channels, const float *guides,
                                           const float *hist_image, const float *hist_guides, const float *hist_count,
                                           const float *hist_moments, const amvpt_view_desc *prev_views, const amvpt_params *p,
                                           const uint32_t *rect, const amvpt_temporal_params *tp, float *out_image,
                                           float *out_count, float *out_moments, TemporalMomentsArgs &A) {
    if (!hist_moments) return R.bad("null hist_moments");
    if (!out_moments) return R.bad("null out_moments");
    A.hist_moments = hist_moments, A.out_moments = out_moments;
    return temporal_check(R, image, channels, guides, hist_image, hist_guides, hist_count, hist_moments, prev_views, p, rect, tp,
                          out_image, out_count, out_moments, A);
}

/* the host half of both entries */
template <class Args> static void temporal_host(const Args &A) {
    for (int32_t y = 0; y < A.L.rh; ++y)
        for (int32_t x = 0; x < A.L.rw; ++x) temporal_pixel(A, x, y);
}

/* the device half of both entries: the view table's upload and the one launch of kernel `k` over checked arguments */
template <class Args>
static amvpt_status temporal_launch(const Refusal &R, void (*k)(Args), Args &A, const amvpt_view_desc *prev_views, void *stream) {
    /* one launch of 32 x 8 tiles covers the rectangle: film sides are at most 2^24 */
    uint64_t tx, ty;
    if (amvpt_status s = check_tiles(R, "rect", (uint32_t) A.L.rw, (uint32_t) A.L.rh, tx, ty)) return s;
    if (amvpt_status s = R.need_device()) return s;
    hipStream_t st = (hipStream_t) stream;
    const uint32_t nv = A.L.multisensor ? A.L.n_views : 1u;
    const size_t vbytes = (size_t) nv * sizeof(amvpt_view_desc);
    return view_buf_launch(
        R.who, vbytes, st, [&](void *host) { std::memcpy(host, prev_views, vbytes); },
        [&](const void *dev) {
            A.views = (const amvpt_view_desc *) dev;
            A.tiles_x = (uint32_t) tx;
            hipLaunchKernelGGL(k, dim3((uint32_t) (tx * ty)), dim3(kTileBlock), 0, st, A);
            return hipGetLastError();
        });
}

} // namespace amvpt

using namespace amvpt;

extern "C" {

uint32_t amvpt_temporal_version(void) { return AMVPT_TEMPORAL_VERSION; }

amvpt_temporal_params amvpt_temporal_default_params(void) {
    amvpt_temporal_params p;
    p.max_history = 32;
    p.plane_tol = 0.02f;
    p.normal_cos = 0.9f;
    return p;
}

amvpt_status amvpt_temporal_host(const float *image, uint32_t channels, const float *guides, const float *hist_image,
                                 const float *hist_guides, const float *hist_count, const amvpt_view_desc *prev_views,
                                 const amvpt_params *params, const uint32_t rect[4], const amvpt_temporal_params *tp,
                                 float *out_image, float *out_count) {
    TemporalArgs A;
    if (amvpt_status s = temporal_check(Refusal("amvpt_temporal_host"), image, channels, guides, hist_image, hist_guides,
                                        hist_count, nullptr, prev_views, params, rect, tp, out_image, out_count, nullptr, A))
        return s;
    temporal_host(A);
    return AMVPT_OK;
}

amvpt_status amvpt_temporal(const float *image_device, uint32_t channels, const float *guides_device,
                            const float *hist_image_device, const float *hist_guides_device,
                            const float *hist_count_device, const amvpt_view_desc *prev_views,
                            const amvpt_params *params, const uint32_t rect[4], const amvpt_temporal_params *tp,
                            float *out_image_device, float *out_count_device, void *stream) {
    const Refusal R("amvpt_temporal");
    TemporalArgs A;
    if (amvpt_status s = temporal_check(R, image_device, channels, guides_device, hist_image_device, hist_guides_device,
                                        hist_count_device, nullptr, prev_views, params, rect, tp, out_image_device,
                                        out_count_device, nullptr, A))
        return s;
    return temporal_launch(R, k_temporal, A, prev_views, stream);
}

/* include/amvpt_variance.h, stage 1 */
amvpt_status amvpt_temporal_moments_host(const float *image, uint32_t channels, const float *guides, const float *hist_image,
                                         const float *hist_guides, const float *hist_count, const float *hist_moments,
                                         const amvpt_view_desc *prev_views, const amvpt_params *params, const uint32_t rect[4],
                                         const amvpt_temporal_params *tp, float *out_image, float *out_count,
                                         float *out_moments) {
    TemporalMomentsArgs A;
    if (amvpt_status s = temporal_moments_check(Refusal("amvpt_temporal_moments_host"), image, channels, guides, hist_image,
                                                hist_guides, hist_count, hist_moments, prev_views, params, rect, tp, out_image,
                                                out_count, out_moments, A))
        return s;
    temporal_host(A);
    return AMVPT_OK;
}

amvpt_status amvpt_temporal_moments(const float *image_device, uint32_t channels, const float *guides_device,
                                    const float *hist_image_device, const float *hist_guides_device,
                                    const float *hist_count_device, const float *hist_moments_device,
                                    const amvpt_view_desc *prev_views, const amvpt_params *params, const uint32_t rect[4],
                                    const amvpt_temporal_params *tp, float *out_image_device, float *out_count_device,
                                    float *out_moments_device, void *stream) {
    const Refusal R("amvpt_temporal_moments");
    TemporalMomentsArgs A;
    if (amvpt_status s = temporal_moments_check(R, image_device, channels, guides_device, hist_image_device, hist_guides_device,
                                                hist_count_device, hist_moments_device, prev_views, params, rect, tp,
                                                out_image_device, out_count_device, out_moments_device, A))
        return s;
    return temporal_launch(R, k_temporal_moments, A, prev_views, stream);
}

} // extern "C"

/*
 * amvpt_synth.hip -- the entries of include/amvpt_synth.h: the views of a dense quilt gathered from the rendered views
 * of a sparse one through the guide records (k_synth), and the fill of the holes that leaves (k_synth_fill, one launch
 * per iteration).  Launches are ordered on the caller's stream, one thread per target pixel, blocks of 32 x 8 pixels in
 * a flat grid; pure gathers with no LDS, no atomics and no device-wide synchronisation.  The source views and the
 * target views' origins travel to the device once per call in one block, into a buffer the library keeps for reuse
 * (ViewBuf of viewbuf.h, the code amvpt_temporal.hip uploads its views with; each unit has a pool of its own).
 * The per-pixel functions are dsynth.h's, shared with the host-only entries below.
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/amvpt_synth.h"
#include "dsynth.h"
#include "dtile.h"
#include "internal.h"
#include "post_host.h"
#include "viewbuf.h"

namespace amvpt {

static constexpr uint32_t kMaxSourceViews = 64;

__global__ void __launch_bounds__(kTileBlock) k_synth(SynthArgs A) {
    const TilePixel t = tile_pixel(A.tiles_x);
    if (t.x >= A.D.rw || t.y >= A.D.rh) return;
    synth_pixel(A, t.x, t.y);
}

__global__ void __launch_bounds__(kTileBlock) k_synth_fill(SynthFillArgs A) {
    const TilePixel t = tile_pixel(A.tiles_x);
    if (t.x >= (int) A.w || t.y >= (int) A.h) return;
    synth_fill_pixel(A, t.x, t.y);
}

/* the parameter ranges, for both stages */
static amvpt_status synth_params_check(const Refusal &R, const amvpt_synth_params *sp) {
    if (!pp_finite(sp->plane_tol) || !(sp->plane_tol > 0.f)) return R.bad("sp: plane_tol must be finite and above 0");
    if (!(sp->normal_cos >= -1.f && sp->normal_cos <= 1.f)) return R.bad("sp: normal_cos must be -1 .. 1");
    if (!pp_finite(sp->view_falloff) || !(sp->view_falloff >= 0.f)) return R.bad("sp: view_falloff must be finite and at least 0");
    if (sp->fill_iterations > 8u) return R.bad("sp: fill_iterations must be 0 .. 8, not " + std::to_string(sp->fill_iterations));
    return AMVPT_OK;
}

/* the refusals of both entries of stage 1; on success A holds everything but the view tables and the launch geometry */
static amvpt_status synth_check(const Refusal &R, const float *src_image, uint32_t channels, const float *src_guides,
                                const amvpt_view_desc *src_views, const amvpt_params *src_params, const float *dst_guides,
                                const amvpt_view_desc *dst_views, const amvpt_params *dst_params, const uint32_t *rect,
                                const amvpt_synth_params *sp, float *dst_image, float *dst_cover, SynthArgs &A) {
    if (!src_image) return R.bad("null src_image");
    if (!src_guides) return R.bad("null src_guides");
    if (!src_views) return R.bad("null src_views");
    if (!src_params) return R.bad("null src_params");
    if (!dst_guides) return R.bad("null dst_guides");
    if (!dst_views) return R.bad("null dst_views");
    if (!dst_params) return R.bad("null dst_params");
    if (!sp) return R.bad("null sp");
    if (!dst_image) return R.bad("null dst_image");
    if (!dst_cover) return R.bad("null dst_cover");
    if (amvpt_status st = check_channels(R, channels)) return st;
    if (amvpt_status st = synth_params_check(R, sp)) return st;
    if (amvpt_status st = check_layout(R, "src_params", src_params, A.S)) return st;
    if (amvpt_status st = check_layout(R, "dst_params", dst_params, A.D)) return st;
    if (A.S.multisensor && A.S.n_views > kMaxSourceViews)
        return R.bad("src_params: more than 64 source views (n_views is " + std::to_string(A.S.n_views) + ")");
    if (amvpt_status st = check_rect(R, rect, A.D)) return st;
    const size_t ncov = (size_t) A.D.rw * (size_t) A.D.rh * sizeof(float), nimg = ncov * channels;
    const size_t nsrc = (size_t) A.S.rw * (size_t) A.S.rh * sizeof(float);
    if (amvpt_status st = check_disjoint(
            R, {{dst_cover, ncov, "dst_cover"}, {dst_image, nimg, "dst_image"}},
            {{src_image, nsrc * channels, "src_image"}, {src_guides, nsrc * 8, "src_guides"}, {dst_guides, ncov * 8, "dst_guides"}}))
        return st;
    A.src_image = src_image, A.src_guides = src_guides, A.dst_guides = dst_guides;
    A.src_views = src_views, A.dst_origins = nullptr;
    A.dst_image = dst_image, A.dst_cover = dst_cover;
    A.channels = channels;
    A.plane_tol = sp->plane_tol, A.normal_cos = sp->normal_cos, A.view_falloff = sp->view_falloff;
    A.tiles_x = 0;
    return AMVPT_OK;
}

static void synth_origins(const amvpt_view_desc *dst_views, uint32_t nd, float *out) {
    for (uint32_t t = 0; t < nd; ++t) {
        const float *m = dst_views[t].to_world;
        out[3 * t] = m[3], out[3 * t + 1] = m[7], out[3 * t + 2] = m[11];
    }
}

/* the refusals of both entries of stage 2 */
static amvpt_status synth_fill_check(const Refusal &R, const float *image, uint32_t channels, uint32_t w, uint32_t h,
                                     const float *cover, const float *guides, const amvpt_synth_params *sp, const float *out,
                                     const float *scratch, const float *cover_out, const float *cover_scratch) {
    if (!image) return R.bad("null image");
    if (!cover) return R.bad("null cover");
    if (!guides) return R.bad("null guides");
    if (!sp) return R.bad("null sp");
    if (!out) return R.bad("null out");
    if (!cover_out) return R.bad("null cover_out");
    if (amvpt_status st = check_channels(R, channels)) return st;
    if (amvpt_status st = check_size_tiles(R, w, h)) return st;
    if (amvpt_status st = synth_params_check(R, sp)) return st;
    if (sp->fill_iterations > 1u && !scratch) return R.bad("null scratch (it may be null only when fill_iterations is at most 1)");
    if (sp->fill_iterations > 1u && !cover_scratch)
        return R.bad("null cover_scratch (it may be null only when fill_iterations is at most 1)");
    const size_t ncov = (size_t) w * h * sizeof(float), nimg = ncov * channels, ngd = ncov * 8;
    return check_disjoint(
        R, {{out, nimg, "out"}, {scratch, nimg, "scratch"}, {cover_out, ncov, "cover_out"}, {cover_scratch, ncov, "cover_scratch"}},
        {{image, nimg, "the image"}, {cover, ncov, "the cover"}, {guides, ngd, "the guides"}});
}

} // namespace amvpt

using namespace amvpt;

extern "C" {

uint32_t amvpt_synth_version(void) { return AMVPT_SYNTH_VERSION; }

amvpt_synth_params amvpt_synth_default_params(void) {
    amvpt_synth_params p;
    p.plane_tol = 0.02f;
    p.normal_cos = 0.9f;
    p.view_falloff = 1e5f;
    p.fill_iterations = 4;
    return p;
}

amvpt_status amvpt_synth_host(const float *src_image, uint32_t channels, const float *src_guides,
                              const amvpt_view_desc *src_views, const amvpt_params *src_params, const float *dst_guides,
                              const amvpt_view_desc *dst_views, const amvpt_params *dst_params, const uint32_t rect[4],
                              const amvpt_synth_params *sp, float *dst_image, float *dst_cover) {
    SynthArgs A;
    if (amvpt_status s = synth_check(Refusal("amvpt_synth_host"), src_image, channels, src_guides, src_views, src_params,
                                     dst_guides, dst_views, dst_params, rect, sp, dst_image, dst_cover, A))
        return s;
    const uint32_t nd = A.D.multisensor ? A.D.n_views : 1u;
    std::vector<float> origins(3 * (size_t) nd);
    synth_origins(dst_views, nd, origins.data());
    A.dst_origins = origins.data();
    for (int32_t y = 0; y < A.D.rh; ++y)
        for (int32_t x = 0; x < A.D.rw; ++x) synth_pixel(A, x, y);
    return AMVPT_OK;
}

amvpt_status amvpt_synth(const float *src_image_device, uint32_t channels, const float *src_guides_device,
                         const amvpt_view_desc *src_views, const amvpt_params *src_params,
                         const float *dst_guides_device, const amvpt_view_desc *dst_views,
                         const amvpt_params *dst_params, const uint32_t rect[4], const amvpt_synth_params *sp,
                         float *dst_image_device, float *dst_cover_device, void *stream) {
    const Refusal R("amvpt_synth");
    SynthArgs A;
    if (amvpt_status s = synth_check(R, src_image_device, channels, src_guides_device, src_views, src_params, dst_guides_device,
                                     dst_views, dst_params, rect, sp, dst_image_device, dst_cover_device, A))
        return s;
    /* one launch of 32 x 8 tiles covers the rectangle: film sides are at most 2^24 */
    uint64_t tx, ty;
    if (amvpt_status s = check_tiles(R, "rect", (uint32_t) A.D.rw, (uint32_t) A.D.rh, tx, ty)) return s;
    if (amvpt_status s = R.need_device()) return s;
    hipStream_t st = (hipStream_t) stream;
    const uint32_t ns = A.S.multisensor ? A.S.n_views : 1u, nd = A.D.multisensor ? A.D.n_views : 1u;
    const size_t vbytes = (size_t) ns * sizeof(amvpt_view_desc), obytes = (size_t) nd * 3 * sizeof(float);
    static_assert(sizeof(amvpt_view_desc) % sizeof(float) == 0, "the origins follow the views in one block");
    return view_buf_launch(
        R.who, vbytes + obytes, st,
        [&](void *host) {
            std::memcpy(host, src_views, vbytes);
            synth_origins(dst_views, nd, (float *) ((char *) host + vbytes));
        },
        [&](const void *dev) {
            A.src_views = (const amvpt_view_desc *) dev;
            A.dst_origins = (const float *) ((const char *) dev + vbytes);
            A.tiles_x = (uint32_t) tx;
            hipLaunchKernelGGL(k_synth, dim3((uint32_t) (tx * ty)), dim3(kTileBlock), 0, st, A);
            return hipGetLastError();
        });
}

amvpt_status amvpt_synth_fill_host(const float *image, uint32_t channels, uint32_t width, uint32_t height,
                                   const float *cover, const float *guides, const amvpt_synth_params *sp, float *out,
                                   float *scratch, float *cover_out, float *cover_scratch) {
    if (amvpt_status s = synth_fill_check(Refusal("amvpt_synth_fill_host"), image, channels, width, height, cover, guides, sp, out, scratch,
                                          cover_out, cover_scratch))
        return s;
    const size_t npx = (size_t) width * height;
    const uint32_t n = sp->fill_iterations;
    if (n == 0) {
        std::memcpy(out, image, npx * channels * sizeof(float));
        std::memcpy(cover_out, cover, npx * sizeof(float));
        return AMVPT_OK;
    }
    const float *in = image, *cin = cover;
    for (uint32_t i = 0; i < n; ++i) {
        float *dst = pingpong_dst(i, n, out, scratch), *cdst = pingpong_dst(i, n, cover_out, cover_scratch);
        const SynthFillArgs A{in, cin, guides, dst, cdst, channels, width, height, 0u, (int32_t) (1u << i), sp->plane_tol, sp->normal_cos};
        for (uint32_t y = 0; y < height; ++y)
            for (uint32_t x = 0; x < width; ++x) synth_fill_pixel(A, (int32_t) x, (int32_t) y);
        in = dst, cin = cdst;
    }
    return AMVPT_OK;
}

amvpt_status amvpt_synth_fill(const float *image_device, uint32_t channels, uint32_t width, uint32_t height,
                              const float *cover_device, const float *guides_device, const amvpt_synth_params *sp,
                              float *out_device, float *scratch_device, float *cover_out_device,
                              float *cover_scratch_device, void *stream) {
    const Refusal R("amvpt_synth_fill");
    if (amvpt_status s = synth_fill_check(R, image_device, channels, width, height, cover_device, guides_device, sp, out_device,
                                          scratch_device, cover_out_device, cover_scratch_device))
        return s;
    if (amvpt_status s = R.need_device()) return s;
    hipStream_t st = (hipStream_t) stream;
    const size_t npx = (size_t) width * height;
    const uint32_t n = sp->fill_iterations;
    if (n == 0) {
        hipError_t e = hipMemcpyAsync(out_device, image_device, npx * channels * sizeof(float), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(cover_out_device, cover_device, npx * sizeof(float), hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) return hip_fail("amvpt_synth_fill copy", (int) e);
        return AMVPT_OK;
    }
    uint64_t tx, ty;
    tile_grid(width, height, tx, ty);
    const float *in = image_device, *cin = cover_device;
    for (uint32_t i = 0; i < n; ++i) {
        float *dst = pingpong_dst(i, n, out_device, scratch_device), *cdst = pingpong_dst(i, n, cover_out_device, cover_scratch_device);
        const SynthFillArgs A{in, cin, guides_device, dst, cdst, channels, width, height, (uint32_t) tx, (int32_t) (1u << i), sp->plane_tol,
                              sp->normal_cos};
        hipLaunchKernelGGL(k_synth_fill, dim3((uint32_t) (tx * ty)), dim3(kTileBlock), 0, st, A);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail("amvpt_synth_fill launch", (int) e);
        in = dst, cin = cdst;
    }
    return AMVPT_OK;
}

} // extern "C"

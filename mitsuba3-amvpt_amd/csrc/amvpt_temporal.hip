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

#include <atomic>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/amvpt_temporal.h"
#include "../../include/amvpt_variance.h"
#include "dtemporal.h"
#include "internal.h"
#include "viewbuf.h"

namespace amvpt {

static constexpr int kTileW = 32, kTileH = 8;
static constexpr uint32_t kTemporalBlock = kTileW * kTileH;

__global__ void __launch_bounds__(kTemporalBlock) k_temporal(TemporalArgs A) {
    const int x = (int) (blockIdx.x % A.tiles_x) * kTileW + (int) (threadIdx.x % kTileW);
    const int y = (int) (blockIdx.x / A.tiles_x) * kTileH + (int) (threadIdx.x / kTileW);
    if (x >= A.L.rw || y >= A.L.rh) return;
    temporal_pixel(A, x, y);
}

/* amvpt_temporal_moments (include/amvpt_variance.h): the moments instance of the same per-pixel function */
__global__ void __launch_bounds__(kTemporalBlock) k_temporal_moments(TemporalMomentsArgs A) {
    const int x = (int) (blockIdx.x % A.tiles_x) * kTileW + (int) (threadIdx.x % kTileW);
    const int y = (int) (blockIdx.x / A.tiles_x) * kTileH + (int) (threadIdx.x / kTileW);
    if (x >= A.L.rw || y >= A.L.rh) return;
    temporal_pixel(A, x, y);
}

/* a visible device is remembered (it does not go away); its absence is asked again on the next call */
static bool temporal_device_ok() {
    static std::atomic<bool> seen{false};
    if (seen.load(std::memory_order_relaxed)) return true;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return false;
    seen.store(true, std::memory_order_relaxed);
    return true;
}

static bool tp_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t a0 = (uintptr_t) a, b0 = (uintptr_t) b;
    return a0 < b0 + nb && b0 < a0 + na;
}

/* the refusals of both entries; on success A holds everything but the view table and the launch geometry */
static amvpt_status temporal_check(const char *who, const float *image, uint32_t channels, const float *guides,
                                   const float *hist_image, const float *hist_guides, const float *hist_count,
                                   const amvpt_view_desc *prev_views, const amvpt_params *p, const uint32_t *rect,
                                   const amvpt_temporal_params *tp, float *out_image, float *out_count, TemporalArgs &A) {
    const std::string s = std::string(who) + ": ";
    auto bad = [&](const std::string &what) { set_error(s + what); return AMVPT_ERR_INVALID; };
    auto unsupported = [&](const std::string &what) { set_error(s + what); return AMVPT_ERR_UNSUPPORTED; };
    if (!image) return bad("null image");
    if (!guides) return bad("null guides");
    if (!hist_image) return bad("null hist_image");
    if (!hist_guides) return bad("null hist_guides");
    if (!hist_count) return bad("null hist_count");
    if (!prev_views) return bad("null prev_views");
    if (!p) return bad("null params");
    if (!tp) return bad("null tp");
    if (!out_image) return bad("null out_image");
    if (!out_count) return bad("null out_count");
    if (channels != 3u && channels != 4u) return bad("channels must be 3 or 4, not " + std::to_string(channels));
    if (p->film_width == 0) return bad("params: film_width is 0");
    if (p->film_height == 0) return bad("params: film_height is 0");
    /* pixel coordinates are formed as floats */
    if (p->film_width > (1u << 24) || p->film_height > (1u << 24)) return bad("params: film_width or film_height above 2^24");
    if (tp->max_history < 1u || tp->max_history > 65535u)
        return bad("tp: max_history must be 1 .. 65535, not " + std::to_string(tp->max_history));
    if (!tp_finite(tp->plane_tol) || !(tp->plane_tol > 0.f)) return bad("tp: plane_tol must be finite and above 0");
    if (!(tp->normal_cos >= -1.f && tp->normal_cos <= 1.f)) return bad("tp: normal_cos must be -1 .. 1");
    if (p->crop_offset_x || p->crop_offset_y) return unsupported("params: a crop window (crop_offset) is not supported");
    if ((p->full_width && p->full_width != p->film_width) || (p->full_height && p->full_height != p->film_height))
        return unsupported("params: a crop window (full_width / full_height differ from the film) is not supported");
    TemporalLayout &L = A.L;
    L.multisensor = p->multisensor ? 1u : 0u;
    L.batch = p->batch ? 1u : 0u;
    L.n_views = p->n_views, L.gx = p->grid_x, L.gy = p->grid_y;
    L.rev_x = p->reverse_x ? 1u : 0u, L.rev_y = p->reverse_y ? 1u : 0u;
    uint32_t tw = p->film_width, th = p->film_height;
    if (L.multisensor) {
        if (p->n_views == 0) return bad("params: n_views is 0");
        if (L.batch) {
            if (p->film_width % p->n_views) return unsupported("params: film_width is not a multiple of n_views");
            tw = p->film_width / p->n_views;
        } else {
            if (p->grid_x == 0 || p->grid_y == 0) return bad("params: grid_x or grid_y is 0");
            if ((uint64_t) p->grid_x * p->grid_y != p->n_views) return unsupported("params: n_views is not grid_x * grid_y");
            if (p->film_width % p->grid_x || p->film_height % p->grid_y)
                return unsupported("params: the film size is not a multiple of the grid");
            tw = p->film_width / p->grid_x, th = p->film_height / p->grid_y;
        }
    }
    L.tw = (int32_t) tw, L.th = (int32_t) th;
    uint32_t r[4] = {0u, 0u, p->film_width, p->film_height};
    if (rect) {
        for (int i = 0; i < 4; ++i) r[i] = rect[i];
        if (r[2] == 0 || r[3] == 0) return bad("rect: zero area");
        if (r[0] >= p->film_width || r[2] > p->film_width - r[0] || r[1] >= p->film_height || r[3] > p->film_height - r[1])
            return bad("rect: outside the film");
        if (r[0] % tw || r[2] % tw || r[1] % th || r[3] % th) return bad("rect: not made of whole tiles");
    }
    L.rx0 = (int32_t) r[0], L.ry0 = (int32_t) r[1], L.rw = (int32_t) r[2], L.rh = (int32_t) r[3];
    const size_t npx = (size_t) r[2] * r[3], ncnt = npx * sizeof(float), nimg = ncnt * channels, ngd = ncnt * 8;
    const struct { const void *p; size_t n; const char *name; } in[5] = {
        {image, nimg, "the image"}, {guides, ngd, "the guides"}, {hist_image, nimg, "hist_image"},
        {hist_guides, ngd, "hist_guides"}, {hist_count, ncnt, "hist_count"}};
    for (const auto &i : in) {
        if (tp_overlap(out_image, nimg, i.p, i.n)) return bad(std::string("out_image overlaps ") + i.name);
        if (tp_overlap(out_count, ncnt, i.p, i.n)) return bad(std::string("out_count overlaps ") + i.name);
    }
    if (tp_overlap(out_image, nimg, out_count, ncnt)) return bad("out_image overlaps out_count");
    A.image = image, A.guides = guides, A.hist_image = hist_image, A.hist_guides = hist_guides, A.hist_count = hist_count;
    A.views = prev_views;
    A.out_image = out_image, A.out_count = out_count;
    A.channels = channels;
    A.max_history = (float) tp->max_history, A.plane_tol = tp->plane_tol, A.normal_cos = tp->normal_cos;
    A.tiles_x = 0;
    return AMVPT_OK;
}

/* the refusals amvpt_temporal_moments adds to temporal_check's: its two planes, h x w x 2 over the same rectangle */
static amvpt_status temporal_moments_check(const char *who, const float *image, uint32_t channels, const float *guides,
                                           const float *hist_image, const float *hist_guides, const float *hist_count,
                                           const float *hist_moments, const amvpt_view_desc *prev_views, const amvpt_params *p,
                                           const uint32_t *rect, const amvpt_temporal_params *tp, float *out_image,
                                           float *out_count, float *out_moments, TemporalMomentsArgs &A) {
    const std::string s = std::string(who) + ": ";
    auto bad = [&](const std::string &what) { set_error(s + what); return AMVPT_ERR_INVALID; };
    if (!hist_moments) return bad("null hist_moments");
    if (!out_moments) return bad("null out_moments");
    if (amvpt_status st = temporal_check(who, image, channels, guides, hist_image, hist_guides, hist_count, prev_views, p, rect,
                                         tp, out_image, out_count, A))
        return st;
    const size_t ncnt = (size_t) A.L.rw * (size_t) A.L.rh * sizeof(float), nimg = ncnt * channels, ngd = ncnt * 8, nmom = ncnt * 2;
    const struct { const void *p; size_t n; const char *name; } in[5] = {
        {image, nimg, "the image"}, {guides, ngd, "the guides"}, {hist_image, nimg, "hist_image"},
        {hist_guides, ngd, "hist_guides"}, {hist_count, ncnt, "hist_count"}};
    for (const auto &i : in)
        if (tp_overlap(out_moments, nmom, i.p, i.n)) return bad(std::string("out_moments overlaps ") + i.name);
    if (tp_overlap(out_image, nimg, hist_moments, nmom)) return bad("out_image overlaps hist_moments");
    if (tp_overlap(out_count, ncnt, hist_moments, nmom)) return bad("out_count overlaps hist_moments");
    if (tp_overlap(out_moments, nmom, hist_moments, nmom)) return bad("out_moments overlaps hist_moments");
    if (tp_overlap(out_moments, nmom, out_image, nimg)) return bad("out_moments overlaps out_image");
    if (tp_overlap(out_moments, nmom, out_count, ncnt)) return bad("out_moments overlaps out_count");
    A.hist_moments = hist_moments, A.out_moments = out_moments;
    return AMVPT_OK;
}

/* the device half of both entries: the view table's upload and the one launch of kernel `k` over checked arguments */
template <class Args>
static amvpt_status temporal_launch(const char *who, void (*k)(Args), Args &A, const amvpt_view_desc *prev_views, void *stream) {
    const std::string s(who);
    /* one launch of 32 x 8 tiles covers the rectangle: film sides are at most 2^24 */
    const uint64_t tx = ((uint32_t) A.L.rw + (uint32_t) kTileW - 1u) / (uint32_t) kTileW;
    const uint64_t ty = ((uint32_t) A.L.rh + (uint32_t) kTileH - 1u) / (uint32_t) kTileH;
    if (tx * ty >= (1ull << 31)) { set_error(s + ": rect above 2^31 tiles of 32 x 8 pixels"); return AMVPT_ERR_INVALID; }
    if (!temporal_device_ok()) { set_error(s + ": no HIP device visible"); return AMVPT_ERR_NO_DEVICE; }
    hipStream_t st = (hipStream_t) stream;
    const uint32_t nv = A.L.multisensor ? A.L.n_views : 1u;
    const size_t vbytes = (size_t) nv * sizeof(amvpt_view_desc);
    ViewBuf vb;
    if (amvpt_status rc = view_buf_take("amvpt_temporal", vbytes, vb)) return rc;
    std::memcpy(vb.host, prev_views, vbytes);
    hipError_t e = hipMemcpyAsync(vb.p, vb.host, vbytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        A.views = (const amvpt_view_desc *) vb.p;
        A.tiles_x = (uint32_t) tx;
        hipLaunchKernelGGL(k, dim3((uint32_t) (tx * ty)), dim3(kTemporalBlock), 0, st, A);
        e = hipGetLastError();
    }
    const hipError_t eg = view_buf_give(vb, st);
    if (e != hipSuccess) return hip_fail((s + " launch").c_str(), (int) e);
    if (eg != hipSuccess) return hip_fail((s + " hipEventRecord").c_str(), (int) eg);
    return AMVPT_OK;
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
    if (amvpt_status s = temporal_check("amvpt_temporal_host", image, channels, guides, hist_image, hist_guides, hist_count,
                                        prev_views, params, rect, tp, out_image, out_count, A))
        return s;
    for (int32_t y = 0; y < A.L.rh; ++y)
        for (int32_t x = 0; x < A.L.rw; ++x) temporal_pixel(A, x, y);
    return AMVPT_OK;
}

amvpt_status amvpt_temporal(const float *image_device, uint32_t channels, const float *guides_device,
                            const float *hist_image_device, const float *hist_guides_device,
                            const float *hist_count_device, const amvpt_view_desc *prev_views,
                            const amvpt_params *params, const uint32_t rect[4], const amvpt_temporal_params *tp,
                            float *out_image_device, float *out_count_device, void *stream) {
    TemporalArgs A;
    if (amvpt_status s = temporal_check("amvpt_temporal", image_device, channels, guides_device, hist_image_device,
                                        hist_guides_device, hist_count_device, prev_views, params, rect, tp,
                                        out_image_device, out_count_device, A))
        return s;
    return temporal_launch("amvpt_temporal", k_temporal, A, prev_views, stream);
}

/* include/amvpt_variance.h, stage 1 */
amvpt_status amvpt_temporal_moments_host(const float *image, uint32_t channels, const float *guides, const float *hist_image,
                                         const float *hist_guides, const float *hist_count, const float *hist_moments,
                                         const amvpt_view_desc *prev_views, const amvpt_params *params, const uint32_t rect[4],
                                         const amvpt_temporal_params *tp, float *out_image, float *out_count,
                                         float *out_moments) {
    TemporalMomentsArgs A;
    if (amvpt_status s = temporal_moments_check("amvpt_temporal_moments_host", image, channels, guides, hist_image, hist_guides,
                                                hist_count, hist_moments, prev_views, params, rect, tp, out_image, out_count,
                                                out_moments, A))
        return s;
    for (int32_t y = 0; y < A.L.rh; ++y)
        for (int32_t x = 0; x < A.L.rw; ++x) temporal_pixel(A, x, y);
    return AMVPT_OK;
}

amvpt_status amvpt_temporal_moments(const float *image_device, uint32_t channels, const float *guides_device,
                                    const float *hist_image_device, const float *hist_guides_device,
                                    const float *hist_count_device, const float *hist_moments_device,
                                    const amvpt_view_desc *prev_views, const amvpt_params *params, const uint32_t rect[4],
                                    const amvpt_temporal_params *tp, float *out_image_device, float *out_count_device,
                                    float *out_moments_device, void *stream) {
    TemporalMomentsArgs A;
    if (amvpt_status s = temporal_moments_check("amvpt_temporal_moments", image_device, channels, guides_device,
                                                hist_image_device, hist_guides_device, hist_count_device, hist_moments_device,
                                                prev_views, params, rect, tp, out_image_device, out_count_device,
                                                out_moments_device, A))
        return s;
    return temporal_launch("amvpt_temporal_moments", k_temporal_moments, A, prev_views, stream);
}

} // extern "C"

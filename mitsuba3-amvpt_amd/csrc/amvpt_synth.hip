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

#include <atomic>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/amvpt_synth.h"
#include "dsynth.h"
#include "internal.h"
#include "viewbuf.h"

namespace amvpt {

static constexpr int kTileW = 32, kTileH = 8;
static constexpr uint32_t kSynthBlock = kTileW * kTileH;
static constexpr uint32_t kMaxSourceViews = 64;

__global__ void __launch_bounds__(kSynthBlock) k_synth(SynthArgs A) {
    const int x = (int) (blockIdx.x % A.tiles_x) * kTileW + (int) (threadIdx.x % kTileW);
    const int y = (int) (blockIdx.x / A.tiles_x) * kTileH + (int) (threadIdx.x / kTileW);
    if (x >= A.D.rw || y >= A.D.rh) return;
    synth_pixel(A, x, y);
}

__global__ void __launch_bounds__(kSynthBlock) k_synth_fill(SynthFillArgs A) {
    const int x = (int) (blockIdx.x % A.tiles_x) * kTileW + (int) (threadIdx.x % kTileW);
    const int y = (int) (blockIdx.x / A.tiles_x) * kTileH + (int) (threadIdx.x / kTileW);
    if (x >= (int) A.w || y >= (int) A.h) return;
    synth_fill_pixel(A, x, y);
}

/* a visible device is remembered (it does not go away); its absence is asked again on the next call */
static bool synth_device_ok() {
    static std::atomic<bool> seen{false};
    if (seen.load(std::memory_order_relaxed)) return true;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return false;
    seen.store(true, std::memory_order_relaxed);
    return true;
}

static bool sy_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t a0 = (uintptr_t) a, b0 = (uintptr_t) b;
    return a0 < b0 + nb && b0 < a0 + na;
}

/* the layout of one quilt (amvpt_temporal.h "Layout") and its refusals, `name` being the argument; the rectangle is
 * the whole film */
static amvpt_status synth_layout(const std::string &s, const char *name, const amvpt_params *p, TemporalLayout &L) {
    const std::string n = s + name + ": ";
    auto bad = [&](const std::string &what) { set_error(n + what); return AMVPT_ERR_INVALID; };
    auto unsupported = [&](const std::string &what) { set_error(n + what); return AMVPT_ERR_UNSUPPORTED; };
    if (p->film_width == 0) return bad("film_width is 0");
    if (p->film_height == 0) return bad("film_height is 0");
    /* pixel coordinates are formed as floats */
    if (p->film_width > (1u << 24) || p->film_height > (1u << 24)) return bad("film_width or film_height above 2^24");
    if (p->crop_offset_x || p->crop_offset_y) return unsupported("a crop window (crop_offset) is not supported");
    if ((p->full_width && p->full_width != p->film_width) || (p->full_height && p->full_height != p->film_height))
        return unsupported("a crop window (full_width / full_height differ from the film) is not supported");
    L.multisensor = p->multisensor ? 1u : 0u;
    L.batch = p->batch ? 1u : 0u;
    L.n_views = p->n_views, L.gx = p->grid_x, L.gy = p->grid_y;
    L.rev_x = p->reverse_x ? 1u : 0u, L.rev_y = p->reverse_y ? 1u : 0u;
    uint32_t tw = p->film_width, th = p->film_height;
    if (L.multisensor) {
        if (p->n_views == 0) return bad("n_views is 0");
        if (L.batch) {
            if (p->film_width % p->n_views) return unsupported("film_width is not a multiple of n_views");
            tw = p->film_width / p->n_views;
        } else {
            if (p->grid_x == 0 || p->grid_y == 0) return bad("grid_x or grid_y is 0");
            if ((uint64_t) p->grid_x * p->grid_y != p->n_views) return unsupported("n_views is not grid_x * grid_y");
            if (p->film_width % p->grid_x || p->film_height % p->grid_y)
                return unsupported("the film size is not a multiple of the grid");
            tw = p->film_width / p->grid_x, th = p->film_height / p->grid_y;
        }
    }
    L.tw = (int32_t) tw, L.th = (int32_t) th;
    L.rx0 = 0, L.ry0 = 0, L.rw = (int32_t) p->film_width, L.rh = (int32_t) p->film_height;
    return AMVPT_OK;
}

/* the parameter ranges, for both stages */
static amvpt_status synth_params_check(const std::string &s, const amvpt_synth_params *sp) {
    auto bad = [&](const std::string &what) { set_error(s + what); return AMVPT_ERR_INVALID; };
    if (!tp_finite(sp->plane_tol) || !(sp->plane_tol > 0.f)) return bad("sp: plane_tol must be finite and above 0");
    if (!(sp->normal_cos >= -1.f && sp->normal_cos <= 1.f)) return bad("sp: normal_cos must be -1 .. 1");
    if (!tp_finite(sp->view_falloff) || !(sp->view_falloff >= 0.f)) return bad("sp: view_falloff must be finite and at least 0");
    if (sp->fill_iterations > 8u) return bad("sp: fill_iterations must be 0 .. 8, not " + std::to_string(sp->fill_iterations));
    return AMVPT_OK;
}

/* the refusals of both entries of stage 1; on success A holds everything but the view tables and the launch geometry */
static amvpt_status synth_check(const char *who, const float *src_image, uint32_t channels, const float *src_guides,
                                const amvpt_view_desc *src_views, const amvpt_params *src_params, const float *dst_guides,
                                const amvpt_view_desc *dst_views, const amvpt_params *dst_params, const uint32_t *rect,
                                const amvpt_synth_params *sp, float *dst_image, float *dst_cover, SynthArgs &A) {
    const std::string s = std::string(who) + ": ";
    auto bad = [&](const std::string &what) { set_error(s + what); return AMVPT_ERR_INVALID; };
    if (!src_image) return bad("null src_image");
    if (!src_guides) return bad("null src_guides");
    if (!src_views) return bad("null src_views");
    if (!src_params) return bad("null src_params");
    if (!dst_guides) return bad("null dst_guides");
    if (!dst_views) return bad("null dst_views");
    if (!dst_params) return bad("null dst_params");
    if (!sp) return bad("null sp");
    if (!dst_image) return bad("null dst_image");
    if (!dst_cover) return bad("null dst_cover");
    if (channels != 3u && channels != 4u) return bad("channels must be 3 or 4, not " + std::to_string(channels));
    if (amvpt_status st = synth_params_check(s, sp)) return st;
    if (amvpt_status st = synth_layout(s, "src_params", src_params, A.S)) return st;
    if (amvpt_status st = synth_layout(s, "dst_params", dst_params, A.D)) return st;
    if (A.S.multisensor && A.S.n_views > kMaxSourceViews)
        return bad("src_params: more than 64 source views (n_views is " + std::to_string(A.S.n_views) + ")");
    TemporalLayout &D = A.D;
    if (rect) {
        const uint32_t fw = dst_params->film_width, fh = dst_params->film_height, tw = (uint32_t) D.tw, th = (uint32_t) D.th;
        if (rect[2] == 0 || rect[3] == 0) return bad("rect: zero area");
        if (rect[0] >= fw || rect[2] > fw - rect[0] || rect[1] >= fh || rect[3] > fh - rect[1]) return bad("rect: outside the film");
        if (rect[0] % tw || rect[2] % tw || rect[1] % th || rect[3] % th) return bad("rect: not made of whole tiles");
        D.rx0 = (int32_t) rect[0], D.ry0 = (int32_t) rect[1], D.rw = (int32_t) rect[2], D.rh = (int32_t) rect[3];
    }
    const size_t ncov = (size_t) D.rw * (size_t) D.rh * sizeof(float), nimg = ncov * channels;
    const size_t nsrc = (size_t) A.S.rw * (size_t) A.S.rh * sizeof(float);
    const struct { const void *p; size_t n; const char *name; } in[3] = {
        {src_image, nsrc * channels, "src_image"}, {src_guides, nsrc * 8, "src_guides"}, {dst_guides, ncov * 8, "dst_guides"}};
    for (const auto &i : in) {
        if (sy_overlap(dst_image, nimg, i.p, i.n)) return bad(std::string("dst_image overlaps ") + i.name);
        if (sy_overlap(dst_cover, ncov, i.p, i.n)) return bad(std::string("dst_cover overlaps ") + i.name);
    }
    if (sy_overlap(dst_image, nimg, dst_cover, ncov)) return bad("dst_image overlaps dst_cover");
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
static amvpt_status synth_fill_check(const char *who, const float *image, uint32_t channels, uint32_t w, uint32_t h,
                                     const float *cover, const float *guides, const amvpt_synth_params *sp, const float *out,
                                     const float *scratch, const float *cover_out, const float *cover_scratch) {
    const std::string s = std::string(who) + ": ";
    auto bad = [&](const std::string &what) { set_error(s + what); return AMVPT_ERR_INVALID; };
    if (!image) return bad("null image");
    if (!cover) return bad("null cover");
    if (!guides) return bad("null guides");
    if (!sp) return bad("null sp");
    if (!out) return bad("null out");
    if (!cover_out) return bad("null cover_out");
    if (channels != 3u && channels != 4u) return bad("channels must be 3 or 4, not " + std::to_string(channels));
    /* pixel coordinates are ints, a tap reaches 2 * 128 pixels, and one launch of 32 x 8 tiles covers the image */
    if (w == 0) return bad("width is 0");
    if (h == 0) return bad("height is 0");
    if (w > 0x7fffff00u || h > 0x7fffff00u) return bad("width or height above 2^31 - 256");
    const uint64_t tx = (w + (uint32_t) kTileW - 1u) / (uint32_t) kTileW, ty = (h + (uint32_t) kTileH - 1u) / (uint32_t) kTileH;
    if (tx * ty >= (1ull << 31)) return bad("width x height above 2^31 tiles of 32 x 8 pixels");
    if (amvpt_status st = synth_params_check(s, sp)) return st;
    if (sp->fill_iterations > 1u && !scratch) return bad("null scratch (it may be null only when fill_iterations is at most 1)");
    if (sp->fill_iterations > 1u && !cover_scratch)
        return bad("null cover_scratch (it may be null only when fill_iterations is at most 1)");
    const size_t ncov = (size_t) w * h * sizeof(float), nimg = ncov * channels, ngd = ncov * 8;
    const struct { const void *p; size_t n; const char *name; } outs[4] = {
        {out, nimg, "out"}, {scratch, nimg, "scratch"}, {cover_out, ncov, "cover_out"}, {cover_scratch, ncov, "cover_scratch"}};
    const struct { const void *p; size_t n; const char *name; } ins[3] = {
        {image, nimg, "the image"}, {cover, ncov, "the cover"}, {guides, ngd, "the guides"}};
    for (int i = 0; i < 4; ++i) {
        if (!outs[i].p) continue;
        for (const auto &in : ins)
            if (sy_overlap(outs[i].p, outs[i].n, in.p, in.n)) return bad(std::string(outs[i].name) + " overlaps " + in.name);
        for (int j = 0; j < i; ++j)
            if (outs[j].p && sy_overlap(outs[i].p, outs[i].n, outs[j].p, outs[j].n))
                return bad(std::string(outs[i].name) + " overlaps " + outs[j].name);
    }
    return AMVPT_OK;
}

/* where iteration i of n writes: the two buffers of a pair take turns so that the last iteration lands in the first */
static float *synth_fill_dst(uint32_t i, uint32_t n, float *out, float *scratch) { return ((n - 1u - i) & 1u) ? scratch : out; }

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
    if (amvpt_status s = synth_check("amvpt_synth_host", src_image, channels, src_guides, src_views, src_params, dst_guides,
                                     dst_views, dst_params, rect, sp, dst_image, dst_cover, A))
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
    SynthArgs A;
    if (amvpt_status s = synth_check("amvpt_synth", src_image_device, channels, src_guides_device, src_views, src_params,
                                     dst_guides_device, dst_views, dst_params, rect, sp, dst_image_device, dst_cover_device, A))
        return s;
    /* one launch of 32 x 8 tiles covers the rectangle: film sides are at most 2^24 */
    const uint64_t tx = ((uint32_t) A.D.rw + (uint32_t) kTileW - 1u) / (uint32_t) kTileW;
    const uint64_t ty = ((uint32_t) A.D.rh + (uint32_t) kTileH - 1u) / (uint32_t) kTileH;
    if (tx * ty >= (1ull << 31)) { set_error("amvpt_synth: rect above 2^31 tiles of 32 x 8 pixels"); return AMVPT_ERR_INVALID; }
    if (!synth_device_ok()) { set_error("amvpt_synth: no HIP device visible"); return AMVPT_ERR_NO_DEVICE; }
    hipStream_t st = (hipStream_t) stream;
    const uint32_t ns = A.S.multisensor ? A.S.n_views : 1u, nd = A.D.multisensor ? A.D.n_views : 1u;
    const size_t vbytes = (size_t) ns * sizeof(amvpt_view_desc), obytes = (size_t) nd * 3 * sizeof(float);
    static_assert(sizeof(amvpt_view_desc) % sizeof(float) == 0, "the origins follow the views in one block");
    ViewBuf vb;
    if (amvpt_status rc = view_buf_take("amvpt_synth", vbytes + obytes, vb)) return rc;
    std::memcpy(vb.host, src_views, vbytes);
    synth_origins(dst_views, nd, (float *) ((char *) vb.host + vbytes));
    hipError_t e = hipMemcpyAsync(vb.p, vb.host, vbytes + obytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        A.src_views = (const amvpt_view_desc *) vb.p;
        A.dst_origins = (const float *) ((const char *) vb.p + vbytes);
        A.tiles_x = (uint32_t) tx;
        hipLaunchKernelGGL(k_synth, dim3((uint32_t) (tx * ty)), dim3(kSynthBlock), 0, st, A);
        e = hipGetLastError();
    }
    const hipError_t eg = view_buf_give(vb, st);
    if (e != hipSuccess) return hip_fail("amvpt_synth launch", (int) e);
    if (eg != hipSuccess) return hip_fail("amvpt_synth hipEventRecord", (int) eg);
    return AMVPT_OK;
}

amvpt_status amvpt_synth_fill_host(const float *image, uint32_t channels, uint32_t width, uint32_t height,
                                   const float *cover, const float *guides, const amvpt_synth_params *sp, float *out,
                                   float *scratch, float *cover_out, float *cover_scratch) {
    if (amvpt_status s = synth_fill_check("amvpt_synth_fill_host", image, channels, width, height, cover, guides, sp, out, scratch,
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
        float *dst = synth_fill_dst(i, n, out, scratch), *cdst = synth_fill_dst(i, n, cover_out, cover_scratch);
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
    if (amvpt_status s = synth_fill_check("amvpt_synth_fill", image_device, channels, width, height, cover_device, guides_device, sp,
                                          out_device, scratch_device, cover_out_device, cover_scratch_device))
        return s;
    if (!synth_device_ok()) { set_error("amvpt_synth_fill: no HIP device visible"); return AMVPT_ERR_NO_DEVICE; }
    hipStream_t st = (hipStream_t) stream;
    const size_t npx = (size_t) width * height;
    const uint32_t n = sp->fill_iterations;
    if (n == 0) {
        hipError_t e = hipMemcpyAsync(out_device, image_device, npx * channels * sizeof(float), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(cover_out_device, cover_device, npx * sizeof(float), hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) return hip_fail("amvpt_synth_fill copy", (int) e);
        return AMVPT_OK;
    }
    const uint32_t tx = (width + (uint32_t) kTileW - 1u) / (uint32_t) kTileW, ty = (height + (uint32_t) kTileH - 1u) / (uint32_t) kTileH;
    const float *in = image_device, *cin = cover_device;
    for (uint32_t i = 0; i < n; ++i) {
        float *dst = synth_fill_dst(i, n, out_device, scratch_device), *cdst = synth_fill_dst(i, n, cover_out_device, cover_scratch_device);
        const SynthFillArgs A{in, cin, guides_device, dst, cdst, channels, width, height, tx, (int32_t) (1u << i), sp->plane_tol,
                              sp->normal_cos};
        hipLaunchKernelGGL(k_synth_fill, dim3(tx * ty), dim3(kSynthBlock), 0, st, A);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail("amvpt_synth_fill launch", (int) e);
        in = dst, cin = cdst;
    }
    return AMVPT_OK;
}

} // extern "C"

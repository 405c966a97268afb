/*
 * amvpt_guides.hip -- the entries of include/amvpt_guides.h.  amvpt_guides itself is k_guides of amvpt_render.hip
 * (it shares the render's raygen, walk and surface interaction: guides_impl); this unit holds the depth planes:
 * k_guide_depth (records -> planar z), k_depth_range (wave reduce, then one unsigned atomic min and max per wave)
 * and k_depth8 (z -> 8-bit quilt, four pixels = 12 bytes = three dword stores per thread, as k_srgb8).  Streaming
 * kernels over a flat pixel index; no LDS, no device-wide synchronisation; everything is ordered on the caller's
 * stream.  The per-element functions are dguides.h's, shared with the host-only entries below.
 */
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/amvpt_guides.h"
#include "dguides.h"
#include "internal.h"
#include "post_host.h"

namespace amvpt {

static constexpr uint32_t kGuideBlock = 256;
/* rows of to_world_inv that travel in one launch's kernel arguments (2 KiB); a longer view table takes a launch per
 * window of views, each writing the pixels of its views */
static constexpr uint32_t kViewWin = 128;
struct ViewRows { float row[kViewWin][4]; };

__global__ void __launch_bounds__(kGuideBlock) k_guide_depth(const float *__restrict__ guides, float *__restrict__ depth,
                                                             uint64_t n, uint32_t n_views, uint32_t v0, ViewRows R) {
    const uint64_t i = (uint64_t) blockIdx.x * kGuideBlock + threadIdx.x;
    if (i >= n) return;
    float rec[8];   /* merged into two 16-byte loads; a record needs no more than a float's alignment */
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) rec[k] = guides[8 * i + k];
    const uint32_t view = guide_view(rec, n_views);
    if (!guide_hit(rec) || view >= n_views) {
        if (v0 == 0u) depth[i] = ginf();   /* a miss, or a view outside the table: the first window writes it */
        return;
    }
    const uint32_t k = view - v0;          /* wraps for the views below the window */
    if (k < kViewWin) depth[i] = guide_depth_value(rec, R.row[k]);
}

/* grid-stride, so that every lane of every wave reaches the reduce; mm[0] = minimum key, mm[1] = maximum key */
__global__ void __launch_bounds__(kGuideBlock) k_depth_range(const float *__restrict__ depth, uint64_t n, uint32_t *mm) {
    uint32_t lo = kDepthKeyMin0, hi = kDepthKeyMax0;
    const uint64_t stride = (uint64_t) gridDim.x * kGuideBlock;
    for (uint64_t i = (uint64_t) blockIdx.x * kGuideBlock + threadIdx.x; i < n; i += stride) {
        const float z = depth[i];
        if (gfinite(z)) {
            const uint32_t k = depth_key(z);
            lo = k < lo ? k : lo;
            hi = k > hi ? k : hi;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t l2 = (uint32_t) __shfl_xor((int) lo, off, 64), h2 = (uint32_t) __shfl_xor((int) hi, off, 64);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if ((threadIdx.x & 63u) == 0u && hi >= lo) {   /* a wave without a finite value adds nothing */
        atomicMin(mm, lo);
        atomicMax(mm + 1, hi);
    }
}

static constexpr uint32_t kPxPerThread = 4;
/* kDword: `out` is 4-byte aligned (three dword stores for four pixels); else byte stores */
template <bool kDword>
__global__ void __launch_bounds__(kGuideBlock) k_depth8(const float *__restrict__ depth, uint8_t *__restrict__ out,
                                                        uint64_t npx, Depth8Params P) {
    const uint64_t p0 = ((uint64_t) blockIdx.x * kGuideBlock + threadIdx.x) * kPxPerThread;
    if (p0 >= npx) return;
    uint8_t *dst = out + p0 * 3;
    if (p0 + kPxPerThread <= npx) {
        uint32_t c[kPxPerThread];
#pragma unroll
        for (uint32_t i = 0; i < kPxPerThread; ++i) c[i] = depth8_value(depth[p0 + i], P);
        if (kDword) {
            uint32_t *o = reinterpret_cast<uint32_t *>(dst);   /* p0 * 3 is a multiple of 4 */
            o[0] = c[0] * 0x010101u | c[1] << 24;
            o[1] = c[1] * 0x0101u | c[2] * 0x01010000u;
            o[2] = c[2] | c[3] * 0x01010100u;
        } else {
#pragma unroll
            for (uint32_t i = 0; i < kPxPerThread; ++i) dst[3 * i] = dst[3 * i + 1] = dst[3 * i + 2] = (uint8_t) c[i];
        }
        return;
    }
    /* the last thread of the image: one to three pixels, stored as bytes */
    for (uint64_t p = p0; p < npx; ++p, dst += 3) dst[0] = dst[1] = dst[2] = depth8_value(depth[p], P);
}

/* one launch covers the plane: HIP refuses a grid of 2^32 threads or more */
static constexpr uint64_t kMaxGuidePixels = 1ull << 31;

static amvpt_status depth_check(const char *who, const float *guides, const amvpt_view_desc *views, uint32_t n_views,
                                const float *depth) {
    const std::string s = std::string(who) + ": ";
    if (!guides) { set_error(s + "null guides"); return AMVPT_ERR_INVALID; }
    if (!views) { set_error(s + "null views"); return AMVPT_ERR_INVALID; }
    if (n_views == 0) { set_error(s + "n_views is 0"); return AMVPT_ERR_INVALID; }
    if (!depth) { set_error(s + "null depth"); return AMVPT_ERR_INVALID; }
    return AMVPT_OK;
}

static amvpt_status depth8_check(const char *who, const float *depth, uint32_t w, uint32_t h, float near, float far,
                                 const uint8_t *out, Depth8Params &P) {
    const std::string s = std::string(who) + ": ";
    if (!depth) { set_error(s + "null depth"); return AMVPT_ERR_INVALID; }
    if (!out) { set_error(s + "null out"); return AMVPT_ERR_INVALID; }
    if (w == 0) { set_error(s + "w is 0"); return AMVPT_ERR_INVALID; }
    if (h == 0) { set_error(s + "h is 0"); return AMVPT_ERR_INVALID; }
    if (!gfinite(near)) { set_error(s + "near is not finite"); return AMVPT_ERR_INVALID; }
    if (!gfinite(far)) { set_error(s + "far is not finite"); return AMVPT_ERR_INVALID; }
    if (far < near) { set_error(s + "far is below near"); return AMVPT_ERR_INVALID; }
    P.far_ = far;
    P.span = far - near;
    return AMVPT_OK;
}

} // namespace amvpt

using namespace amvpt;

extern "C" {

uint32_t amvpt_guides_version(void) { return AMVPT_GUIDES_VERSION; }

amvpt_status amvpt_guides(amvpt_scene *scene, const amvpt_view_desc *views, const amvpt_params *params,
                          const uint32_t rect[4], float *out_device, void *stream) {
    if (!device_ok()) { set_error("amvpt_guides: no HIP device visible"); return AMVPT_ERR_NO_DEVICE; }
    return guides_impl(scene, views, params, rect, out_device, stream);
}

amvpt_status amvpt_guide_depth_host(const float *guides, const amvpt_view_desc *views, uint32_t n_views,
                                    uint64_t n_pixels, float *depth) {
    if (amvpt_status s = depth_check("amvpt_guide_depth_host", guides, views, n_views, depth)) return s;
    for (uint64_t i = 0; i < n_pixels; ++i)
        if (guide_view(guides + 8 * i, n_views) >= n_views) {
            set_error("amvpt_guide_depth_host: guides: the view index of pixel " + std::to_string(i) + " is not below n_views (" +
                      std::to_string(n_views) + ")");
            return AMVPT_ERR_INVALID;
        }
    for (uint64_t i = 0; i < n_pixels; ++i) {
        const float *rec = guides + 8 * i;
        depth[i] = guide_hit(rec) ? guide_depth_value(rec, views[guide_view(rec, n_views)].to_world_inv + 8) : ginf();
    }
    return AMVPT_OK;
}

amvpt_status amvpt_guide_depth(const float *guides_device, const amvpt_view_desc *views, uint32_t n_views,
                               uint64_t n_pixels, float *depth_device, void *stream) {
    if (amvpt_status s = depth_check("amvpt_guide_depth", guides_device, views, n_views, depth_device)) return s;
    if (n_pixels > kMaxGuidePixels) { set_error("amvpt_guide_depth: n_pixels above 2^31"); return AMVPT_ERR_INVALID; }
    if (!device_ok()) { set_error("amvpt_guide_depth: no HIP device visible"); return AMVPT_ERR_NO_DEVICE; }
    if (n_pixels == 0) return AMVPT_OK;
    const dim3 grid((uint32_t) ((n_pixels + kGuideBlock - 1) / kGuideBlock)), block(kGuideBlock);
    hipStream_t st = (hipStream_t) stream;
    for (uint32_t v0 = 0; v0 < n_views; v0 += kViewWin) {
        ViewRows R;
        for (uint32_t k = 0; k < kViewWin; ++k)
            for (uint32_t j = 0; j < 4; ++j) R.row[k][j] = v0 + k < n_views ? views[v0 + k].to_world_inv[8 + j] : 0.f;
        hipLaunchKernelGGL(k_guide_depth, grid, block, 0, st, guides_device, depth_device, n_pixels, n_views, v0, R);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail("amvpt_guide_depth launch", (int) e);
    }
    return AMVPT_OK;
}

amvpt_status amvpt_guide_depth_range_host(const float *depth, uint64_t n, float near_far[2]) {
    if (n && !depth) { set_error("amvpt_guide_depth_range_host: null depth"); return AMVPT_ERR_INVALID; }
    if (!near_far) { set_error("amvpt_guide_depth_range_host: null near_far"); return AMVPT_ERR_INVALID; }
    uint32_t lo = kDepthKeyMin0, hi = kDepthKeyMax0;
    for (uint64_t i = 0; i < n; ++i)
        if (gfinite(depth[i])) {
            const uint32_t k = depth_key(depth[i]);
            lo = k < lo ? k : lo;
            hi = k > hi ? k : hi;
        }
    near_far[0] = hi >= lo ? depth_unkey(lo) : 0.f;
    near_far[1] = hi >= lo ? depth_unkey(hi) : 0.f;
    return AMVPT_OK;
}

amvpt_status amvpt_guide_depth_range(const float *depth_device, uint64_t n, float near_far_host[2], void *stream) {
    if (n && !depth_device) { set_error("amvpt_guide_depth_range: null depth"); return AMVPT_ERR_INVALID; }
    if (!near_far_host) { set_error("amvpt_guide_depth_range: null near_far_host"); return AMVPT_ERR_INVALID; }
    if (!device_ok()) { set_error("amvpt_guide_depth_range: no HIP device visible"); return AMVPT_ERR_NO_DEVICE; }
    hipStream_t st = (hipStream_t) stream;
    uint32_t mm[2] = {kDepthKeyMin0, kDepthKeyMax0};
    if (n) {
        /* the two keys the waves reduce into: 8 bytes for the length of the call */
        uint32_t *d = nullptr;
        hipError_t e = hipMalloc(&d, sizeof(mm));
        if (e != hipSuccess) return hip_fail("amvpt_guide_depth_range hipMalloc", (int) e);
        e = hipMemcpyAsync(d, mm, sizeof(mm), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) {
            /* 4096 blocks of grid-stride loops cover any plane */
            const uint64_t want = (n + kGuideBlock - 1) / kGuideBlock;
            hipLaunchKernelGGL(k_depth_range, dim3((uint32_t) (want < 4096 ? want : 4096)), dim3(kGuideBlock), 0, st,
                               depth_device, n, d);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(mm, d, sizeof(mm), hipMemcpyDeviceToHost, st);
        const hipError_t es = hipStreamSynchronize(st);   /* also before the free on an error path */
        (void) hipFree(d);
        if (e != hipSuccess) return hip_fail("amvpt_guide_depth_range", (int) e);
        if (es != hipSuccess) return hip_fail("amvpt_guide_depth_range hipStreamSynchronize", (int) es);
    } else {
        const hipError_t es = hipStreamSynchronize(st);
        if (es != hipSuccess) return hip_fail("amvpt_guide_depth_range hipStreamSynchronize", (int) es);
    }
    near_far_host[0] = mm[1] >= mm[0] ? depth_unkey(mm[0]) : 0.f;
    near_far_host[1] = mm[1] >= mm[0] ? depth_unkey(mm[1]) : 0.f;
    return AMVPT_OK;
}

amvpt_status amvpt_depth8_host(const float *depth, uint32_t w, uint32_t h, float near, float far, uint8_t *out) {
    Depth8Params P;
    if (amvpt_status s = depth8_check("amvpt_depth8_host", depth, w, h, near, far, out, P)) return s;
    const size_t npx = (size_t) w * h;
    for (size_t p = 0; p < npx; ++p) out[3 * p] = out[3 * p + 1] = out[3 * p + 2] = depth8_value(depth[p], P);
    return AMVPT_OK;
}

amvpt_status amvpt_depth8(const float *depth_device, uint32_t w, uint32_t h, float near, float far, uint8_t *out_device,
                          void *stream) {
    Depth8Params P;
    if (amvpt_status s = depth8_check("amvpt_depth8", depth_device, w, h, near, far, out_device, P)) return s;
    const uint64_t npx = (uint64_t) w * h;
    if (npx > 4 * kMaxGuidePixels) { set_error("amvpt_depth8: w * h above 2^33 pixels"); return AMVPT_ERR_INVALID; }
    if (!device_ok()) { set_error("amvpt_depth8: no HIP device visible"); return AMVPT_ERR_NO_DEVICE; }
    const uint64_t per = (uint64_t) kGuideBlock * kPxPerThread;
    const dim3 grid((uint32_t) ((npx + per - 1) / per)), block(kGuideBlock);
    hipStream_t st = (hipStream_t) stream;
    if (((uintptr_t) out_device & 3u) == 0) hipLaunchKernelGGL((k_depth8<true>), grid, block, 0, st, depth_device, out_device, npx, P);
    else hipLaunchKernelGGL((k_depth8<false>), grid, block, 0, st, depth_device, out_device, npx, P);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail("amvpt_depth8 launch", (int) e);
    return AMVPT_OK;
}

} // extern "C"

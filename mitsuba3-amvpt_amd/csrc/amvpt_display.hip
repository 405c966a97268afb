/*
 * amvpt_display.hip -- the display stage (include/amvpt_display.h): k_srgb8 turns the developed float32 quilt
 * into 8-bit sRGB, k_interlace gathers that quilt into the native image of a lenticular display.  Both are
 * streaming kernels over a flat pixel index, four pixels = 12 bytes = three dword stores per thread, so a row
 * pitch (3W) that is no multiple of 4 needs no special case: only the last thread of the image can hold fewer
 * than four pixels, and it stores bytes.  A destination that is not dword-aligned (or, for k_srgb8, a source that
 * is not 16-byte aligned) takes the byte-store / scalar-load instance of the same kernel.  No LDS, no atomics, no
 * device-wide synchronisation; everything is ordered on the caller's stream.  The per-element functions are
 * ddisplay.h's, shared with the host-only entries below.
 */
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/amvpt_display.h"
#include "ddisplay.h"
#include "internal.h"
#include "post_host.h"

namespace amvpt {

static constexpr uint32_t kDisplayBlock = 256;
static constexpr uint32_t kPxPerThread = 4;

/* kVec: `in` is 16-byte and `out` 4-byte aligned (whole float4 loads, dword stores) */
template <uint32_t kCh, bool kVec>
__global__ void __launch_bounds__(kDisplayBlock) k_srgb8(const float *__restrict__ in, uint8_t *__restrict__ out,
                                                          uint64_t npx) {
    const uint64_t p0 = ((uint64_t) blockIdx.x * kDisplayBlock + threadIdx.x) * kPxPerThread;
    if (p0 >= npx) return;
    const float *src = in + p0 * kCh;
    uint8_t *dst = out + p0 * 3;
    if (p0 + kPxPerThread <= npx) {
        float f[kPxPerThread * kCh];
        if (kVec) {
            const float4 *s4 = reinterpret_cast<const float4 *>(src);   /* p0 * kCh * 4 B is a multiple of 16 */
#pragma unroll
            for (uint32_t i = 0; i < kCh; ++i) {
                const float4 q = s4[i];
                f[4 * i] = q.x, f[4 * i + 1] = q.y, f[4 * i + 2] = q.z, f[4 * i + 3] = q.w;
            }
        } else {
#pragma unroll
            for (uint32_t i = 0; i < kPxPerThread * kCh; ++i) f[i] = src[i];
        }
        uint8_t v[12];
#pragma unroll
        for (uint32_t i = 0; i < kPxPerThread; ++i)
            for (uint32_t c = 0; c < 3; ++c) v[3 * i + c] = srgb8_value(f[i * kCh + c]);
        store12<kVec>(dst, v);
        return;
    }
    for (uint64_t p = p0; p < npx; ++p, src += kCh, dst += 3)
        for (uint32_t c = 0; c < 3; ++c) dst[c] = srgb8_value(src[c]);
}

template <bool kDword>
__global__ void __launch_bounds__(kDisplayBlock) k_interlace(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                              DisplayParams P) {
    const uint64_t npx = (uint64_t) P.dw * P.dh;
    const uint64_t p0 = ((uint64_t) blockIdx.x * kDisplayBlock + threadIdx.x) * kPxPerThread;
    if (p0 >= npx) return;
    uint32_t dy = (uint32_t) (p0 / P.dw);
    uint32_t px = (uint32_t) (p0 - (uint64_t) dy * P.dw);
    uint8_t *out = dst + p0 * 3;
    if (p0 + kPxPerThread <= npx) {
        uint8_t v[12];
#pragma unroll
        for (uint32_t i = 0; i < kPxPerThread; ++i) {
#pragma unroll
            for (uint32_t c = 0; c < 3; ++c) v[3 * i + c] = interlace_value(src, P, px, dy, c);
            if (++px == P.dw) px = 0, ++dy;   /* the four pixels may straddle a row end */
        }
        store12<kDword>(out, v);
        return;
    }
    /* the last thread of the image: one to three pixels, stored as bytes */
    for (uint64_t p = p0; p < npx; ++p, out += 3) {
        for (uint32_t c = 0; c < 3; ++c) out[c] = interlace_value(src, P, px, dy, c);
        if (++px == P.dw) px = 0, ++dy;
    }
}

static bool finite_preset(const amvpt_display_preset &p, const char *&field) {
    const float v[7] = {p.center, p.focus, p.pitch, p.tilt, p.subp, p.view[0], p.view[1]};
    static const char *const names[7] = {"center", "focus", "pitch", "tilt", "subp", "view[0]", "view[1]"};
    for (int i = 0; i < 7; ++i)
        if (!std::isfinite(v[i])) { field = names[i]; return false; }
    return true;
}

/* the argument checks of amvpt_interlace* and display_image's loop invariants; src / dst null checks are the caller's */
static amvpt_status display_params(const char *who, uint32_t sw, uint32_t sh, uint32_t nch,
                                   const amvpt_display_preset *p, int quilt, int nearest, uint32_t dw, uint32_t dh,
                                   DisplayParams &P) {
    const std::string w = std::string(who) + ": ";
    if (!p) { set_error(w + "null preset"); return AMVPT_ERR_INVALID; }
    if (dw < 2) { set_error(w + "dst_w must be at least 2 (the reference divides by 3 * dst_w - 1 and dst_h - 1)"); return AMVPT_ERR_INVALID; }
    if (dh < 2) { set_error(w + "dst_h must be at least 2 (the reference divides by 3 * dst_w - 1 and dst_h - 1)"); return AMVPT_ERR_INVALID; }
    if (dw > 0xffffffffu / 3u) { set_error(w + "dst_w too large (3 * dst_w must fit 32 bits)"); return AMVPT_ERR_INVALID; }
    if (sw == 0) { set_error(w + "src_w is 0"); return AMVPT_ERR_INVALID; }
    if (sh == 0) { set_error(w + "src_h is 0"); return AMVPT_ERR_INVALID; }
    if (nch != 3 && nch != 4) { set_error(w + "src_channels must be 3 or 4, not " + std::to_string(nch)); return AMVPT_ERR_INVALID; }
    for (int i = 0; i < 2; ++i)
        if (p->grid[i] < 1) {
            set_error(w + "grid[" + std::to_string(i) + "] must be at least 1, not " + std::to_string(p->grid[i]));
            return AMVPT_ERR_INVALID;
        }
    if ((int64_t) p->grid[0] * p->grid[1] > INT32_MAX) { set_error(w + "grid[0] * grid[1] overflows"); return AMVPT_ERR_INVALID; }
    const char *field = nullptr;
    if (!finite_preset(*p, field)) { set_error(w + "preset " + field + " is not finite"); return AMVPT_ERR_INVALID; }
    P.center = p->center, P.focus = p->focus, P.pitch = p->pitch, P.tilt = p->tilt, P.subp = p->subp;
    P.gx = (float) p->grid[0];
    P.grid_n = (float) (p->grid[0] * p->grid[1]);
    P.grid_scl = 1.f / P.grid_n;
    P.igx = 1.f / (float) p->grid[0];
    P.vix = p->view[0] * P.igx;
    P.viy = p->view[1] * (1.f / (float) p->grid[1]);
    P.dsx = 1.f / ((float) (3u * dw) - 1.f);
    P.dsy = 1.f / ((float) dh - 1.f);
    P.ssx = (float) sw - 1.f;
    P.ssy = (float) sh - 1.f;
    P.sw = sw, P.sh = sh, P.nch = nch, P.dw = dw, P.dh = dh;
    P.quilt = quilt ? 1u : 0u, P.nearest = nearest ? 1u : 0u;
    return AMVPT_OK;
}

static amvpt_status srgb8_check(const char *who, const void *in, uint32_t ch, uint32_t w, uint32_t h, const void *out) {
    const std::string s = std::string(who) + ": ";
    if (!in) { set_error(s + "null image"); return AMVPT_ERR_INVALID; }
    if (!out) { set_error(s + "null out"); return AMVPT_ERR_INVALID; }
    if (ch != 3 && ch != 4) { set_error(s + "channels must be 3 or 4, not " + std::to_string(ch)); return AMVPT_ERR_INVALID; }
    if (w == 0) { set_error(s + "width is 0"); return AMVPT_ERR_INVALID; }
    if (h == 0) { set_error(s + "height is 0"); return AMVPT_ERR_INVALID; }
    return AMVPT_OK;
}

/* one launch covers the image: HIP refuses a grid of 2^32 threads or more, so an image is held to 2^33 pixels
 * (2^23 blocks of 256 threads, four pixels each) and a larger one is refused by name before the launch */
static constexpr uint64_t kMaxDisplayPixels = 1ull << 33;
static uint32_t display_blocks(uint64_t npx) {
    const uint64_t per = (uint64_t) kDisplayBlock * kPxPerThread;
    return (uint32_t) ((npx + per - 1) / per);
}

} // namespace amvpt

using namespace amvpt;

extern "C" {

uint32_t amvpt_display_version(void) { return AMVPT_DISPLAY_VERSION; }

amvpt_display_preset amvpt_display_default_preset(void) {
    amvpt_display_preset p;
    p.center = -0.5f, p.focus = -0.05f, p.pitch = 354.548f, p.tilt = -0.114f, p.subp = 0.00013f;
    p.view[0] = p.view[1] = 1.f;
    p.grid[0] = 4, p.grid[1] = 8;
    p.flip_rgb = 0;
    return p;
}

amvpt_status amvpt_srgb8_host(const float *image, uint32_t channels, uint32_t width, uint32_t height, uint8_t *out) {
    if (amvpt_status s = srgb8_check("amvpt_srgb8_host", image, channels, width, height, out)) return s;
    const size_t npx = (size_t) width * height;
    for (size_t p = 0; p < npx; ++p)
        for (uint32_t c = 0; c < 3; ++c) out[p * 3 + c] = srgb8_value(image[p * channels + c]);
    return AMVPT_OK;
}

amvpt_status amvpt_srgb8(const float *image, uint32_t channels, uint32_t width, uint32_t height, uint8_t *out,
                         void *stream) {
    if (amvpt_status s = srgb8_check("amvpt_srgb8", image, channels, width, height, out)) return s;
    const uint64_t npx = (uint64_t) width * height;
    if (npx > kMaxDisplayPixels) { set_error("amvpt_srgb8: width * height above 2^33 pixels"); return AMVPT_ERR_INVALID; }
    if (!device_ok()) { set_error("amvpt_srgb8: no HIP device visible"); return AMVPT_ERR_NO_DEVICE; }
    const bool vec = ((uintptr_t) image & 15u) == 0 && ((uintptr_t) out & 3u) == 0;
    const dim3 grid(display_blocks(npx)), block(kDisplayBlock);
    hipStream_t st = (hipStream_t) stream;
    if (channels == 3) {
        if (vec) hipLaunchKernelGGL((k_srgb8<3, true>), grid, block, 0, st, image, out, npx);
        else hipLaunchKernelGGL((k_srgb8<3, false>), grid, block, 0, st, image, out, npx);
    } else {
        if (vec) hipLaunchKernelGGL((k_srgb8<4, true>), grid, block, 0, st, image, out, npx);
        else hipLaunchKernelGGL((k_srgb8<4, false>), grid, block, 0, st, image, out, npx);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail("amvpt_srgb8 launch", (int) e);
    return AMVPT_OK;
}

amvpt_status amvpt_interlace_host(const uint8_t *src, uint32_t src_w, uint32_t src_h, uint32_t src_channels,
                                  const amvpt_display_preset *preset, int quilt, int nearest, uint8_t *dst,
                                  uint32_t dst_w, uint32_t dst_h) {
    if (!src) { set_error("amvpt_interlace_host: null src"); return AMVPT_ERR_INVALID; }
    if (!dst) { set_error("amvpt_interlace_host: null dst"); return AMVPT_ERR_INVALID; }
    DisplayParams P;
    if (amvpt_status s = display_params("amvpt_interlace_host", src_w, src_h, src_channels, preset, quilt, nearest,
                                        dst_w, dst_h, P))
        return s;
    for (uint32_t dy = 0; dy < dst_h; ++dy)
        for (uint32_t px = 0; px < dst_w; ++px)
            for (uint32_t c = 0; c < 3; ++c)
                dst[((size_t) dy * dst_w + px) * 3 + c] = interlace_value(src, P, px, dy, c);
    return AMVPT_OK;
}

amvpt_status amvpt_interlace_views_host(const amvpt_display_preset *preset, int32_t *views, uint32_t dst_w,
                                        uint32_t dst_h) {
    if (!views) { set_error("amvpt_interlace_views_host: null views"); return AMVPT_ERR_INVALID; }
    DisplayParams P;
    if (amvpt_status s = display_params("amvpt_interlace_views_host", 1, 1, 3, preset, 0, 0, dst_w, dst_h, P)) return s;
    for (uint32_t dy = 0; dy < dst_h; ++dy)
        for (uint32_t px = 0; px < dst_w; ++px)
            for (uint32_t c = 0; c < 3; ++c) {
                float x, y;
                const float z1 = interlace_coord(P, px, dy, c, x, y);
                views[((size_t) dy * dst_w + px) * 3 + c] = z1 == z1 ? (int32_t) z1 : -1;
            }
    return AMVPT_OK;
}

amvpt_status amvpt_interlace(const uint8_t *src, uint32_t src_w, uint32_t src_h, uint32_t src_channels,
                             const amvpt_display_preset *preset, int quilt, int nearest, uint8_t *dst, uint32_t dst_w,
                             uint32_t dst_h, void *stream) {
    if (!src) { set_error("amvpt_interlace: null src"); return AMVPT_ERR_INVALID; }
    if (!dst) { set_error("amvpt_interlace: null dst"); return AMVPT_ERR_INVALID; }
    DisplayParams P;
    if (amvpt_status s = display_params("amvpt_interlace", src_w, src_h, src_channels, preset, quilt, nearest, dst_w,
                                        dst_h, P))
        return s;
    const uint64_t npx = (uint64_t) dst_w * dst_h;
    if (npx > kMaxDisplayPixels) { set_error("amvpt_interlace: dst_w * dst_h above 2^33 pixels"); return AMVPT_ERR_INVALID; }
    if (!device_ok()) { set_error("amvpt_interlace: no HIP device visible"); return AMVPT_ERR_NO_DEVICE; }
    const dim3 grid(display_blocks(npx)), block(kDisplayBlock);
    hipStream_t st = (hipStream_t) stream;
    if (((uintptr_t) dst & 3u) == 0) hipLaunchKernelGGL((k_interlace<true>), grid, block, 0, st, src, dst, P);
    else hipLaunchKernelGGL((k_interlace<false>), grid, block, 0, st, src, dst, P);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail("amvpt_interlace launch", (int) e);
    return AMVPT_OK;
}

} // extern "C"

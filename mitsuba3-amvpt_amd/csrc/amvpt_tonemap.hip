/*
 * amvpt_tonemap.hip -- the tone-mapping stage (include/amvpt_tonemap.h): k_tonemap_hist meters the developed quilt
 * into a log-luminance histogram, k_exposure turns the histogram into the exposure of this frame, k_tonemap scales
 * every pixel by it, applies the operator and writes floats or, fused with amvpt_srgb8's curve, sRGB bytes.  All
 * three are ordered on the caller's stream and nothing returns to the host between them.  The streaming kernels have
 * k_srgb8's shape: a flat pixel index, four pixels per thread, float4 loads where the source is 16-byte aligned and a
 * scalar-load instance where it is not.  The per-pixel functions are dtonemap.h's, shared with the host-only entries
 * below.
 *
 * The histogram: one block keeps a histogram of 512 bins and the skipped count in LDS, a
 * wave merges the lanes that share its first lane's bin into one integer add and the other lanes add for themselves;
 * after the block's last pixel every non-zero LDS count is added to the state with one integer atomic.  No block waits
 * for another: the stream orders k_exposure behind the last of them.
 */
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/amvpt_tonemap.h"
#include "dtonemap.h"
#include "internal.h"
#include "post_host.h"

namespace amvpt {

static constexpr uint32_t kTmBlock = 256;
static constexpr uint32_t kTmPx = 4;                  /* pixels per thread and round */
static constexpr uint32_t kHistMaxBlocks = 1024;      /* four blocks on each of 256 compute units */
static constexpr uint32_t kHistSlots = kTmBins + 1;   /* the bins, and the skipped pixels in slot 512 */

struct HistArgs {
    const float *in;      /* the first metered pixel */
    uint64_t npx;         /* metered pixels */
    uint32_t rw, pitch;   /* kRect: the rectangle's width and the image's, in pixels */
    amvpt_tonemap_state *state;
};

static __device__ __forceinline__ uint32_t hist_slot(const float *c) {
    const int32_t b = tm_bin(pp_lum(c));
    return b == kTmSkipped ? kTmBins : (uint32_t) b;
}

/* one pixel of every active lane into the LDS histogram h: the lanes in the bin of the wave's first active lane become
 * one add of their number (a frame of one bin is one add per wave instead of 64 on one word), the others add for
 * themselves */
static __device__ __forceinline__ void hist_add(uint32_t *h, uint32_t slot) {
    const uint32_t lead = (uint32_t) __builtin_amdgcn_readfirstlane((int) slot);
    const uint64_t same = __ballot(slot == lead);
    if (slot != lead) atomicAdd(&h[slot], 1u);
    else if ((uint32_t) __lane_id() == (uint32_t) __ffsll((unsigned long long) same) - 1u)
        atomicAdd(&h[lead], (uint32_t) __popcll(same));
}

/* kVec: A.in is 16-byte aligned (whole float4 loads); kRect: the metered pixels are a rectangle narrower than the
 * image, pixel p of it lies at row p / rw, column p % rw */
template <uint32_t kCh, bool kVec, bool kRect>
__global__ void __launch_bounds__(kTmBlock) k_tonemap_hist(HistArgs A) {
    __shared__ uint32_t h[kHistSlots];
    for (uint32_t i = threadIdx.x; i < kHistSlots; i += kTmBlock) h[i] = 0;
    __syncthreads();
    const uint64_t stride = (uint64_t) gridDim.x * kTmBlock * kTmPx;
    for (uint64_t p0 = ((uint64_t) blockIdx.x * kTmBlock + threadIdx.x) * kTmPx; p0 < A.npx; p0 += stride) {
        if (!kRect && p0 + kTmPx <= A.npx) {
            const float *src = A.in + p0 * kCh;
            float f[kTmPx * kCh];
            if (kVec) {
                const float4 *s4 = reinterpret_cast<const float4 *>(src);   /* p0 * kCh * 4 B is a multiple of 16 */
#pragma unroll
                for (uint32_t i = 0; i < kCh; ++i) {
                    const float4 q = s4[i];
                    f[4 * i] = q.x, f[4 * i + 1] = q.y, f[4 * i + 2] = q.z, f[4 * i + 3] = q.w;
                }
            } else {
#pragma unroll
                for (uint32_t i = 0; i < kTmPx * kCh; ++i) f[i] = src[i];
            }
#pragma unroll
            for (uint32_t i = 0; i < kTmPx; ++i) hist_add(h, hist_slot(f + i * kCh));
        } else {
            /* a rectangle's pixels, or the last one to three of the image */
            const uint64_t pe = p0 + kTmPx < A.npx ? p0 + kTmPx : A.npx;
            for (uint64_t p = p0; p < pe; ++p) {
                const uint64_t at = kRect ? (p / A.rw) * A.pitch + p % A.rw : p;
                hist_add(h, hist_slot(A.in + at * kCh));
            }
        }
    }
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < kHistSlots; s += kTmBlock) {
        const uint32_t n = h[s];
        if (n) atomicAdd(s < kTmBins ? &A.state->hist[s] : &A.state->skipped, n);
    }
}

/* one block: the histogram into LDS, then the serial definition on one lane */
__global__ void __launch_bounds__(kTmBins) k_exposure(amvpt_tonemap_state *state, amvpt_tonemap_params q) {
    __shared__ uint32_t h[kTmBins];
    h[threadIdx.x] = state->hist[threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) tm_exposure(h, q, state);
}

struct TonemapArgs {
    const float *in;
    void *out;                          /* kBytes: npx x 3 uint8, else npx x kCh float32; may be `in` itself */
    uint64_t npx;
    const amvpt_tonemap_state *state;   /* null: `exposure` is used */
    float exposure;
    TonemapOp op;
};

/* kVec: `in` is 16-byte aligned and `out` 4-byte (bytes) or 16-byte (floats) aligned */
template <uint32_t kCh, bool kVec, bool kBytes>
__global__ void __launch_bounds__(kTmBlock) k_tonemap(TonemapArgs A) {
    const uint64_t p0 = ((uint64_t) blockIdx.x * kTmBlock + threadIdx.x) * kTmPx;
    if (p0 >= A.npx) return;
    const float ex = A.state ? A.state->exposure : A.exposure;
    const float *src = A.in + p0 * kCh;
    uint8_t *dst8 = static_cast<uint8_t *>(A.out) + p0 * 3;
    float *dstf = static_cast<float *>(A.out) + p0 * kCh;
    if (p0 + kTmPx <= A.npx) {
        float f[kTmPx * kCh];
        if (kVec) {
            const float4 *s4 = reinterpret_cast<const float4 *>(src);
#pragma unroll
            for (uint32_t i = 0; i < kCh; ++i) {
                const float4 q = s4[i];
                f[4 * i] = q.x, f[4 * i + 1] = q.y, f[4 * i + 2] = q.z, f[4 * i + 3] = q.w;
            }
        } else {
#pragma unroll
            for (uint32_t i = 0; i < kTmPx * kCh; ++i) f[i] = src[i];
        }
        uint8_t v[12];
#pragma unroll
        for (uint32_t i = 0; i < kTmPx; ++i) {
            float y[3];
            tm_pixel(f + i * kCh, ex, A.op, y);
#pragma unroll
            for (uint32_t c = 0; c < 3; ++c) {
                if (kBytes) v[3 * i + c] = srgb8_value(y[c]);
                else f[i * kCh + c] = y[c];   /* a fourth channel stays as loaded */
            }
        }
        if (kBytes) {
            store12<kVec>(dst8, v);
        } else if (kVec) {
            float4 *d4 = reinterpret_cast<float4 *>(dstf);
#pragma unroll
            for (uint32_t i = 0; i < kCh; ++i) d4[i] = make_float4(f[4 * i], f[4 * i + 1], f[4 * i + 2], f[4 * i + 3]);
        } else {
#pragma unroll
            for (uint32_t i = 0; i < kTmPx * kCh; ++i) dstf[i] = f[i];
        }
        return;
    }
    /* the last thread of the image: one to three pixels, stored one value at a time */
    for (uint64_t p = p0; p < A.npx; ++p, src += kCh, dst8 += 3, dstf += kCh) {
        float y[3];
        tm_pixel(src, ex, A.op, y);
        const float alpha = kCh == 4 ? src[kCh - 1] : 0.f;
        for (uint32_t c = 0; c < 3; ++c) {
            if (kBytes) dst8[c] = srgb8_value(y[c]);
            else dstf[c] = y[c];
        }
        if (!kBytes && kCh == 4) dstf[3] = alpha;
    }
}

static amvpt_status params_check(const Refusal &R, const amvpt_tonemap_params &q) {
    if (q.op != AMVPT_TONEMAP_LINEAR && q.op != AMVPT_TONEMAP_REINHARD && q.op != AMVPT_TONEMAP_ACES)
        return R.bad("params: unknown op " + std::to_string(q.op));
    const float v[8] = {q.ev, q.key, q.lo, q.hi, q.adapt, q.white, q.min_ev, q.max_ev};
    static const char *const names[8] = {"ev", "key", "lo", "hi", "adapt", "white", "min_ev", "max_ev"};
    for (int i = 0; i < 8; ++i)
        if (!pp_finite(v[i])) return R.bad(std::string("params: ") + names[i] + " is not finite");
    if (!(q.key > 0.f)) return R.bad("params: key must be above 0");
    if (!(q.white > 0.f)) return R.bad("params: white must be above 0");
    if (!(q.lo >= 0.f && q.hi <= 1.f && q.lo < q.hi)) return R.bad("params: lo and hi must be 0 <= lo < hi <= 1");
    if (!(q.adapt >= 0.f && q.adapt <= 1.f)) return R.bad("params: adapt must be 0 .. 1");
    if (q.min_ev > q.max_ev) return R.bad("params: min_ev is above max_ev");
    return AMVPT_OK;
}

/* what every entry refuses first; `out` null is each entry's own */
static amvpt_status image_check(const Refusal &R, const float *image, uint32_t channels, uint32_t w, uint32_t h,
                                const amvpt_tonemap_params *params) {
    if (!image) return R.bad("null image");
    if (!params) return R.bad("null params");
    if (amvpt_status s = check_channels(R, channels)) return s;
    if (amvpt_status s = check_size(R, w, h)) return s;
    return params_check(R, *params);
}

/* the metered rectangle {x0, y0, w, h} of both meter entries */
static amvpt_status meter_check(const Refusal &R, const float *image, uint32_t channels, uint32_t w, uint32_t h,
                                const uint32_t *rect, const amvpt_tonemap_params *params, const amvpt_tonemap_state *state,
                                uint32_t r[4]) {
    if (amvpt_status s = image_check(R, image, channels, w, h, params)) return s;
    if (!state) return R.bad("null state");
    r[0] = 0, r[1] = 0, r[2] = w, r[3] = h;
    if (rect) {
        if (rect[2] == 0 || rect[3] == 0) return R.bad("rect: zero area");
        if (rect[0] >= w || rect[2] > w - rect[0] || rect[1] >= h || rect[3] > h - rect[1]) return R.bad("rect: outside the image");
        for (int i = 0; i < 4; ++i) r[i] = rect[i];
    }
    if ((uint64_t) r[2] * r[3] >= (1ull << 32))
        return R.bad(rect ? "rect: 2^32 pixels or more (the counts are 32 bits)" : "width * height is 2^32 pixels or more (the counts are 32 bits)");
    return check_disjoint(R, {{state, sizeof(amvpt_tonemap_state), "state"}},
                          {{image, (size_t) w * h * channels * sizeof(float), "the image"}});
}

/* apply and srgb8, device and host: out_bytes is the size of one output pixel; on success ex is the manual exposure */
static amvpt_status map_check(const Refusal &R, const float *image, uint32_t channels, uint32_t w, uint32_t h,
                              const amvpt_tonemap_params *params, const amvpt_tonemap_state *state, const void *out,
                              size_t out_bytes, bool in_place_ok, TonemapOp &op, float &ex) {
    if (amvpt_status s = image_check(R, image, channels, w, h, params)) return s;
    if (!out) return R.bad("null out");
    if (params->auto_exposure && !state) return R.bad("null state with auto_exposure set");
    const size_t npx = (size_t) w * h, nimg = npx * channels * sizeof(float);
    const Span st{params->auto_exposure ? state : nullptr, sizeof(amvpt_tonemap_state), "the state"};
    if (in_place_ok && out == (const void *) image) {
        if (amvpt_status s = check_disjoint(R, {{out, npx * out_bytes, "out"}}, {st})) return s;
    } else if (amvpt_status s = check_disjoint(R, {{out, npx * out_bytes, "out"}}, {{image, nimg, "the image"}, st})) {
        return s;
    }
    op.op = params->op, op.white2 = params->white * params->white;
    ex = tm_manual_exposure(*params);
    return AMVPT_OK;
}

template <bool kBytes>
static void map_host(const float *image, uint32_t ch, size_t npx, float ex, const TonemapOp &op, void *out) {
    for (size_t p = 0; p < npx; ++p) {
        const float *src = image + p * ch;
        float y[3];
        tm_pixel(src, ex, op, y);
        if (kBytes) {
            uint8_t *d = static_cast<uint8_t *>(out) + p * 3;
            for (uint32_t c = 0; c < 3; ++c) d[c] = srgb8_value(y[c]);
        } else {
            float *d = static_cast<float *>(out) + p * ch;
            const float alpha = ch == 4 ? src[3] : 0.f;
            for (uint32_t c = 0; c < 3; ++c) d[c] = y[c];
            if (ch == 4) d[3] = alpha;
        }
    }
}

/* one launch covers the image, as in amvpt_srgb8: 2^23 blocks of 256 threads, four pixels each */
static constexpr uint64_t kMaxMapPixels = 1ull << 33;

template <bool kBytes>
static amvpt_status map_device(const Refusal &R, const float *image, uint32_t channels, uint32_t w, uint32_t h,
                               const amvpt_tonemap_params *params, const amvpt_tonemap_state *state, void *out,
                               void *stream) {
    TonemapArgs A;
    if (amvpt_status s = map_check(R, image, channels, w, h, params, state, out, kBytes ? 3 : channels * sizeof(float),
                                   !kBytes, A.op, A.exposure))
        return s;
    A.in = image, A.out = out, A.npx = (uint64_t) w * h;
    A.state = params->auto_exposure ? state : nullptr;
    if (A.npx > kMaxMapPixels) return R.bad("width * height above 2^33 pixels");
    if (amvpt_status s = R.need_device()) return s;
    const bool vec = ((uintptr_t) image & 15u) == 0 && ((uintptr_t) out & (kBytes ? 3u : 15u)) == 0;
    const uint64_t per = (uint64_t) kTmBlock * kTmPx;
    const dim3 grid((uint32_t) ((A.npx + per - 1) / per)), block(kTmBlock);
    hipStream_t st = (hipStream_t) stream;
    if (channels == 3) {
        if (vec) hipLaunchKernelGGL((k_tonemap<3, true, kBytes>), grid, block, 0, st, A);
        else hipLaunchKernelGGL((k_tonemap<3, false, kBytes>), grid, block, 0, st, A);
    } else {
        if (vec) hipLaunchKernelGGL((k_tonemap<4, true, kBytes>), grid, block, 0, st, A);
        else hipLaunchKernelGGL((k_tonemap<4, false, kBytes>), grid, block, 0, st, A);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail((R.who + " launch").c_str(), (int) e);
    return AMVPT_OK;
}

template <uint32_t kCh> static void launch_hist(bool vec, bool rect, dim3 grid, hipStream_t st, const HistArgs &A) {
    const dim3 block(kTmBlock);
    if (rect) hipLaunchKernelGGL((k_tonemap_hist<kCh, false, true>), grid, block, 0, st, A);
    else if (vec) hipLaunchKernelGGL((k_tonemap_hist<kCh, true, false>), grid, block, 0, st, A);
    else hipLaunchKernelGGL((k_tonemap_hist<kCh, false, false>), grid, block, 0, st, A);
}

} // namespace amvpt

using namespace amvpt;

extern "C" {

uint32_t amvpt_tonemap_version(void) { return AMVPT_TONEMAP_VERSION; }

amvpt_tonemap_params amvpt_tonemap_default_params(void) {
    amvpt_tonemap_params q;
    q.op = AMVPT_TONEMAP_LINEAR, q.auto_exposure = 0;
    q.ev = 0.f, q.key = 0.18f, q.lo = 0.10f, q.hi = 0.95f, q.adapt = 1.f, q.white = 4.f, q.min_ev = -16.f, q.max_ev = 16.f;
    return q;
}

double amvpt_tonemap_exp2_host(double x) { return exp2_pm(x); }

amvpt_status amvpt_tonemap_meter_host(const float *image, uint32_t channels, uint32_t width, uint32_t height,
                                      const uint32_t rect[4], const amvpt_tonemap_params *params,
                                      amvpt_tonemap_state *state) {
    uint32_t r[4];
    if (amvpt_status s = meter_check(Refusal("amvpt_tonemap_meter_host"), image, channels, width, height, rect, params,
                                     state, r))
        return s;
    for (uint32_t b = 0; b < kTmBins; ++b) state->hist[b] = 0;
    state->counted = state->skipped = 0;
    for (uint32_t y = r[1]; y < r[1] + r[3]; ++y)
        for (uint32_t x = r[0]; x < r[0] + r[2]; ++x) {
            const int32_t b = tm_bin(pp_lum(image + ((size_t) y * width + x) * channels));
            if (b == kTmSkipped) ++state->skipped;
            else ++state->hist[b];
        }
    tm_exposure(state->hist, *params, state);
    return AMVPT_OK;
}

amvpt_status amvpt_tonemap_meter(const float *image, uint32_t channels, uint32_t width, uint32_t height,
                                 const uint32_t rect[4], const amvpt_tonemap_params *params, amvpt_tonemap_state *state,
                                 void *stream) {
    const Refusal R("amvpt_tonemap_meter");
    uint32_t r[4];
    if (amvpt_status s = meter_check(R, image, channels, width, height, rect, params, state, r)) return s;
    if (amvpt_status s = R.need_device()) return s;
    hipStream_t st = (hipStream_t) stream;
    /* hist, counted and skipped lead the struct */
    hipError_t e = hipMemsetAsync(state, 0, (kTmBins + 2) * sizeof(uint32_t), st);
    if (e != hipSuccess) return hip_fail("amvpt_tonemap_meter fill", (int) e);
    HistArgs A;
    const bool narrow = r[2] != width;   /* rows of the full width are one flat run of pixels */
    A.in = image + ((size_t) r[1] * width + (narrow ? r[0] : 0u)) * channels;
    A.npx = (uint64_t) r[2] * r[3];
    A.rw = r[2], A.pitch = width, A.state = state;
    const uint64_t per = (uint64_t) kTmBlock * kTmPx, need = (A.npx + per - 1) / per;
    const dim3 grid((uint32_t) (need < kHistMaxBlocks ? need : kHistMaxBlocks));
    const bool vec = ((uintptr_t) A.in & 15u) == 0;
    if (channels == 3) launch_hist<3>(vec, narrow, grid, st, A);
    else launch_hist<4>(vec, narrow, grid, st, A);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail("amvpt_tonemap_meter launch", (int) e);
    hipLaunchKernelGGL(k_exposure, dim3(1), dim3(kTmBins), 0, st, state, *params);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail("amvpt_tonemap_meter exposure launch", (int) e);
    return AMVPT_OK;
}

amvpt_status amvpt_tonemap_apply_host(const float *image, uint32_t channels, uint32_t width, uint32_t height,
                                      const amvpt_tonemap_params *params, const amvpt_tonemap_state *state, float *out) {
    TonemapOp op;
    float ex;
    if (amvpt_status s = map_check(Refusal("amvpt_tonemap_apply_host"), image, channels, width, height, params, state, out,
                                   channels * sizeof(float), true, op, ex))
        return s;
    map_host<false>(image, channels, (size_t) width * height, params->auto_exposure ? state->exposure : ex, op, out);
    return AMVPT_OK;
}

amvpt_status amvpt_tonemap_srgb8_host(const float *image, uint32_t channels, uint32_t width, uint32_t height,
                                      const amvpt_tonemap_params *params, const amvpt_tonemap_state *state, uint8_t *out) {
    TonemapOp op;
    float ex;
    if (amvpt_status s = map_check(Refusal("amvpt_tonemap_srgb8_host"), image, channels, width, height, params, state, out,
                                   3, false, op, ex))
        return s;
    map_host<true>(image, channels, (size_t) width * height, params->auto_exposure ? state->exposure : ex, op, out);
    return AMVPT_OK;
}

amvpt_status amvpt_tonemap_apply(const float *image, uint32_t channels, uint32_t width, uint32_t height,
                                 const amvpt_tonemap_params *params, const amvpt_tonemap_state *state, float *out,
                                 void *stream) {
    return map_device<false>(Refusal("amvpt_tonemap_apply"), image, channels, width, height, params, state, out, stream);
}

amvpt_status amvpt_tonemap_srgb8(const float *image, uint32_t channels, uint32_t width, uint32_t height,
                                 const amvpt_tonemap_params *params, const amvpt_tonemap_state *state, uint8_t *out,
                                 void *stream) {
    return map_device<true>(Refusal("amvpt_tonemap_srgb8"), image, channels, width, height, params, state, out, stream);
}

} // extern "C"

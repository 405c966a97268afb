/*
 * amvpt_denoise.hip -- the entries of include/amvpt_denoise.h: the a-trous denoiser over a developed quilt and its
 * guide records.  One launch per iteration on the caller's stream, one thread per pixel, blocks of 32 x 8 pixels;
 * no atomics, no device-wide synchronisation, nothing allocated.  Two kernels, one per step class (DESIGN.md has
 * the measurements behind the split):
 *   k_denoise_tile<S>   steps 1 and 2: a block's 25 x 256 taps fall into (32 + 4 S) x (8 + 4 S) pixels, so the
 *                       block stages those (records and colour, 44 bytes a pixel, 27.5 KiB at S = 2) in LDS once
 *                       and every tap reads LDS
 *   k_denoise_direct    steps >= 4: the taps of neighbouring pixels no longer coincide inside a block; they go to
 *                       memory directly (L2 serves the re-reads between blocks)
 * The per-pixel function is ddenoise.h's, shared with the host-only entry below.
 */
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <string>

#include "../../include/amvpt_denoise.h"
#include "ddenoise.h"
#include "internal.h"

namespace amvpt {

static constexpr int kTileW = 32, kTileH = 8;
static constexpr uint32_t kDenoiseBlock = kTileW * kTileH;

struct DenoiseArgs {
    const float *in, *guides;
    float *out;
    uint32_t channels, w, h, tiles_x;
    DenoiseStep K;
};

/* the pixel's RGB, and with four channels the alpha of the iteration's input (the image's own, handed down) */
__device__ __forceinline__ void denoise_store(const DenoiseArgs &A, int x, int y, const float rgb[3]) {
    const size_t at = ((size_t) y * A.w + (size_t) x) * A.channels;
    A.out[at] = rgb[0], A.out[at + 1] = rgb[1], A.out[at + 2] = rgb[2];
    if (A.channels == 4u) A.out[at + 3] = A.in[at + 3];
}

__global__ void __launch_bounds__(kDenoiseBlock) k_denoise_direct(DenoiseArgs A) {
    const int x = (int) (blockIdx.x % A.tiles_x) * kTileW + (int) (threadIdx.x % kTileW);
    const int y = (int) (blockIdx.x / A.tiles_x) * kTileH + (int) (threadIdx.x / kTileW);
    if (x >= (int) A.w || y >= (int) A.h) return;
    const DenoisePlanes P{A.in, A.guides, A.channels, A.w};
    float rgb[3];
    denoise_pixel(P, x, y, (int) A.w, (int) A.h, A.K, rgb);
    denoise_store(A, x, y, rgb);
}

/* the staged pixels of one block, plane by plane: consecutive lanes read consecutive 16-byte heads (ds_read_b128)
 * and consecutive dwords of every other plane, so no read conflicts on a bank */
template <int S>
struct DenoiseTile {
    static constexpr int kHalo = 2 * S, kW = kTileW + 2 * kHalo, kH = kTileH + 2 * kHalo, kN = kW * kH;
    float4 head[kN];      /* shape, normal */
    float view[kN];
    float pos[3][kN];
    float rgb[3][kN];
};

template <int S>
struct DenoiseTileSrc {
    const DenoiseTile<S> &T;
    int x0, y0;   /* image coordinates of the tile's first staged pixel */
    __device__ __forceinline__ int at(int x, int y) const { return (y - y0) * DenoiseTile<S>::kW + (x - x0); }
    __device__ __forceinline__ void head(int x, int y, float g[4]) const {
        const float4 v = T.head[at(x, y)];
        g[0] = v.x, g[1] = v.y, g[2] = v.z, g[3] = v.w;
    }
    __device__ __forceinline__ float view(int x, int y) const { return T.view[at(x, y)]; }
    __device__ __forceinline__ void point(int x, int y, float p[3]) const {
        const int i = at(x, y);
        p[0] = T.pos[0][i], p[1] = T.pos[1][i], p[2] = T.pos[2][i];
    }
    __device__ __forceinline__ void color(int x, int y, float c[3]) const {
        const int i = at(x, y);
        c[0] = T.rgb[0][i], c[1] = T.rgb[1][i], c[2] = T.rgb[2][i];
    }
};

template <int S>
__global__ void __launch_bounds__(kDenoiseBlock) k_denoise_tile(DenoiseArgs A) {
    using Tile = DenoiseTile<S>;
    __shared__ Tile T;
    const int bx = (int) (blockIdx.x % A.tiles_x) * kTileW, by = (int) (blockIdx.x / A.tiles_x) * kTileH;
    const int x0 = bx - Tile::kHalo, y0 = by - Tile::kHalo;
    /* pixels outside the image stay unstaged: denoise_pixel tests a tap's coordinates before it reads anything */
    for (int i = (int) threadIdx.x; i < Tile::kN; i += (int) kDenoiseBlock) {
        const int gx = x0 + i % Tile::kW, gy = y0 + i / Tile::kW;
        if (gx < 0 || gy < 0 || gx >= (int) A.w || gy >= (int) A.h) continue;
        const size_t px = (size_t) gy * A.w + (size_t) gx;
        const float *r = A.guides + 8 * px, *c = A.in + A.channels * px;
        T.head[i] = make_float4(r[0], r[1], r[2], r[3]);
        T.pos[0][i] = r[4], T.pos[1][i] = r[5], T.pos[2][i] = r[6];
        T.view[i] = r[7];
        T.rgb[0][i] = c[0], T.rgb[1][i] = c[1], T.rgb[2][i] = c[2];
    }
    __syncthreads();
    const int x = bx + (int) (threadIdx.x % kTileW), y = by + (int) (threadIdx.x / kTileW);
    if (x >= (int) A.w || y >= (int) A.h) return;
    DenoiseStep K = A.K;
    K.step = S;
    const DenoiseTileSrc<S> src{T, x0, y0};
    float rgb[3];
    denoise_pixel(src, x, y, (int) A.w, (int) A.h, K, rgb);
    denoise_store(A, x, y, rgb);
}

/* a visible device is remembered (it does not go away); its absence is asked again on the next call */
static bool denoise_device_ok() {
    static std::atomic<bool> seen{false};
    if (seen.load(std::memory_order_relaxed)) return true;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return false;
    seen.store(true, std::memory_order_relaxed);
    return true;
}

static bool dn_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t a0 = (uintptr_t) a, b0 = (uintptr_t) b;
    return a0 < b0 + nb && b0 < a0 + na;
}

/* the refusals of both entries */
static amvpt_status denoise_check(const char *who, const float *image, uint32_t channels, uint32_t w, uint32_t h,
                                  const float *guides, const amvpt_denoise_params *p, const float *out, const float *scratch) {
    const std::string s = std::string(who) + ": ";
    auto bad = [&](const std::string &what) { set_error(s + what); return AMVPT_ERR_INVALID; };
    if (!image) return bad("null image");
    if (!guides) return bad("null guides");
    if (!p) return bad("null params");
    if (!out) return bad("null out");
    if (channels != 3u && channels != 4u) return bad("channels must be 3 or 4, not " + std::to_string(channels));
    if (w == 0) return bad("width is 0");
    if (h == 0) return bad("height is 0");
    if (p->iterations < 1u || p->iterations > 8u) return bad("params: iterations must be 1 .. 8, not " + std::to_string(p->iterations));
    if (!dn_finite(p->sigma_color) || !(p->sigma_color > 0.f)) return bad("params: sigma_color must be finite and above 0");
    if (!dn_finite(p->color_floor) || !(p->color_floor > 0.f)) return bad("params: color_floor must be finite and above 0");
    if (!dn_finite(p->sigma_plane) || !(p->sigma_plane > 0.f)) return bad("params: sigma_plane must be finite and above 0");
    if (p->normal_squarings > 7u) return bad("params: normal_squarings must be 0 .. 7, not " + std::to_string(p->normal_squarings));
    if (p->iterations > 1u && !scratch) return bad("null scratch (it may be null only when iterations is 1)");
    const size_t npx = (size_t) w * h, nimg = npx * channels * sizeof(float), ngd = npx * 8 * sizeof(float);
    if (dn_overlap(out, nimg, image, nimg)) return bad("out overlaps the image");
    if (dn_overlap(out, nimg, guides, ngd)) return bad("out overlaps the guides");
    if (scratch) {
        if (dn_overlap(scratch, nimg, image, nimg)) return bad("scratch overlaps the image");
        if (dn_overlap(scratch, nimg, guides, ngd)) return bad("scratch overlaps the guides");
        if (dn_overlap(scratch, nimg, out, nimg)) return bad("scratch overlaps out");
    }
    return AMVPT_OK;
}

/* iteration i of n: its constants, and where it reads and writes -- out and scratch take turns so that the last
 * iteration lands in out */
static DenoiseStep denoise_step(const amvpt_denoise_params &p, uint32_t i) {
    DenoiseStep K;
    K.inv_s2 = 1.f / (p.sigma_color * p.sigma_color);
    for (uint32_t j = 0; j < i; ++j) K.inv_s2 = 4.f * K.inv_s2;
    K.floor2 = p.color_floor * p.color_floor;
    K.inv_sp = 1.f / p.sigma_plane;
    K.squarings = p.normal_squarings;
    K.step = (int32_t) (1u << i);
    return K;
}
static float *denoise_dst(uint32_t i, uint32_t n, float *out, float *scratch) { return ((n - 1u - i) & 1u) ? scratch : out; }

} // namespace amvpt

using namespace amvpt;

extern "C" {

uint32_t amvpt_denoise_version(void) { return AMVPT_DENOISE_VERSION; }

amvpt_denoise_params amvpt_denoise_default_params(void) {
    amvpt_denoise_params p;
    p.iterations = 3;
    p.sigma_color = 1.0f;
    p.color_floor = 0.01f;
    p.sigma_plane = 0.05f;
    p.normal_squarings = 5;
    return p;
}

amvpt_status amvpt_denoise_host(const float *image, uint32_t channels, uint32_t width, uint32_t height, const float *guides,
                                const amvpt_denoise_params *params, float *out, float *scratch) {
    if (amvpt_status s = denoise_check("amvpt_denoise_host", image, channels, width, height, guides, params, out, scratch)) return s;
    const float *in = image;
    for (uint32_t i = 0; i < params->iterations; ++i) {
        const DenoiseStep K = denoise_step(*params, i);
        float *dst = denoise_dst(i, params->iterations, out, scratch);
        const DenoisePlanes P{in, guides, channels, width};
        for (uint32_t y = 0; y < height; ++y)
            for (uint32_t x = 0; x < width; ++x) {
                float rgb[3];
                denoise_pixel(P, (int) x, (int) y, (int) width, (int) height, K, rgb);
                const size_t at = ((size_t) y * width + x) * channels;
                dst[at] = rgb[0], dst[at + 1] = rgb[1], dst[at + 2] = rgb[2];
                if (channels == 4u) dst[at + 3] = in[at + 3];
            }
        in = dst;
    }
    return AMVPT_OK;
}

amvpt_status amvpt_denoise(const float *image_device, uint32_t channels, uint32_t width, uint32_t height,
                           const float *guides_device, const amvpt_denoise_params *params, float *out_device,
                           float *scratch_device, void *stream) {
    if (amvpt_status s = denoise_check("amvpt_denoise", image_device, channels, width, height, guides_device, params, out_device,
                                       scratch_device))
        return s;
    /* pixel coordinates are ints, and one launch of 32 x 8 tiles covers the image */
    if (width > 0x7fffff00u || height > 0x7fffff00u) { set_error("amvpt_denoise: width or height above 2^31 - 256"); return AMVPT_ERR_INVALID; }
    const uint64_t tx = (width + (uint32_t) kTileW - 1u) / (uint32_t) kTileW, ty = (height + (uint32_t) kTileH - 1u) / (uint32_t) kTileH;
    if (tx * ty >= (1ull << 31)) { set_error("amvpt_denoise: width x height above 2^31 tiles of 32 x 8 pixels"); return AMVPT_ERR_INVALID; }
    if (!denoise_device_ok()) { set_error("amvpt_denoise: no HIP device visible"); return AMVPT_ERR_NO_DEVICE; }
    const dim3 grid((uint32_t) (tx * ty)), block(kDenoiseBlock);
    hipStream_t st = (hipStream_t) stream;
    const float *in = image_device;
    for (uint32_t i = 0; i < params->iterations; ++i) {
        float *dst = denoise_dst(i, params->iterations, out_device, scratch_device);
        const DenoiseArgs A{in, guides_device, dst, channels, width, height, (uint32_t) tx, denoise_step(*params, i)};
        if (i == 0) hipLaunchKernelGGL(k_denoise_tile<1>, grid, block, 0, st, A);
        else if (i == 1) hipLaunchKernelGGL(k_denoise_tile<2>, grid, block, 0, st, A);
        else hipLaunchKernelGGL(k_denoise_direct, grid, block, 0, st, A);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail("amvpt_denoise launch", (int) e);
        in = dst;
    }
    return AMVPT_OK;
}

} // extern "C"

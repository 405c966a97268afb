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

#include <cstdint>
#include <string>

#include "../../include/amvpt_denoise.h"
#include "ddenoise.h"
#include "dtile.h"
#include "internal.h"
#include "post_host.h"

namespace amvpt {

struct DenoiseArgs {
    const float *in, *guides;
    float *out;
    uint32_t channels, w, h, tiles_x;
    DenoiseStep K;
};

/* the pixel's RGB, and with four channels the alpha of the iteration's input (the image's own, handed down) */
__host__ __device__ __forceinline__ void denoise_store(const DenoiseArgs &A, int x, int y, const float rgb[3]) {
    const size_t at = ((size_t) y * A.w + (size_t) x) * A.channels;
    A.out[at] = rgb[0], A.out[at + 1] = rgb[1], A.out[at + 2] = rgb[2];
    if (A.channels == 4u) A.out[at + 3] = A.in[at + 3];
}

__global__ void __launch_bounds__(kTileBlock) k_denoise_direct(DenoiseArgs A) {
    const TilePixel t = tile_pixel(A.tiles_x);
    if (t.x >= (int) A.w || t.y >= (int) A.h) return;
    const DenoisePlanes P{{A.guides, A.w}, A.in, A.channels};
    float rgb[3];
    denoise_pixel(P, t.x, t.y, (int) A.w, (int) A.h, A.K, rgb);
    denoise_store(A, t.x, t.y, rgb);
}

/* the staged pixels of one block: the guide records and the colour */
template <int S>
struct DenoiseTile : GuideTile<2 * S> {
    float rgb[3][GuideTile<2 * S>::kN];
};

template <int S>
struct DenoiseTileSrc : GuideTileSrc<DenoiseTile<S>> {
    __device__ __forceinline__ void color(int x, int y, float c[3]) const {
        const int i = this->at(x, y);
        c[0] = this->T.rgb[0][i], c[1] = this->T.rgb[1][i], c[2] = this->T.rgb[2][i];
    }
};

template <int S>
__global__ void __launch_bounds__(kTileBlock) k_denoise_tile(DenoiseArgs A) {
    using Tile = DenoiseTile<S>;
    __shared__ Tile T;
    const TilePixel t = tile_pixel(A.tiles_x);
    const int x0 = t.bx - Tile::kHalo, y0 = t.by - Tile::kHalo;
    tile_stage<Tile>(x0, y0, A.w, A.h, [&](int i, size_t px) {
        const float *r = A.guides + 8 * px, *c = A.in + A.channels * px;
        T.stage(i, r);
        T.rgb[0][i] = c[0], T.rgb[1][i] = c[1], T.rgb[2][i] = c[2];
    });
    __syncthreads();
    if (t.x >= (int) A.w || t.y >= (int) A.h) return;
    DenoiseStep K = A.K;
    K.step = S;
    const DenoiseTileSrc<S> src{{T, x0, y0}};
    float rgb[3];
    denoise_pixel(src, t.x, t.y, (int) A.w, (int) A.h, K, rgb);
    denoise_store(A, t.x, t.y, rgb);
}

/* the refusals of both entries */
static amvpt_status denoise_check(const Refusal &R, const float *image, uint32_t channels, uint32_t w, uint32_t h,
                                  const float *guides, const amvpt_denoise_params *p, const float *out, const float *scratch) {
    if (!image) return R.bad("null image");
    if (!guides) return R.bad("null guides");
    if (!p) return R.bad("null params");
    if (!out) return R.bad("null out");
    if (amvpt_status st = check_channels(R, channels)) return st;
    if (amvpt_status st = check_size(R, w, h)) return st;
    if (p->iterations < 1u || p->iterations > 8u) return R.bad("params: iterations must be 1 .. 8, not " + std::to_string(p->iterations));
    if (!pp_finite(p->sigma_color) || !(p->sigma_color > 0.f)) return R.bad("params: sigma_color must be finite and above 0");
    if (!pp_finite(p->color_floor) || !(p->color_floor > 0.f)) return R.bad("params: color_floor must be finite and above 0");
    if (!pp_finite(p->sigma_plane) || !(p->sigma_plane > 0.f)) return R.bad("params: sigma_plane must be finite and above 0");
    if (p->normal_squarings > 7u) return R.bad("params: normal_squarings must be 0 .. 7, not " + std::to_string(p->normal_squarings));
    if (p->iterations > 1u && !scratch) return R.bad("null scratch (it may be null only when iterations is 1)");
    const size_t npx = (size_t) w * h, nimg = npx * channels * sizeof(float), ngd = npx * 8 * sizeof(float);
    return check_disjoint(R, {{out, nimg, "out"}, {scratch, nimg, "scratch"}}, {{image, nimg, "the image"}, {guides, ngd, "the guides"}});
}

/* the constants of iteration i */
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
    const Refusal R("amvpt_denoise_host");
    if (amvpt_status s = denoise_check(R, image, channels, width, height, guides, params, out, scratch)) return s;
    const float *in = image;
    for (uint32_t i = 0; i < params->iterations; ++i) {
        float *dst = pingpong_dst(i, params->iterations, out, scratch);
        const DenoiseArgs A{in, guides, dst, channels, width, height, 0u, denoise_step(*params, i)};
        const DenoisePlanes P{{guides, width}, in, channels};
        for (uint32_t y = 0; y < height; ++y)
            for (uint32_t x = 0; x < width; ++x) {
                float rgb[3];
                denoise_pixel(P, (int) x, (int) y, (int) width, (int) height, A.K, rgb);
                denoise_store(A, (int) x, (int) y, rgb);
            }
        in = dst;
    }
    return AMVPT_OK;
}

amvpt_status amvpt_denoise(const float *image_device, uint32_t channels, uint32_t width, uint32_t height,
                           const float *guides_device, const amvpt_denoise_params *params, float *out_device,
                           float *scratch_device, void *stream) {
    const Refusal R("amvpt_denoise");
    if (amvpt_status s = denoise_check(R, image_device, channels, width, height, guides_device, params, out_device, scratch_device))
        return s;
    if (amvpt_status s = check_size_tiles(R, width, height)) return s;
    if (amvpt_status s = R.need_device()) return s;
    uint64_t tx, ty;
    tile_grid(width, height, tx, ty);
    const dim3 grid((uint32_t) (tx * ty)), block(kTileBlock);
    hipStream_t st = (hipStream_t) stream;
    const float *in = image_device;
    for (uint32_t i = 0; i < params->iterations; ++i) {
        float *dst = pingpong_dst(i, params->iterations, out_device, scratch_device);
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

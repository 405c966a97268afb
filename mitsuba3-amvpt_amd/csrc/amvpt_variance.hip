/*
 * amvpt_variance.hip -- stages 2 and 3 of include/amvpt_variance.h: the variance of the accumulated luminance from
 * the temporal moments, and the a-trous filter that variance guides.  (Stage 1, amvpt_temporal_moments, is an
 * instance of the temporal kernel and lives in amvpt_temporal.hip.)  Every launch is ordered on the caller's stream,
 * one thread per pixel, blocks of 32 x 8 pixels in a flat grid; pure gathers with no atomics, no device-wide
 * synchronisation, nothing allocated.  The kernels:
 *   k_variance                   stage 2: the 7 x 7 window runs only where the history is shorter than min_history,
 *                                on scattered pixels along disocclusions; a block with such a pixel stages its
 *                                38 x 14 pixels in LDS, every other block reads its own pixels and is done
 *   k_denoise_variance_tile<S>   stage 3, steps 1 and 2: as k_denoise_tile<S> of amvpt_denoise.hip, the block stages
 *                                its (32 + 4 S) x (8 + 4 S) pixels in LDS once (records, colour and variance, 48
 *                                bytes a pixel, 30 KiB at S = 2); the 3 x 3 prefilter reads the same tile
 *   k_denoise_variance_direct    stage 3, steps >= 4: the 25 taps go to memory directly; the nine of the 3 x 3
 *                                prefilter, which stays at step 1, read a 34 x 10 tile of shape, view and variance
 * The per-pixel functions are dvariance.h's, shared with the host-only entries below.
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/amvpt_variance.h"
#include "dtile.h"
#include "dvariance.h"
#include "internal.h"
#include "post_host.h"

namespace amvpt {

struct VarianceArgs {
    const float *moments, *count, *guides;
    float *out;
    uint32_t w, h, tiles_x;
    VarianceConst K;
};

/* the pixels a block's 7 x 7 windows fall into: the guide records, the count and the moments */
struct MomentTile : GuideTile<3> {
    float cnt[kN];
    float mom[2][kN];
};

struct MomentTileSrc : GuideTileSrc<MomentTile> {
    __device__ __forceinline__ float count(int x, int y) const { return T.cnt[at(x, y)]; }
    __device__ __forceinline__ void moments(int x, int y, float m[2]) const {
        const int i = at(x, y);
        m[0] = T.mom[0][i], m[1] = T.mom[1][i];
    }
};

/* A block none of whose pixels takes the window (the steady state away from disocclusions) reads its own 16 bytes a
 * pixel and is done; a block with one stages its 38 x 14 pixels (44 bytes each, 22.9 KiB) in LDS once, and the
 * windows read LDS. */
__global__ void __launch_bounds__(kTileBlock) k_variance(VarianceArgs A) {
    __shared__ MomentTile T;
    const TilePixel t = tile_pixel(A.tiles_x);
    const bool inside = t.x < (int) A.w && t.y < (int) A.h;
    const MomentPlanes P{{A.guides, A.w}, A.moments, A.count};
    const bool window = inside && variance_takes_window(P, t.x, t.y, A.K);
    if (!__syncthreads_or(window ? 1 : 0)) {
        if (inside) A.out[(size_t) t.y * A.w + (size_t) t.x] = variance_pixel(P, t.x, t.y, (int) A.w, (int) A.h, A.K);
        return;
    }
    const int x0 = t.bx - MomentTile::kHalo, y0 = t.by - MomentTile::kHalo;
    tile_stage<MomentTile>(x0, y0, A.w, A.h, [&](int i, size_t px) {
        T.stage(i, A.guides + 8 * px);
        T.cnt[i] = A.count[px];
        T.mom[0][i] = A.moments[2 * px], T.mom[1][i] = A.moments[2 * px + 1];
    });
    __syncthreads();
    if (!inside) return;
    const MomentTileSrc src{{T, x0, y0}};
    A.out[(size_t) t.y * A.w + (size_t) t.x] = variance_pixel(src, t.x, t.y, (int) A.w, (int) A.h, A.K);
}

struct DenoiseVarianceArgs {
    const float *in, *vin, *guides;
    float *out, *vout;   /* vout may be null: the variance of the last iteration nobody asked for */
    uint32_t channels, w, h, tiles_x;
    VarianceStep K;
};

/* the pixel's RGB and variance, and with four channels the alpha of the iteration's input (the image's own) */
__host__ __device__ __forceinline__ void denoise_variance_store(const DenoiseVarianceArgs &A, int x, int y, const float rgb[3],
                                                                float v) {
    const size_t px = (size_t) y * A.w + (size_t) x, at = px * A.channels;
    A.out[at] = rgb[0], A.out[at + 1] = rgb[1], A.out[at + 2] = rgb[2];
    if (A.channels == 4u) A.out[at + 3] = A.in[at + 3];
    if (A.vout) A.vout[px] = v;
}

/* what the 3 x 3 prefilter of a block reads: shape, view and variance of its 34 x 10 pixels (12 bytes each, 4 KiB) */
struct PrefilterTile {
    static constexpr int kW = kTileW + 2, kH = kTileH + 2, kN = kW * kH;
    float shape[kN], view[kN], var[kN];
};

struct PrefilterTileSrc {
    const PrefilterTile &T;
    int x0, y0;   /* image coordinates of the tile's first staged pixel */
    __device__ __forceinline__ int at(int x, int y) const { return (y - y0) * PrefilterTile::kW + (x - x0); }
    __device__ __forceinline__ float shape(int x, int y) const { return T.shape[at(x, y)]; }
    __device__ __forceinline__ float view(int x, int y) const { return T.view[at(x, y)]; }
    __device__ __forceinline__ float var(int x, int y) const { return T.var[at(x, y)]; }
};

__global__ void __launch_bounds__(kTileBlock) k_denoise_variance_direct(DenoiseVarianceArgs A) {
    __shared__ PrefilterTile T;
    const TilePixel t = tile_pixel(A.tiles_x);
    const int x0 = t.bx - 1, y0 = t.by - 1;
    tile_stage<PrefilterTile>(x0, y0, A.w, A.h, [&](int i, size_t px) {
        T.shape[i] = A.guides[8 * px], T.view[i] = A.guides[8 * px + 7], T.var[i] = A.vin[px];
    });
    __syncthreads();
    if (t.x >= (int) A.w || t.y >= (int) A.h) return;
    const VariancePlanes P{{A.guides, A.w}, A.in, A.vin, A.channels};
    const PrefilterTileSrc pre{T, x0, y0};
    float rgb[3], v;
    denoise_variance_pixel(P, pre, t.x, t.y, (int) A.w, (int) A.h, A.K, rgb, v);
    denoise_variance_store(A, t.x, t.y, rgb, v);
}

/* the staged pixels of one block: the guide records, the colour and the variance */
template <int S>
struct VarianceTile : GuideTile<2 * S> {
    float rgb[3][GuideTile<2 * S>::kN];
    float var[GuideTile<2 * S>::kN];
};

template <int S>
struct VarianceTileSrc : GuideTileSrc<VarianceTile<S>> {
    __device__ __forceinline__ void color(int x, int y, float c[3]) const {
        const int i = this->at(x, y);
        c[0] = this->T.rgb[0][i], c[1] = this->T.rgb[1][i], c[2] = this->T.rgb[2][i];
    }
    __device__ __forceinline__ float var(int x, int y) const { return this->T.var[this->at(x, y)]; }
};

/* every tap of a pixel of the block, the prefilter's at step 1 among them, lies within the halo of 2 S */
template <int S>
__global__ void __launch_bounds__(kTileBlock) k_denoise_variance_tile(DenoiseVarianceArgs A) {
    using Tile = VarianceTile<S>;
    __shared__ Tile T;
    const TilePixel t = tile_pixel(A.tiles_x);
    const int x0 = t.bx - Tile::kHalo, y0 = t.by - Tile::kHalo;
    tile_stage<Tile>(x0, y0, A.w, A.h, [&](int i, size_t px) {
        const float *r = A.guides + 8 * px, *c = A.in + A.channels * px;
        T.stage(i, r);
        T.rgb[0][i] = c[0], T.rgb[1][i] = c[1], T.rgb[2][i] = c[2];
        T.var[i] = A.vin[px];
    });
    __syncthreads();
    if (t.x >= (int) A.w || t.y >= (int) A.h) return;
    VarianceStep K = A.K;
    K.step = S;
    const VarianceTileSrc<S> src{{T, x0, y0}};
    float rgb[3], v;
    denoise_variance_pixel(src, src, t.x, t.y, (int) A.w, (int) A.h, K, rgb, v);
    denoise_variance_store(A, t.x, t.y, rgb, v);
}

/* the parameter ranges, for all three of the struct's users */
static amvpt_status variance_params_check(const Refusal &R, const amvpt_variance_params *p) {
    if (p->iterations < 1u || p->iterations > 8u) return R.bad("params: iterations must be 1 .. 8, not " + std::to_string(p->iterations));
    if (!pp_finite(p->sigma_lum) || !(p->sigma_lum > 0.f)) return R.bad("params: sigma_lum must be finite and above 0");
    if (!pp_finite(p->var_floor) || !(p->var_floor > 0.f)) return R.bad("params: var_floor must be finite and above 0");
    if (!pp_finite(p->sigma_plane) || !(p->sigma_plane > 0.f)) return R.bad("params: sigma_plane must be finite and above 0");
    if (p->normal_squarings > 7u) return R.bad("params: normal_squarings must be 0 .. 7, not " + std::to_string(p->normal_squarings));
    if (p->min_history < 1u || p->min_history > 65535u)
        return R.bad("params: min_history must be 1 .. 65535, not " + std::to_string(p->min_history));
    return AMVPT_OK;
}

/* the refusals of both entries of stage 2; on success A holds everything but the launch geometry */
static amvpt_status variance_check(const Refusal &R, const float *moments, const float *count, const float *guides, uint32_t w,
                                   uint32_t h, const amvpt_variance_params *p, float *out, VarianceArgs &A) {
    if (!moments) return R.bad("null moments");
    if (!count) return R.bad("null count");
    if (!guides) return R.bad("null guides");
    if (!p) return R.bad("null params");
    if (!out) return R.bad("null out");
    if (amvpt_status st = check_size_tiles(R, w, h)) return st;
    if (amvpt_status st = variance_params_check(R, p)) return st;
    const size_t npx = (size_t) w * h, ncnt = npx * sizeof(float);
    if (amvpt_status st = check_disjoint(R, {{out, ncnt, "out"}},
                                         {{moments, 2 * ncnt, "the moments"}, {count, ncnt, "the count"}, {guides, 8 * ncnt, "the guides"}}))
        return st;
    A.moments = moments, A.count = count, A.guides = guides, A.out = out;
    A.w = w, A.h = h, A.tiles_x = 0;
    A.K.inv_sp = 1.f / p->sigma_plane;
    A.K.min_history = (float) p->min_history;
    A.K.squarings = p->normal_squarings;
    return AMVPT_OK;
}

/* the refusals of both entries of stage 3 */
static amvpt_status denoise_variance_check(const Refusal &R, const float *image, uint32_t channels, uint32_t w, uint32_t h,
                                           const float *variance, const float *guides, const amvpt_variance_params *p,
                                           const float *out, const float *scratch, const float *var_out, const float *var_scratch) {
    if (!image) return R.bad("null image");
    if (!variance) return R.bad("null variance");
    if (!guides) return R.bad("null guides");
    if (!p) return R.bad("null params");
    if (!out) return R.bad("null out");
    if (amvpt_status st = check_channels(R, channels)) return st;
    if (amvpt_status st = check_size_tiles(R, w, h)) return st;
    if (amvpt_status st = variance_params_check(R, p)) return st;
    if (p->iterations > 1u && !scratch) return R.bad("null scratch (it may be null only when iterations is 1)");
    if (p->iterations > 1u && !var_scratch) return R.bad("null var_scratch (it may be null only when iterations is 1)");
    if (p->iterations > 2u && !var_out) return R.bad("null var_out (it may be null only when iterations is at most 2)");
    const size_t npx = (size_t) w * h, nvar = npx * sizeof(float), nimg = nvar * channels, ngd = nvar * 8;
    return check_disjoint(
        R, {{out, nimg, "out"}, {scratch, nimg, "scratch"}, {var_out, nvar, "var_out"}, {var_scratch, nvar, "var_scratch"}},
        {{image, nimg, "the image"}, {variance, nvar, "the variance"}, {guides, ngd, "the guides"}});
}

/* the constants of iteration i */
static VarianceStep variance_step(const amvpt_variance_params &p, uint32_t i) {
    VarianceStep K;
    K.sl2 = p.sigma_lum * p.sigma_lum;
    K.var_floor = p.var_floor;
    K.inv_sp = 1.f / p.sigma_plane;
    K.squarings = p.normal_squarings;
    K.step = (int32_t) (1u << i);
    return K;
}

} // namespace amvpt

using namespace amvpt;

extern "C" {

uint32_t amvpt_variance_version(void) { return AMVPT_VARIANCE_VERSION; }

amvpt_variance_params amvpt_variance_default_params(void) {
    amvpt_variance_params p;
    p.iterations = 4;
    p.sigma_lum = 2.0f;
    p.var_floor = 1e-8f;
    p.sigma_plane = 0.05f;
    p.normal_squarings = 5;
    p.min_history = 4;
    return p;
}

amvpt_status amvpt_variance_host(const float *moments, const float *count, const float *guides, uint32_t width,
                                 uint32_t height, const amvpt_variance_params *params, float *out) {
    VarianceArgs A;
    if (amvpt_status s = variance_check(Refusal("amvpt_variance_host"), moments, count, guides, width, height, params, out, A))
        return s;
    const MomentPlanes P{{guides, width}, moments, count};
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x)
            out[(size_t) y * width + x] = variance_pixel(P, (int) x, (int) y, (int) width, (int) height, A.K);
    return AMVPT_OK;
}

amvpt_status amvpt_variance(const float *moments_device, const float *count_device, const float *guides_device,
                            uint32_t width, uint32_t height, const amvpt_variance_params *params, float *out_device,
                            void *stream) {
    const Refusal R("amvpt_variance");
    VarianceArgs A;
    if (amvpt_status s = variance_check(R, moments_device, count_device, guides_device, width, height, params, out_device, A))
        return s;
    if (amvpt_status s = R.need_device()) return s;
    uint64_t tx, ty;
    tile_grid(width, height, tx, ty);
    A.tiles_x = (uint32_t) tx;
    hipLaunchKernelGGL(k_variance, dim3((uint32_t) (tx * ty)), dim3(kTileBlock), 0, (hipStream_t) stream, A);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail("amvpt_variance launch", (int) e);
    return AMVPT_OK;
}

amvpt_status amvpt_denoise_variance_host(const float *image, uint32_t channels, uint32_t width, uint32_t height,
                                         const float *variance, const float *guides, const amvpt_variance_params *params,
                                         float *out, float *scratch, float *var_out, float *var_scratch) {
    if (amvpt_status s = denoise_variance_check(Refusal("amvpt_denoise_variance_host"), image, channels, width, height, variance,
                                                guides, params, out, scratch, var_out, var_scratch))
        return s;
    const float *in = image, *vin = variance;
    for (uint32_t i = 0; i < params->iterations; ++i) {
        float *dst = pingpong_dst(i, params->iterations, out, scratch);
        float *vdst = pingpong_dst(i, params->iterations, var_out, var_scratch);
        const DenoiseVarianceArgs A{in, vin, guides, dst, vdst, channels, width, height, 0u, variance_step(*params, i)};
        const VariancePlanes P{{guides, width}, in, vin, channels};
        for (uint32_t y = 0; y < height; ++y)
            for (uint32_t x = 0; x < width; ++x) {
                float rgb[3], v;
                denoise_variance_pixel(P, P, (int) x, (int) y, (int) width, (int) height, A.K, rgb, v);
                denoise_variance_store(A, (int) x, (int) y, rgb, v);
            }
        in = dst, vin = vdst;
    }
    return AMVPT_OK;
}

amvpt_status amvpt_denoise_variance(const float *image_device, uint32_t channels, uint32_t width, uint32_t height,
                                    const float *variance_device, const float *guides_device,
                                    const amvpt_variance_params *params, float *out_device, float *scratch_device,
                                    float *var_out_device, float *var_scratch_device, void *stream) {
    const Refusal R("amvpt_denoise_variance");
    if (amvpt_status s = denoise_variance_check(R, image_device, channels, width, height, variance_device, guides_device, params,
                                                out_device, scratch_device, var_out_device, var_scratch_device))
        return s;
    if (amvpt_status s = R.need_device()) return s;
    uint64_t tx, ty;
    tile_grid(width, height, tx, ty);
    const dim3 grid((uint32_t) (tx * ty)), block(kTileBlock);
    hipStream_t st = (hipStream_t) stream;
    const float *in = image_device, *vin = variance_device;
    for (uint32_t i = 0; i < params->iterations; ++i) {
        float *dst = pingpong_dst(i, params->iterations, out_device, scratch_device);
        float *vdst = pingpong_dst(i, params->iterations, var_out_device, var_scratch_device);
        const DenoiseVarianceArgs A{in, vin, guides_device, dst, vdst, channels, width, height, (uint32_t) tx, variance_step(*params, i)};
        if (i == 0) hipLaunchKernelGGL(k_denoise_variance_tile<1>, grid, block, 0, st, A);
        else if (i == 1) hipLaunchKernelGGL(k_denoise_variance_tile<2>, grid, block, 0, st, A);
        else hipLaunchKernelGGL(k_denoise_variance_direct, grid, block, 0, st, A);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail("amvpt_denoise_variance launch", (int) e);
        in = dst, vin = vdst;
    }
    return AMVPT_OK;
}

} // extern "C"

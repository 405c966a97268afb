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

#include <atomic>
#include <cstdint>
#include <string>

#include "../../include/amvpt_variance.h"
#include "dvariance.h"
#include "internal.h"

namespace amvpt {

static constexpr int kTileW = 32, kTileH = 8;
static constexpr uint32_t kVarianceBlock = kTileW * kTileH;

struct VarianceArgs {
    const float *moments, *count, *guides;
    float *out;
    uint32_t w, h, tiles_x;
    VarianceConst K;
};

/* the pixels a block's 7 x 7 windows fall into, plane by plane as in VarianceTile below */
struct MomentTile {
    static constexpr int kHalo = 3, kW = kTileW + 2 * kHalo, kH = kTileH + 2 * kHalo, kN = kW * kH;
    float4 head[kN];      /* shape, normal */
    float view[kN];
    float pos[3][kN];
    float cnt[kN];
    float mom[2][kN];
};

struct MomentTileSrc {
    const MomentTile &T;
    int x0, y0;   /* image coordinates of the tile's first staged pixel */
    __device__ __forceinline__ int at(int x, int y) const { return (y - y0) * MomentTile::kW + (x - x0); }
    __device__ __forceinline__ void head(int x, int y, float g[4]) const {
        const float4 v = T.head[at(x, y)];
        g[0] = v.x, g[1] = v.y, g[2] = v.z, g[3] = v.w;
    }
    __device__ __forceinline__ float view(int x, int y) const { return T.view[at(x, y)]; }
    __device__ __forceinline__ void point(int x, int y, float p[3]) const {
        const int i = at(x, y);
        p[0] = T.pos[0][i], p[1] = T.pos[1][i], p[2] = T.pos[2][i];
    }
    __device__ __forceinline__ float count(int x, int y) const { return T.cnt[at(x, y)]; }
    __device__ __forceinline__ void moments(int x, int y, float m[2]) const {
        const int i = at(x, y);
        m[0] = T.mom[0][i], m[1] = T.mom[1][i];
    }
};

/* A block none of whose pixels takes the window (the steady state away from disocclusions) reads its own 16 bytes a
 * pixel and is done; a block with one stages its 38 x 14 pixels (44 bytes each, 22.9 KiB) in LDS once, and the
 * windows read LDS. */
__global__ void __launch_bounds__(kVarianceBlock) k_variance(VarianceArgs A) {
    __shared__ MomentTile T;
    const int bx = (int) (blockIdx.x % A.tiles_x) * kTileW, by = (int) (blockIdx.x / A.tiles_x) * kTileH;
    const int x = bx + (int) (threadIdx.x % kTileW), y = by + (int) (threadIdx.x / kTileW);
    const bool inside = x < (int) A.w && y < (int) A.h;
    const MomentPlanes P{A.moments, A.count, A.guides, A.w};
    const bool window = inside && variance_takes_window(P, x, y, A.K);
    if (!__syncthreads_or(window ? 1 : 0)) {
        if (inside) A.out[(size_t) y * A.w + (size_t) x] = variance_pixel(P, x, y, (int) A.w, (int) A.h, A.K);
        return;
    }
    const int x0 = bx - MomentTile::kHalo, y0 = by - MomentTile::kHalo;
    /* pixels outside the image stay unstaged: variance_pixel tests a tap's coordinates before it reads anything */
    for (int i = (int) threadIdx.x; i < MomentTile::kN; i += (int) kVarianceBlock) {
        const int gx = x0 + i % MomentTile::kW, gy = y0 + i / MomentTile::kW;
        if (gx < 0 || gy < 0 || gx >= (int) A.w || gy >= (int) A.h) continue;
        const size_t px = (size_t) gy * A.w + (size_t) gx;
        const float *r = A.guides + 8 * px;
        T.head[i] = make_float4(r[0], r[1], r[2], r[3]);
        T.pos[0][i] = r[4], T.pos[1][i] = r[5], T.pos[2][i] = r[6];
        T.view[i] = r[7];
        T.cnt[i] = A.count[px];
        T.mom[0][i] = A.moments[2 * px], T.mom[1][i] = A.moments[2 * px + 1];
    }
    __syncthreads();
    if (!inside) return;
    const MomentTileSrc src{T, x0, y0};
    A.out[(size_t) y * A.w + (size_t) x] = variance_pixel(src, x, y, (int) A.w, (int) A.h, A.K);
}

struct DenoiseVarianceArgs {
    const float *in, *vin, *guides;
    float *out, *vout;   /* vout may be null: the variance of the last iteration nobody asked for */
    uint32_t channels, w, h, tiles_x;
    VarianceStep K;
};

/* the pixel's RGB and variance, and with four channels the alpha of the iteration's input (the image's own) */
__device__ __forceinline__ void denoise_variance_store(const DenoiseVarianceArgs &A, int x, int y, const float rgb[3], float v) {
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

__global__ void __launch_bounds__(kVarianceBlock) k_denoise_variance_direct(DenoiseVarianceArgs A) {
    __shared__ PrefilterTile T;
    const int bx = (int) (blockIdx.x % A.tiles_x) * kTileW, by = (int) (blockIdx.x / A.tiles_x) * kTileH;
    const int x0 = bx - 1, y0 = by - 1;
    /* pixels outside the image stay unstaged: variance_prefilter tests a tap's coordinates before it reads anything */
    for (int i = (int) threadIdx.x; i < PrefilterTile::kN; i += (int) kVarianceBlock) {
        const int gx = x0 + i % PrefilterTile::kW, gy = y0 + i / PrefilterTile::kW;
        if (gx < 0 || gy < 0 || gx >= (int) A.w || gy >= (int) A.h) continue;
        const size_t px = (size_t) gy * A.w + (size_t) gx;
        T.shape[i] = A.guides[8 * px], T.view[i] = A.guides[8 * px + 7], T.var[i] = A.vin[px];
    }
    __syncthreads();
    const int x = bx + (int) (threadIdx.x % kTileW), y = by + (int) (threadIdx.x / kTileW);
    if (x >= (int) A.w || y >= (int) A.h) return;
    const VariancePlanes P{A.in, A.vin, A.guides, A.channels, A.w};
    const PrefilterTileSrc pre{T, x0, y0};
    float rgb[3], v;
    denoise_variance_pixel(P, pre, x, y, (int) A.w, (int) A.h, A.K, rgb, v);
    denoise_variance_store(A, x, y, rgb, v);
}

/* the staged pixels of one block, plane by plane: consecutive lanes read consecutive 16-byte heads (ds_read_b128)
 * and consecutive dwords of every other plane, so no read conflicts on a bank */
template <int S>
struct VarianceTile {
    static constexpr int kHalo = 2 * S, kW = kTileW + 2 * kHalo, kH = kTileH + 2 * kHalo, kN = kW * kH;
    float4 head[kN];      /* shape, normal */
    float view[kN];
    float pos[3][kN];
    float rgb[3][kN];
    float var[kN];
};

template <int S>
struct VarianceTileSrc {
    const VarianceTile<S> &T;
    int x0, y0;   /* image coordinates of the tile's first staged pixel */
    __device__ __forceinline__ int at(int x, int y) const { return (y - y0) * VarianceTile<S>::kW + (x - x0); }
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
    __device__ __forceinline__ float var(int x, int y) const { return T.var[at(x, y)]; }
    __device__ __forceinline__ float shape(int x, int y) const { return T.head[at(x, y)].x; }
};

template <int S>
__global__ void __launch_bounds__(kVarianceBlock) k_denoise_variance_tile(DenoiseVarianceArgs A) {
    using Tile = VarianceTile<S>;
    __shared__ Tile T;
    const int bx = (int) (blockIdx.x % A.tiles_x) * kTileW, by = (int) (blockIdx.x / A.tiles_x) * kTileH;
    const int x0 = bx - Tile::kHalo, y0 = by - Tile::kHalo;
    /* pixels outside the image stay unstaged: the per-pixel function tests a tap's coordinates before it reads anything,
     * and every tap of a pixel of this block, the prefilter's at step 1 among them, lies within the halo of 2 S */
    for (int i = (int) threadIdx.x; i < Tile::kN; i += (int) kVarianceBlock) {
        const int gx = x0 + i % Tile::kW, gy = y0 + i / Tile::kW;
        if (gx < 0 || gy < 0 || gx >= (int) A.w || gy >= (int) A.h) continue;
        const size_t px = (size_t) gy * A.w + (size_t) gx;
        const float *r = A.guides + 8 * px, *c = A.in + A.channels * px;
        T.head[i] = make_float4(r[0], r[1], r[2], r[3]);
        T.pos[0][i] = r[4], T.pos[1][i] = r[5], T.pos[2][i] = r[6];
        T.view[i] = r[7];
        T.rgb[0][i] = c[0], T.rgb[1][i] = c[1], T.rgb[2][i] = c[2];
        T.var[i] = A.vin[px];
    }
    __syncthreads();
    const int x = bx + (int) (threadIdx.x % kTileW), y = by + (int) (threadIdx.x / kTileW);
    if (x >= (int) A.w || y >= (int) A.h) return;
    VarianceStep K = A.K;
    K.step = S;
    const VarianceTileSrc<S> src{T, x0, y0};
    float rgb[3], v;
    denoise_variance_pixel(src, src, x, y, (int) A.w, (int) A.h, K, rgb, v);
    denoise_variance_store(A, x, y, rgb, v);
}

/* a visible device is remembered (it does not go away); its absence is asked again on the next call */
static bool variance_device_ok() {
    static std::atomic<bool> seen{false};
    if (seen.load(std::memory_order_relaxed)) return true;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return false;
    seen.store(true, std::memory_order_relaxed);
    return true;
}

static bool vr_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t a0 = (uintptr_t) a, b0 = (uintptr_t) b;
    return a0 < b0 + nb && b0 < a0 + na;
}

/* the parameter ranges, for all three of the struct's users */
static amvpt_status variance_params_check(const std::string &s, const amvpt_variance_params *p) {
    auto bad = [&](const std::string &what) { set_error(s + what); return AMVPT_ERR_INVALID; };
    if (p->iterations < 1u || p->iterations > 8u) return bad("params: iterations must be 1 .. 8, not " + std::to_string(p->iterations));
    if (!dn_finite(p->sigma_lum) || !(p->sigma_lum > 0.f)) return bad("params: sigma_lum must be finite and above 0");
    if (!dn_finite(p->var_floor) || !(p->var_floor > 0.f)) return bad("params: var_floor must be finite and above 0");
    if (!dn_finite(p->sigma_plane) || !(p->sigma_plane > 0.f)) return bad("params: sigma_plane must be finite and above 0");
    if (p->normal_squarings > 7u) return bad("params: normal_squarings must be 0 .. 7, not " + std::to_string(p->normal_squarings));
    if (p->min_history < 1u || p->min_history > 65535u)
        return bad("params: min_history must be 1 .. 65535, not " + std::to_string(p->min_history));
    return AMVPT_OK;
}

/* pixel coordinates are ints in the per-pixel functions of both entries, and one launch of 32 x 8 tiles covers the image */
static amvpt_status variance_size_check(const std::string &s, uint32_t w, uint32_t h) {
    auto bad = [&](const std::string &what) { set_error(s + what); return AMVPT_ERR_INVALID; };
    if (w == 0) return bad("width is 0");
    if (h == 0) return bad("height is 0");
    if (w > 0x7fffff00u || h > 0x7fffff00u) return bad("width or height above 2^31 - 256");
    const uint64_t tx = (w + (uint32_t) kTileW - 1u) / (uint32_t) kTileW, ty = (h + (uint32_t) kTileH - 1u) / (uint32_t) kTileH;
    if (tx * ty >= (1ull << 31)) return bad("width x height above 2^31 tiles of 32 x 8 pixels");
    return AMVPT_OK;
}

/* the refusals of both entries of stage 2; on success A holds everything but the launch geometry */
static amvpt_status variance_check(const char *who, const float *moments, const float *count, const float *guides, uint32_t w,
                                   uint32_t h, const amvpt_variance_params *p, float *out, VarianceArgs &A) {
    const std::string s = std::string(who) + ": ";
    auto bad = [&](const std::string &what) { set_error(s + what); return AMVPT_ERR_INVALID; };
    if (!moments) return bad("null moments");
    if (!count) return bad("null count");
    if (!guides) return bad("null guides");
    if (!p) return bad("null params");
    if (!out) return bad("null out");
    if (amvpt_status st = variance_size_check(s, w, h)) return st;
    if (amvpt_status st = variance_params_check(s, p)) return st;
    const size_t npx = (size_t) w * h, ncnt = npx * sizeof(float);
    if (vr_overlap(out, ncnt, moments, 2 * ncnt)) return bad("out overlaps the moments");
    if (vr_overlap(out, ncnt, count, ncnt)) return bad("out overlaps the count");
    if (vr_overlap(out, ncnt, guides, 8 * ncnt)) return bad("out overlaps the guides");
    A.moments = moments, A.count = count, A.guides = guides, A.out = out;
    A.w = w, A.h = h, A.tiles_x = 0;
    A.K.inv_sp = 1.f / p->sigma_plane;
    A.K.min_history = (float) p->min_history;
    A.K.squarings = p->normal_squarings;
    return AMVPT_OK;
}

/* the refusals of both entries of stage 3 */
static amvpt_status denoise_variance_check(const char *who, const float *image, uint32_t channels, uint32_t w, uint32_t h,
                                           const float *variance, const float *guides, const amvpt_variance_params *p,
                                           const float *out, const float *scratch, const float *var_out, const float *var_scratch) {
    const std::string s = std::string(who) + ": ";
    auto bad = [&](const std::string &what) { set_error(s + what); return AMVPT_ERR_INVALID; };
    if (!image) return bad("null image");
    if (!variance) return bad("null variance");
    if (!guides) return bad("null guides");
    if (!p) return bad("null params");
    if (!out) return bad("null out");
    if (channels != 3u && channels != 4u) return bad("channels must be 3 or 4, not " + std::to_string(channels));
    if (amvpt_status st = variance_size_check(s, w, h)) return st;
    if (amvpt_status st = variance_params_check(s, p)) return st;
    if (p->iterations > 1u && !scratch) return bad("null scratch (it may be null only when iterations is 1)");
    if (p->iterations > 1u && !var_scratch) return bad("null var_scratch (it may be null only when iterations is 1)");
    if (p->iterations > 2u && !var_out) return bad("null var_out (it may be null only when iterations is at most 2)");
    const size_t npx = (size_t) w * h, nvar = npx * sizeof(float), nimg = nvar * channels, ngd = nvar * 8;
    const struct { const void *p; size_t n; const char *name; } outs[4] = {
        {out, nimg, "out"}, {scratch, nimg, "scratch"}, {var_out, nvar, "var_out"}, {var_scratch, nvar, "var_scratch"}};
    const struct { const void *p; size_t n; const char *name; } ins[3] = {
        {image, nimg, "the image"}, {variance, nvar, "the variance"}, {guides, ngd, "the guides"}};
    for (int i = 0; i < 4; ++i) {
        if (!outs[i].p) continue;
        for (const auto &in : ins)
            if (vr_overlap(outs[i].p, outs[i].n, in.p, in.n)) return bad(std::string(outs[i].name) + " overlaps " + in.name);
        for (int j = 0; j < i; ++j)
            if (outs[j].p && vr_overlap(outs[i].p, outs[i].n, outs[j].p, outs[j].n))
                return bad(std::string(outs[i].name) + " overlaps " + outs[j].name);
    }
    return AMVPT_OK;
}

/* iteration i: its constants; and where iteration i of n writes -- the two buffers of a pair take turns so that the
 * last iteration lands in the first */
static VarianceStep variance_step(const amvpt_variance_params &p, uint32_t i) {
    VarianceStep K;
    K.sl2 = p.sigma_lum * p.sigma_lum;
    K.var_floor = p.var_floor;
    K.inv_sp = 1.f / p.sigma_plane;
    K.squarings = p.normal_squarings;
    K.step = (int32_t) (1u << i);
    return K;
}
static float *variance_dst(uint32_t i, uint32_t n, float *out, float *scratch) { return ((n - 1u - i) & 1u) ? scratch : out; }

/* the launch geometry of a checked size (variance_size_check) */
static amvpt_status variance_grid(const std::string &who, uint32_t width, uint32_t height, uint64_t &tx, uint64_t &ty) {
    tx = (width + (uint32_t) kTileW - 1u) / (uint32_t) kTileW, ty = (height + (uint32_t) kTileH - 1u) / (uint32_t) kTileH;
    if (!variance_device_ok()) { set_error(who + ": no HIP device visible"); return AMVPT_ERR_NO_DEVICE; }
    return AMVPT_OK;
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
    if (amvpt_status s = variance_check("amvpt_variance_host", moments, count, guides, width, height, params, out, A)) return s;
    const MomentPlanes P{moments, count, guides, width};
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x)
            out[(size_t) y * width + x] = variance_pixel(P, (int) x, (int) y, (int) width, (int) height, A.K);
    return AMVPT_OK;
}

amvpt_status amvpt_variance(const float *moments_device, const float *count_device, const float *guides_device,
                            uint32_t width, uint32_t height, const amvpt_variance_params *params, float *out_device,
                            void *stream) {
    VarianceArgs A;
    if (amvpt_status s = variance_check("amvpt_variance", moments_device, count_device, guides_device, width, height, params,
                                        out_device, A))
        return s;
    uint64_t tx, ty;
    if (amvpt_status s = variance_grid("amvpt_variance", width, height, tx, ty)) return s;
    A.tiles_x = (uint32_t) tx;
    hipLaunchKernelGGL(k_variance, dim3((uint32_t) (tx * ty)), dim3(kVarianceBlock), 0, (hipStream_t) stream, A);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail("amvpt_variance launch", (int) e);
    return AMVPT_OK;
}

amvpt_status amvpt_denoise_variance_host(const float *image, uint32_t channels, uint32_t width, uint32_t height,
                                         const float *variance, const float *guides, const amvpt_variance_params *params,
                                         float *out, float *scratch, float *var_out, float *var_scratch) {
    if (amvpt_status s = denoise_variance_check("amvpt_denoise_variance_host", image, channels, width, height, variance, guides,
                                                params, out, scratch, var_out, var_scratch))
        return s;
    const float *in = image, *vin = variance;
    for (uint32_t i = 0; i < params->iterations; ++i) {
        const VarianceStep K = variance_step(*params, i);
        float *dst = variance_dst(i, params->iterations, out, scratch);
        float *vdst = variance_dst(i, params->iterations, var_out, var_scratch);
        const VariancePlanes P{in, vin, guides, channels, width};
        for (uint32_t y = 0; y < height; ++y)
            for (uint32_t x = 0; x < width; ++x) {
                float rgb[3], v;
                denoise_variance_pixel(P, P, (int) x, (int) y, (int) width, (int) height, K, rgb, v);
                const size_t px = (size_t) y * width + x, at = px * channels;
                dst[at] = rgb[0], dst[at + 1] = rgb[1], dst[at + 2] = rgb[2];
                if (channels == 4u) dst[at + 3] = in[at + 3];
                if (vdst) vdst[px] = v;
            }
        in = dst, vin = vdst;
    }
    return AMVPT_OK;
}

amvpt_status amvpt_denoise_variance(const float *image_device, uint32_t channels, uint32_t width, uint32_t height,
                                    const float *variance_device, const float *guides_device,
                                    const amvpt_variance_params *params, float *out_device, float *scratch_device,
                                    float *var_out_device, float *var_scratch_device, void *stream) {
    if (amvpt_status s = denoise_variance_check("amvpt_denoise_variance", image_device, channels, width, height, variance_device,
                                                guides_device, params, out_device, scratch_device, var_out_device,
                                                var_scratch_device))
        return s;
    uint64_t tx, ty;
    if (amvpt_status s = variance_grid("amvpt_denoise_variance", width, height, tx, ty)) return s;
    const dim3 grid((uint32_t) (tx * ty)), block(kVarianceBlock);
    hipStream_t st = (hipStream_t) stream;
    const float *in = image_device, *vin = variance_device;
    for (uint32_t i = 0; i < params->iterations; ++i) {
        float *dst = variance_dst(i, params->iterations, out_device, scratch_device);
        float *vdst = variance_dst(i, params->iterations, var_out_device, var_scratch_device);
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

/*
 * dtile.h -- what the post-process kernels share on the device (amvpt_denoise.hip, amvpt_temporal.hip,
 * amvpt_variance.hip, amvpt_synth.hip): the 32 x 8 pixel block of a flat grid, and the LDS tile a block stages its
 * pixels and their halo in, with the source the per-pixel functions read it through (dpost.h has the source in memory).
 */
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace amvpt {

static constexpr int kTileW = 32, kTileH = 8;
static constexpr uint32_t kTileBlock = kTileW * kTileH;

/* block blockIdx.x of a flat grid with tiles_x blocks per row: its first pixel (bx, by) and the thread's own (x, y) */
struct TilePixel {
    int bx, by, x, y;
};
__device__ __forceinline__ TilePixel tile_pixel(uint32_t tiles_x) {
    TilePixel p;
    p.bx = (int) (blockIdx.x % tiles_x) * kTileW, p.by = (int) (blockIdx.x / tiles_x) * kTileH;
    p.x = p.bx + (int) (threadIdx.x % kTileW), p.y = p.by + (int) (threadIdx.x / kTileW);
    return p;
}

/* the staged guide records of one block and its halo, plane by plane: consecutive lanes read consecutive 16-byte heads
 * (ds_read_b128) and consecutive dwords of every other plane, so no read conflicts on a bank.  A stage derives from
 * this and adds its own planes of kN floats */
template <int kHalo_>
struct GuideTile {
    static constexpr int kHalo = kHalo_, kW = kTileW + 2 * kHalo, kH = kTileH + 2 * kHalo, kN = kW * kH;
    float4 head[kN];      /* shape, normal */
    float view[kN];
    float pos[3][kN];
    /* staged pixel i takes the guide record r */
    __device__ __forceinline__ void stage(int i, const float *r) {
        head[i] = make_float4(r[0], r[1], r[2], r[3]);
        pos[0][i] = r[4], pos[1][i] = r[5], pos[2][i] = r[6];
        view[i] = r[7];
    }
};

/* the source over a tile whose first staged pixel is (x0, y0) of the image; derive to read the planes a tile adds */
template <class Tile>
struct GuideTileSrc {
    const Tile &T;
    int x0, y0;
    __device__ __forceinline__ int at(int x, int y) const { return (y - y0) * Tile::kW + (x - x0); }
    __device__ __forceinline__ void head(int x, int y, float g[4]) const {
        const float4 v = T.head[at(x, y)];
        g[0] = v.x, g[1] = v.y, g[2] = v.z, g[3] = v.w;
    }
    __device__ __forceinline__ float view(int x, int y) const { return T.view[at(x, y)]; }
    __device__ __forceinline__ void point(int x, int y, float p[3]) const {
        const int i = at(x, y);
        p[0] = T.pos[0][i], p[1] = T.pos[1][i], p[2] = T.pos[2][i];
    }
    __device__ __forceinline__ float shape(int x, int y) const { return T.head[at(x, y)].x; }
};

/* the staging loop of a block: every pixel of the Tile::kW x Tile::kH rectangle at (x0, y0) that lies inside the
 * w x h image goes to f(i, px), i its place in the tile and px its place in the image.  Pixels outside stay unstaged:
 * the per-pixel functions test a tap's coordinates before they read anything */
template <class Tile, class F>
__device__ __forceinline__ void tile_stage(int x0, int y0, uint32_t w, uint32_t h, F f) {
    for (int i = (int) threadIdx.x; i < Tile::kN; i += (int) kTileBlock) {
        const int gx = x0 + i % Tile::kW, gy = y0 + i / Tile::kW;
        if (gx < 0 || gy < 0 || gx >= (int) w || gy >= (int) h) continue;
        f(i, (size_t) gy * w + (size_t) gx);
    }
}

} // namespace amvpt

/*
 * ddisplay.h -- the per-element functions of the display stage (include/amvpt_display.h).  The kernels of
 * amvpt_display.hip and its host-only entries call these same functions.  The interlacer is float32 in the
 * reference's order, the sRGB curve float64 built from +, -, * alone; everything is unfused (-ffp-contract=off) and
 * no library function beyond floorf / rint is called, so host and device agree bit for bit.
 *
 * Reference: Program::display_image (src/mitsuba/program.cpp:199-276, screenshot branch), clip / mod / lerp2 /
 * interpolate2d (src/mitsuba/util.h:53-55, 104-129), StructConverter::save (src/core/struct.cpp:1645-1667).
 */
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace amvpt {

#define DHD __host__ __device__ __forceinline__

/* what display_image hoists out of its loops (program.cpp:224-229), formed once on the host */
struct DisplayParams {
    float center, focus, pitch, tilt, subp;
    float gx;               /* (float) grid[0], mod's divisor */
    float grid_n, grid_scl; /* grid[0] * grid[1] and its reciprocal */
    float igx;              /* igrid[0] (the reference uses it for the row too) */
    float vix, viy;         /* view * igrid, formed first (program.cpp:261) */
    float dsx, dsy;         /* dst_scl = 1 / ((3W, H) - 1) */
    float ssx, ssy;         /* src_scl = src_dim - 1 */
    uint32_t sw, sh, nch;   /* the source */
    uint32_t dw, dh;        /* the destination, in pixels */
    uint32_t quilt, nearest;
};

/* clip (util.h:53) for every ordered argument; a NaN gives 0 where std::min(std::max()) passes it on, so that
 * no texel index is ever formed from one (the cast would be undefined) */
DHD float dclip(float x) { return x > 0.f ? (x < 1.f ? x : 1.f) : 0.f; }

/* x^(1/2.4) = x^(5/12) for 0.003 < x < 1 from float64 +, -, * alone, so that host and device give the same bits
 * (a library pow is each platform's own).  r = x^(-1/12) by Newton's r <- r (13 - x r^12) / 12 from the
 * log-linear guess bits(r) = 13/12 bits(1) - bits(x) / 12, centred by 0.0465 in the exponent: within 3.3 %.  The
 * error e goes to 6.5 e^2 per step: 7.9e-3, 3.9e-4, 1.0e-6, 6.6e-12, then the rounding floor at the fifth step.
 * x r^7 = x^(5/12) is then within 3e-15 of the true value (relative), 8e-13 of a code. */
DHD double pow_5_12(double x) {
    uint64_t i;
    __builtin_memcpy(&i, &x, 8);
    i = 0x45434189374bc6a8ull - i / 12u;   /* 13/12 * 0x3ff0000000000000 - 0.0465 * 2^52 */
    double r;
    __builtin_memcpy(&r, &i, 8);
    for (int k = 0; k < 5; ++k) {
        const double r2 = r * r, r4 = r2 * r2, r6 = r4 * r2, r12 = r6 * r6;
        r = r * ((13.0 - x * r12) * (1.0 / 12.0));
    }
    const double r2 = r * r, r4 = r2 * r2;
    return x * (r4 * r2 * r);
}

/* linear -> 8-bit sRGB: IEC 61966-2-1, x 255, clamp, round to nearest even; NaN -> 0 (amvpt_display.h).  The
 * curve is evaluated in float64 (the reference's float32 linear_to_srgb is within 4.3e-5 code units of it). */
DHD uint8_t srgb8_value(float xf) {
    const double x = (double) xf;
    if (!(x > 0.0)) return 0;      /* negatives, -0, -inf and NaN */
    if (x >= 1.0) return 255;      /* 1 maps to 255 exactly; above it and +inf clamp */
    double v = x <= 0.0031308 ? 12.92 * x : 1.055 * pow_5_12(x) - 0.055;
    v *= 255.0;
    v = v > 0.0 ? (v < 255.0 ? v : 255.0) : 0.0;
    return (uint8_t) rint(v);
}

/* the view index z1 of subpixel c of pixel (px, dy), and its quilt coordinate xy in [0, 1]^2 */
DHD float interlace_coord(const DisplayParams &P, uint32_t px, uint32_t dy, uint32_t c, float &x, float &y) {
    const float y0 = (float) dy * P.dsy;
    const float x0 = (float) (3u * px) * P.dsx;   /* over the byte index: the last pixel's x0 is (3W-3)/(3W-1) */
    float z = P.pitch * (x0 + (float) c * P.subp + (1.f - y0) * P.tilt) - P.center;
    z = 1.f - (z - floorf(z));
    const float z1 = floorf(z * P.grid_n);          /* camera id */
    const float z2 = floorf((1.f - z) * P.grid_n);  /* inverse camera id */
    const float w = P.focus * (1.f - 2.f * dclip(z1 * P.grid_scl));   /* depth */
    const float X = (z1 - P.gx * floorf(z1 / P.gx)) + dclip(x0 + w);
    const float Y = floorf(z2 * P.igx) + y0;
    x = P.quilt ? x0 : dclip(P.vix * X);
    y = P.quilt ? y0 : dclip(P.viy * Y);
    return z1;
}

/* lerp2<uint8_t, float> (util.h:55): the float result truncated to a byte */
DHD uint8_t lerp2_u8(uint8_t a, uint8_t b, float t) { return (uint8_t) ((1.f - t) * (float) a + t * (float) b); }

/* interpolate2d<uint8_t> (util.h:104-129) at xy = src_scl * (x, y); indices are held inside the source */
DHD uint8_t interpolate2d_u8(const uint8_t *src, const DisplayParams &P, float x, float y, uint32_t c) {
    x = P.ssx * x;
    y = P.ssy * y;
    const uint32_t w = P.sw, h = P.sh;
    if (P.nearest) {
        uint32_t x1 = (uint32_t) (x + 0.5f), y1 = (uint32_t) (y + 0.5f);
        x1 = x1 < w ? x1 : w - 1;
        y1 = y1 < h ? y1 : h - 1;
        return src[((size_t) x1 + (size_t) y1 * w) * P.nch + c];
    }
    uint32_t x1 = (uint32_t) x, y1 = (uint32_t) y;
    x1 = x1 < w ? x1 : w - 1;
    y1 = y1 < h ? y1 : h - 1;
    const float tx = x - (float) x1, ty = y - (float) y1;
    const uint32_t x2 = x1 + 1 < w ? x1 + 1 : x1;
    const uint32_t y2 = y1 + 1 < h ? y1 + 1 : y1;
    const size_t r1 = (size_t) y1 * w, r2 = (size_t) y2 * w;
    const uint8_t a00 = src[(x1 + r1) * P.nch + c];
    const uint8_t a10 = src[(x2 + r1) * P.nch + c];
    const uint8_t a01 = src[(x1 + r2) * P.nch + c];
    const uint8_t a11 = src[(x2 + r2) * P.nch + c];
    return lerp2_u8(lerp2_u8(a00, a10, tx), lerp2_u8(a01, a11, tx), ty);
}

/* one subpixel of the interlaced image */
DHD uint8_t interlace_value(const uint8_t *src, const DisplayParams &P, uint32_t px, uint32_t dy, uint32_t c) {
    float x, y;
    (void) interlace_coord(P, px, dy, c, x, y);
    return interpolate2d_u8(src, P, x, y, c);
}

#undef DHD

/* device only, for the kernels that write RGB bytes (amvpt_display.hip, amvpt_tonemap.hip) */
static __device__ __forceinline__ uint32_t pack4(uint8_t a, uint8_t b, uint8_t c, uint8_t d) {
    return (uint32_t) a | ((uint32_t) b << 8) | ((uint32_t) c << 16) | ((uint32_t) d << 24);
}

/* 12 bytes at out (the bytes of four RGB pixels): three dword stores, or byte stores */
template <bool kDword> static __device__ __forceinline__ void store12(uint8_t *out, const uint8_t *v) {
    if (kDword) {
        uint32_t *o = reinterpret_cast<uint32_t *>(out);
        o[0] = pack4(v[0], v[1], v[2], v[3]);
        o[1] = pack4(v[4], v[5], v[6], v[7]);
        o[2] = pack4(v[8], v[9], v[10], v[11]);
    } else {
#pragma unroll
        for (uint32_t i = 0; i < 12; ++i) out[i] = v[i];
    }
}

} // namespace amvpt

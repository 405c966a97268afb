/*
 * amvpt_display.h -- the display stage of libamvpt_hip.so: the developed quilt as 8-bit sRGB, and
 * that quilt interlaced into the native image of a lenticular light-field display.
 *
 * Reference interfaces replaced (file:line in xacond00/mitsuba3-amvpt):
 *   amvpt_srgb8     <- Bitmap::convert(RGB, UInt8, srgb_gamma = true), src/mitsuba/program.h:55,
 *                      per value StructConverter::save, src/core/struct.cpp:1645-1667
 *   amvpt_interlace <- the screenshot branch of Program::display_image, src/mitsuba/program.cpp:199-276
 *                      (dst_ch = 3, flip_rgb = true), with interpolate2d, src/mitsuba/util.h:104-129
 *   amvpt_display_preset <- Preset, src/mitsuba/preset.h:12-17
 *
 * These are new entry points only: no struct of amvpt.h changes, AMVPT_ABI_VERSION stays as it is and
 * this header carries a version of its own.  Status codes and amvpt_last_error() are amvpt.h's.
 *
 * Numerics.  amvpt_interlace is integer and unfused IEEE float32 arithmetic ending in a byte: the device
 * entry, the host entry and a float32 restatement of the reference agree byte for byte.  amvpt_srgb8 is
 * the IEC 61966-2-1 curve  x <= 0.0031308 ? 12.92 x : 1.055 x^(1/2.4) - 0.055  (the function the
 * reference's dr::linear_to_srgb approximates), times 255, clamped to [0, 255], rounded to nearest even.
 * It is evaluated in float64 with the power formed from +, -, * alone, so host and device agree byte for
 * byte here too, within 1e-12 of a code of the exact curve (the reference's float32 evaluation is within
 * 4.3e-5 of it: the two can differ only where the exact value lies that close to a half-integer).
 * Negative values and -inf give 0, values above 1 and +inf give 255.  NaN gives 0: the reference casts a
 * NaN double to an integer there, which C++ leaves undefined, so the choice is this library's.  No
 * dithering (the reference converts without it).
 */
#ifndef AMVPT_DISPLAY_H
#define AMVPT_DISPLAY_H

#include "amvpt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AMVPT_DISPLAY_VERSION 1

/* A lenticular display's calibration (Preset, preset.h:12-17).  flip_rgb is carried for the presets.csv
 * round trip; the exported image ignores it, as the screenshot branch does (program.cpp:215). */
typedef struct amvpt_display_preset {
    float center, focus, pitch, tilt, subp;
    float view[2];
    int32_t grid[2];
    uint32_t flip_rgb;
} amvpt_display_preset;

uint32_t amvpt_display_version(void);

/* The reference's LKG4x8 (program.h:74-75): -0.5, -0.05, 354.548, -0.114, 0.00013, view (1, 1), grid (4, 8). */
amvpt_display_preset amvpt_display_default_preset(void);

/*
 * Developed float32 image (height x width x channels, channels 3 or 4: what amvpt_develop writes) ->
 * height x width x 3 uint8, sRGB.  Alpha is dropped.  Device pointers; ordered on `stream`.
 * AMVPT_ERR_INVALID: a null pointer, channels not 3 or 4, a dimension of 0, more than 2^33 pixels (one
 * launch covers the image).
 */
amvpt_status amvpt_srgb8(const float *image_device, uint32_t channels, uint32_t width, uint32_t height,
                         uint8_t *out_device, void *stream);

/*
 * 8-bit quilt (src_h x src_w x src_channels, channels 3 or 4) -> dst_h x dst_w x 3 uint8: every subpixel
 * picks its view from pitch / tilt / center / subp, shifts by focus and resamples the quilt, bilinearly
 * (every lerp truncated to a byte, as interpolate2d<uint8_t> does) or (nearest != 0) at the nearest texel.
 * quilt != 0 resamples the whole quilt to dst_w x dst_h instead ("Display quilt").  Device pointers;
 * ordered on `stream`; the source is only read.
 * AMVPT_ERR_INVALID, naming the argument: dst_w < 2 or dst_h < 2 (the reference divides by dst - 1),
 * a source dimension of 0, grid[i] < 1, src_channels not 3 or 4, a null pointer, a preset field that is
 * not finite, more than 2^33 destination pixels (device entry only).
 */
amvpt_status amvpt_interlace(const uint8_t *src_device, uint32_t src_w, uint32_t src_h, uint32_t src_channels,
                             const amvpt_display_preset *preset, int quilt, int nearest, uint8_t *dst_device,
                             uint32_t dst_w, uint32_t dst_h, void *stream);

/* The same functions over host pointers, compiled for the host from the same per-element code: they
 * need no device and never return AMVPT_ERR_NO_DEVICE. */
amvpt_status amvpt_srgb8_host(const float *image, uint32_t channels, uint32_t width, uint32_t height, uint8_t *out);
amvpt_status amvpt_interlace_host(const uint8_t *src, uint32_t src_w, uint32_t src_h, uint32_t src_channels,
                                  const amvpt_display_preset *preset, int quilt, int nearest, uint8_t *dst,
                                  uint32_t dst_w, uint32_t dst_h);

/* The view index (z1, the "camera id" of display_image) every subpixel of a dst_w x dst_h image picks:
 * dst_h x dst_w x 3 int32.  Host only. */
amvpt_status amvpt_interlace_views_host(const amvpt_display_preset *preset, int32_t *views, uint32_t dst_w,
                                        uint32_t dst_h);

#ifdef __cplusplus
}
#endif

#endif /* AMVPT_DISPLAY_H */

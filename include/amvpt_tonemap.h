/*
 * amvpt_tonemap.h -- the tone-mapping stage of libamvpt_hip.so: a metered exposure for the whole quilt and a
 * tone-reproduction operator in front of the 8-bit sRGB conversion of amvpt_display.h.
 *
 * The reference's front end has nothing here (Program::display_image converts and clips), so the definition below is
 * this library's own and is normative.  These are new entry points only: no struct of amvpt.h changes,
 * AMVPT_ABI_VERSION stays as it is and this header carries a version of its own.  Status codes and
 * amvpt_last_error() are amvpt.h's.
 *
 * All views of a quilt are seen at once on one panel, so the exposure is one number for the whole quilt, and it
 * moves from frame to frame by a fixed share of the remaining gap (adapt) instead of jumping.
 *
 * Metering.  The luminance of a pixel is (0.2126 r + 0.7152 g) + 0.0722 b in unfused float32 (Rec. 709).  A pixel
 * whose luminance is NaN, not finite, zero, negative or below 2^-16 is added to state.skipped and to no bin.  Every
 * other pixel falls in one of 512 bins, sixteen per octave, over [2^-16, 2^16):
 *     bin = 16 * (E + 16) + j
 * with E the unbiased exponent read from the float's bits and j the number of entries of the table 2^(j/16),
 * j = 1 .. 15, rounded to float32, that are <= the significand in [1, 2).  A luminance of 2^16 or more goes to bin
 * 511.  This is integer and compare arithmetic only (no logarithm is evaluated), so the bin of a value is the same on
 * host and device by construction.  Counts are uint32_t and integer adds commute: the histogram is exact and does not
 * depend on scheduling.  An image or rectangle of 2^32 pixels or more is refused.
 *
 * Exposure.  From the histogram, in float64, serially in bin order:
 *     N     = counted (the sum of the bins)
 *     n_lo  = floor((double) lo * N),  n_hi = floor((double) hi * N), raised to n_lo + 1 where it is not above n_lo
 *             and held to N
 *     ov_b  = the integer overlap of [cum_b, cum_b + count_b) with [n_lo, n_hi), cum_b the counts before bin b
 *     S = sum ov_b * b,  M = sum ov_b                                  (64-bit integers)
 *     mean  = -16 + (S / M + 0.5) / 16                                 (the trimmed mean log2 luminance)
 *     l_target = clamp(ev - mean, min_ev, max_ev)
 *     l     = l_prev + (l_target - l_prev) * adapt,  l = l_target where state.frames == 0
 *     exposure = (float) ((double) key * exp2_pm(l)),  frames += 1
 * With N == 0, l, exposure and frames stay as they were, except that a fresh state (frames == 0) takes l = ev and
 * the exposure that gives.  exp2_pm is 2^x from float64 +, -, * and bit construction of the exponent, within 1e-12
 * (relative) of the correctly rounded value over [-40, 40]; S / M is the correctly rounded float64 quotient.  Host
 * and device give the same bits, the double included.
 *
 * The exposure used.  With params.auto_exposure != 0 the kernels read state->exposure from device memory; nothing
 * returns to the host between metering and tone mapping.  With auto_exposure == 0 the state may be null and the
 * exposure is (float) ((double) key / 0.18 * exp2_pm(ev)): with the default key, ev = 0 is the identity.
 *
 * Operators.  Float32, unfused, correctly rounded division.  x_c = c * exposure for the three colour channels, then
 *     AMVPT_TONEMAP_LINEAR    y_c = x_c
 *     AMVPT_TONEMAP_REINHARD  the extended Reinhard operator on luminance, which keeps hue: L the luminance of x;
 *                             where L is finite and above 0, s = (1 + L / (white * white)) / (1 + L) and
 *                             y_c = x_c * s; otherwise y_c = x_c
 *     AMVPT_TONEMAP_ACES      Narkowicz's fit, per channel: y = x (2.51 x + 0.03) / (x (2.43 x + 0.59) + 0.14);
 *                             x <= 0 gives 0, x above 2^60 gives the float 2.51f / 2.43f, NaN stays NaN
 * amvpt_tonemap_apply writes y as floats and passes a fourth channel through; amvpt_tonemap_srgb8 writes
 * amvpt_srgb8's byte of y_c (the same function, amvpt_display.h "Numerics"): it reads the frame once and never
 * writes a float frame.  Device entry and host entry agree bit for bit, byte for byte.
 */
#ifndef AMVPT_TONEMAP_H
#define AMVPT_TONEMAP_H

#include "amvpt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AMVPT_TONEMAP_VERSION 1
#define AMVPT_TONEMAP_BINS 512

enum { AMVPT_TONEMAP_LINEAR = 0, AMVPT_TONEMAP_REINHARD = 1, AMVPT_TONEMAP_ACES = 2 };

typedef struct amvpt_tonemap_params {
    uint32_t op;              /* AMVPT_TONEMAP_*; default LINEAR */
    uint32_t auto_exposure;   /* != 0: the exposure is the state's; default 0 */
    float ev;                 /* exposure compensation in stops; default 0 */
    float key;                /* the value the metered mean is brought to; default 0.18 */
    float lo, hi;             /* the share of the counted pixels the mean is taken over; default 0.10, 0.95 */
    float adapt;              /* the share of the gap in log2 exposure closed per metered frame; default 1 */
    float white;              /* REINHARD: the luminance that maps to 1; default 4 */
    float min_ev, max_ev;     /* the bounds of log2 exposure / key; default -16, 16 */
} amvpt_tonemap_params;

/* In caller-owned memory: device memory for the device entries, host memory for the host entries.  A zero-filled
 * state is a fresh one.  amvpt_tonemap_meter zeroes hist, counted and skipped at its start and keeps the rest. */
typedef struct amvpt_tonemap_state {
    uint32_t hist[AMVPT_TONEMAP_BINS];
    uint32_t counted, skipped;
    uint32_t frames;
    float exposure;
    double log2_exposure;
} amvpt_tonemap_state;

uint32_t amvpt_tonemap_version(void);
amvpt_tonemap_params amvpt_tonemap_default_params(void);

/*
 * Meter the developed float32 image (height x width x channels, channels 3 or 4) into *state and update its
 * exposure.  rect = {x0, y0, w, h} in pixels restricts the metering (null: the whole image).  Device pointers;
 * ordered on `stream`: a fill of the counts, the histogram kernel, the one-block exposure kernel.
 * AMVPT_ERR_INVALID, by name: a null pointer, channels not 3 or 4, a dimension of 0, a parameter out of range (below),
 * a rectangle that is empty or leaves the image, 2^32 pixels or more, a state that overlaps the image.
 */
amvpt_status amvpt_tonemap_meter(const float *image_device, uint32_t channels, uint32_t width, uint32_t height,
                                 const uint32_t rect[4], const amvpt_tonemap_params *params,
                                 amvpt_tonemap_state *state_device, void *stream);

/*
 * image -> out_device, height x width x channels float32; alpha is passed through.  out_device may be image_device
 * itself, exactly; any other overlap is refused.  state_device may be null unless params->auto_exposure is set.
 * Parameter ranges: op one of the three; every field finite; key > 0; white > 0; 0 <= lo < hi <= 1;
 * 0 <= adapt <= 1; min_ev <= max_ev.
 */
amvpt_status amvpt_tonemap_apply(const float *image_device, uint32_t channels, uint32_t width, uint32_t height,
                                 const amvpt_tonemap_params *params, const amvpt_tonemap_state *state_device,
                                 float *out_device, void *stream);

/* image -> out_device, height x width x 3 uint8 sRGB of the mapped colours: amvpt_srgb8 fused behind the operator.
 * More than 2^33 pixels are refused (one launch covers the image). */
amvpt_status amvpt_tonemap_srgb8(const float *image_device, uint32_t channels, uint32_t width, uint32_t height,
                                 const amvpt_tonemap_params *params, const amvpt_tonemap_state *state_device,
                                 uint8_t *out_device, void *stream);

/* The same functions over host pointers, compiled for the host from the same per-pixel code: they need no device
 * and never return AMVPT_ERR_NO_DEVICE. */
amvpt_status amvpt_tonemap_meter_host(const float *image, uint32_t channels, uint32_t width, uint32_t height,
                                      const uint32_t rect[4], const amvpt_tonemap_params *params,
                                      amvpt_tonemap_state *state);
amvpt_status amvpt_tonemap_apply_host(const float *image, uint32_t channels, uint32_t width, uint32_t height,
                                      const amvpt_tonemap_params *params, const amvpt_tonemap_state *state, float *out);
amvpt_status amvpt_tonemap_srgb8_host(const float *image, uint32_t channels, uint32_t width, uint32_t height,
                                      const amvpt_tonemap_params *params, const amvpt_tonemap_state *state,
                                      uint8_t *out);

/* exp2_pm (above) at x, for tests.  Host only. */
double amvpt_tonemap_exp2_host(double x);

#ifdef __cplusplus
}
#endif

#endif /* AMVPT_TONEMAP_H */

/*
 * dtonemap.h -- the per-pixel and per-histogram functions of the tone-mapping stage (include/amvpt_tonemap.h).  The
 * kernels of amvpt_tonemap.hip and its host-only entries call these same functions.  The bin of a luminance is integer
 * and compare arithmetic on the float's bits; the exposure is float64 +, -, *, one correctly rounded division and a
 * power of two built from its bits; the operators are unfused float32 (-ffp-contract=off) with correctly rounded
 * division.  No library function is called, so host and device agree bit for bit.
 */
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/amvpt_tonemap.h"
#include "ddisplay.h"
#include "dpost.h"

namespace amvpt {

#define TM_HD __host__ __device__ __forceinline__

static constexpr uint32_t kTmBins = AMVPT_TONEMAP_BINS;   /* sixteen per octave over [2^-16, 2^16) */
static constexpr int32_t kTmSkipped = -1;                  /* tm_bin of a pixel that is not metered */

/* the number of entries of 2^(j/16), j = 1 .. 15 (rounded to float32), that are <= s, for s in [1, 2); as selects */
TM_HD uint32_t tm_sixteenth(float s) {
    return (uint32_t) (s >= 0x1.0b5586p+0f) + (uint32_t) (s >= 0x1.172b84p+0f) + (uint32_t) (s >= 0x1.2387a6p+0f) +
           (uint32_t) (s >= 0x1.306fe0p+0f) + (uint32_t) (s >= 0x1.3dea64p+0f) + (uint32_t) (s >= 0x1.4bfdaep+0f) +
           (uint32_t) (s >= 0x1.5ab07ep+0f) + (uint32_t) (s >= 0x1.6a09e6p+0f) + (uint32_t) (s >= 0x1.7a1148p+0f) +
           (uint32_t) (s >= 0x1.8ace54p+0f) + (uint32_t) (s >= 0x1.9c4918p+0f) + (uint32_t) (s >= 0x1.ae89fap+0f) +
           (uint32_t) (s >= 0x1.c199bep+0f) + (uint32_t) (s >= 0x1.d5818ep+0f) + (uint32_t) (s >= 0x1.ea4afap+0f);
}

/* the histogram bin of the luminance L, or kTmSkipped: NaN, +-inf, zero, negatives and everything below 2^-16 (the
 * denormals among it) are skipped, 2^16 and above goes to the last bin */
TM_HD int32_t tm_bin(float L) {
    uint32_t u;
    __builtin_memcpy(&u, &L, 4);
    if (u >> 31) return kTmSkipped;            /* negatives, -0, -inf, NaN with the sign set */
    const uint32_t e = u >> 23;                /* the biased exponent */
    if (e == 255u || e < 127u - 16u) return kTmSkipped;
    if (e >= 127u + 16u) return (int32_t) kTmBins - 1;
    const uint32_t sb = (u & 0x007fffffu) | 0x3f800000u;
    float s;
    __builtin_memcpy(&s, &sb, 4);
    return (int32_t) (16u * (e - (127u - 16u)) + tm_sixteenth(s));
}

/* 2^x from float64 +, -, * and the exponent's bits: x = n + f with n the nearest integer, 2^f = exp(f ln 2) by its
 * Taylor polynomial of degree 13 (|f ln 2| <= 0.3466: the remainder is below 4e-18, the Horner rounding a few 1e-16),
 * times 2^n.  x is held to [-1022, 1023] (a NaN gives 2^-1022); the callers pass finite exposures of a few tens. */
TM_HD double exp2_pm(double x) {
    x = x > -1022.0 ? (x < 1023.0 ? x : 1023.0) : -1022.0;
    const int32_t n = (int32_t) (x + (x < 0.0 ? -0.5 : 0.5));
    const double t = (x - (double) n) * 0.69314718055994530942;
    double p = 1.0 / 6227020800.0;
    p = p * t + 1.0 / 479001600.0;
    p = p * t + 1.0 / 39916800.0;
    p = p * t + 1.0 / 3628800.0;
    p = p * t + 1.0 / 362880.0;
    p = p * t + 1.0 / 40320.0;
    p = p * t + 1.0 / 5040.0;
    p = p * t + 1.0 / 720.0;
    p = p * t + 1.0 / 120.0;
    p = p * t + 1.0 / 24.0;
    p = p * t + 1.0 / 6.0;
    p = p * t + 0.5;
    p = p * t + 1.0;
    p = p * t + 1.0;
    const uint64_t sb = (uint64_t) (n + 1023) << 52;
    double scale;
    __builtin_memcpy(&scale, &sb, 8);
    return p * scale;
}

/* the exposure of a frame that is not metered (amvpt_tonemap.h "The exposure used"); host only in effect */
TM_HD float tm_manual_exposure(const amvpt_tonemap_params &q) {
    return (float) ((double) q.key / 0.18 * exp2_pm((double) q.ev));
}

/* the exposure step (amvpt_tonemap.h "Exposure"): hist is the 512 counts of this frame; counted, frames, exposure and
 * log2_exposure of *s are updated.  Serial, in bin order. */
TM_HD void tm_exposure(const uint32_t *hist, const amvpt_tonemap_params &q, amvpt_tonemap_state *s) {
    uint64_t N = 0;
    for (uint32_t b = 0; b < kTmBins; ++b) N += hist[b];
    s->counted = (uint32_t) N;
    if (N == 0) {
        if (s->frames == 0) {   /* a fresh state and nothing to meter: the manual exposure without the 0.18 */
            s->log2_exposure = (double) q.ev;
            s->exposure = (float) ((double) q.key * exp2_pm((double) q.ev));
        }
        return;
    }
    const uint64_t n_lo = (uint64_t) ((double) q.lo * (double) N);   /* floor: the product is not negative */
    uint64_t n_hi = (uint64_t) ((double) q.hi * (double) N);
    /* lo < 1 in float32 and N < 2^32 give n_lo < N, so the window holds a sample and M below is at least 1 */
    if (n_hi <= n_lo) n_hi = n_lo + 1;
    if (n_hi > N) n_hi = N;
    uint64_t S = 0, M = 0, cum = 0;
    for (uint32_t b = 0; b < kTmBins; ++b) {
        const uint64_t end = cum + hist[b];
        const uint64_t a = cum > n_lo ? cum : n_lo, z = end < n_hi ? end : n_hi;
        const uint64_t ov = z > a ? z - a : 0;
        S += ov * b, M += ov;
        cum = end;
    }
    const double mean = -16.0 + ((double) S / (double) M + 0.5) / 16.0;
    double target = (double) q.ev - mean;
    target = target > (double) q.min_ev ? (target < (double) q.max_ev ? target : (double) q.max_ev) : (double) q.min_ev;
    double l = s->log2_exposure + (target - s->log2_exposure) * (double) q.adapt;
    if (s->frames == 0) l = target;
    s->log2_exposure = l;
    s->exposure = (float) ((double) q.key * exp2_pm(l));
    s->frames += 1;
}

/* Narkowicz's fit of the ACES curve, one channel */
TM_HD float tm_aces(float x) {
    if (x != x) return x;
    if (!(x > 0.f)) return 0.f;
    if (x > 0x1p60f) return 2.51f / 2.43f;   /* the limit; above it x * x leaves float32 */
    return (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f);
}

/* what the kernels and the host loops hand to every pixel */
struct TonemapOp {
    uint32_t op;
    float white2;   /* white * white */
};

/* one pixel: the three colour channels c scaled by the exposure and mapped by the operator -> y */
TM_HD void tm_pixel(const float *c, float exposure, const TonemapOp &O, float y[3]) {
    const float x[3] = {c[0] * exposure, c[1] * exposure, c[2] * exposure};
    if (O.op == AMVPT_TONEMAP_ACES) {
        y[0] = tm_aces(x[0]), y[1] = tm_aces(x[1]), y[2] = tm_aces(x[2]);
        return;
    }
    if (O.op == AMVPT_TONEMAP_REINHARD) {
        const float L = pp_lum(x);
        if (pp_finite(L) && L > 0.f) {
            const float s = (1.f + L / O.white2) / (1.f + L);
            y[0] = x[0] * s, y[1] = x[1] * s, y[2] = x[2] * s;
            return;
        }
    }
    y[0] = x[0], y[1] = x[1], y[2] = x[2];
}

#undef TM_HD

} // namespace amvpt

/*
 * dfixed.h -- per-element code of the fixed-point film's accumulate and resolve (include/amvpt_fixed.h), shared
 * by the device kernels (amvpt_render.hip) and the host entry points (amvpt_fixed_host.cpp).
 */
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FXHD __host__ __device__ __forceinline__
#else
#define FXHD inline
#endif

namespace amvpt {

/* a 32.32 sum as the film's float: exact int64 -> double up to 2^53 (round to nearest even above), an exact
 * scaling by 2^-32, one rounding to float */
FXHD float fixed_to_float(int64_t q) { return (float) ((double) q * (1.0 / 4294967296.0)); }
FXHD float fixed_resolve_value(int64_t q, float film, int add) { return add ? film + fixed_to_float(q) : fixed_to_float(q); }
/* two's complement add: wraps, never signed overflow */
FXHD int64_t fixed_sum(int64_t a, int64_t b) { return (int64_t) ((uint64_t) a + (uint64_t) b); }
/* quilt element of window element i of window row y */
FXHD uint64_t fixed_window_index(uint32_t qw, uint32_t C, uint32_t x0, uint32_t y0, uint32_t y, uint32_t i) {
    return ((uint64_t) (y0 + y) * qw + x0) * C + i;
}

/* the argument checks of amvpt_fixed_accumulate / _host: null on success, else the message */
inline const char *fixed_accumulate_check(const void *quilt, uint32_t qw, uint32_t qh, uint32_t C, const void *win,
                                          uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, const void *ov, uint64_t n_ov) {
    if (!quilt) return "amvpt_fixed_accumulate: quilt is null";
    if (w && h && !win) return "amvpt_fixed_accumulate: window is null";
    if (n_ov && !ov) return "amvpt_fixed_accumulate: overflow_entries is null";
    if (C != 4 && C != 5) return "amvpt_fixed_accumulate: channels must be 4 or 5";
    if ((uint64_t) x0 + w > qw || (uint64_t) y0 + h > qh) return "amvpt_fixed_accumulate: window outside the quilt";
    return nullptr;
}

} // namespace amvpt

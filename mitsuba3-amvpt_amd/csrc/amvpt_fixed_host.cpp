/*
 * amvpt_fixed_host.cpp -- the host entry points of include/amvpt_fixed.h: plain C++ over host pointers, from the
 * per-element code the device kernels use (dfixed.h).  No HIP call: they work without a device.
 */
#include <string>

#include "../../include/amvpt_fixed.h"
#include "dfixed.h"

namespace amvpt {
void set_error(const std::string &msg);
}

extern "C" {

uint32_t amvpt_fixed_version(void) { return AMVPT_FIXED_VERSION; }

amvpt_status amvpt_fixed_accumulate_host(int64_t *quilt, uint32_t qw, uint32_t qh, uint32_t C, const int64_t *win,
                                         uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, const uint64_t *ov,
                                         uint64_t n_ov) {
    if (const char *bad = amvpt::fixed_accumulate_check(quilt, qw, qh, C, win, x0, y0, w, h, ov, n_ov)) {
        amvpt::set_error(bad);
        return AMVPT_ERR_INVALID;
    }
    const uint32_t row = w * C;
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t i = 0; i < row; ++i) {
            int64_t &q = quilt[amvpt::fixed_window_index(qw, C, x0, y0, y, i)];
            q = amvpt::fixed_sum(q, win[(uint64_t) y * row + i]);
        }
    const uint64_t n = (uint64_t) qw * qh * C;
    for (uint64_t e = 0; e < n_ov; ++e) {
        const uint64_t idx = ov[2 * e];
        if (idx < n) quilt[idx] = amvpt::fixed_sum(quilt[idx], (int64_t) ov[2 * e + 1]);
    }
    return AMVPT_OK;
}

amvpt_status amvpt_fixed_resolve_host(const int64_t *fixed, float *film, uint64_t n, int add) {
    if (n && !fixed) { amvpt::set_error("amvpt_fixed_resolve: fixed is null"); return AMVPT_ERR_INVALID; }
    if (n && !film) { amvpt::set_error("amvpt_fixed_resolve: film is null"); return AMVPT_ERR_INVALID; }
    for (uint64_t i = 0; i < n; ++i) film[i] = amvpt::fixed_resolve_value(fixed[i], film[i], add);
    return AMVPT_OK;
}

} // extern "C"

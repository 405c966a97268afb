/*
 * post_host.h -- the host side the post-process units share (amvpt_display.hip, amvpt_guides.hip, amvpt_denoise.hip,
 * amvpt_temporal.hip, amvpt_variance.hip, amvpt_synth.hip, amvpt_tonemap.hip): the device test, and the refusals that are the same from
 * entry to entry, each worded once (post_host.cpp).  A unit keeps its own null tests and parameter ranges and calls
 * these between them; the order decides which of two faults a call hears of.  The upload of a view table is viewbuf.h's,
 * beside the pool it draws on.
 */
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <string>

#include "../../include/amvpt.h"

namespace amvpt {

struct TemporalLayout;   /* dtemporal.h */

/* a visible device is remembered (it does not go away); its absence is asked again on the next call */
bool device_ok();

bool overlap(const void *a, size_t na, const void *b, size_t nb);

/* where iteration i of n writes: the two buffers of a pair take turns so that the last iteration lands in `out` */
inline float *pingpong_dst(uint32_t i, uint32_t n, float *out, float *scratch) { return ((n - 1u - i) & 1u) ? scratch : out; }

/* the refusals of the entry `who`: every message starts "who: " */
struct Refusal {
    std::string who, prefix;
    explicit Refusal(const std::string &w) : who(w), prefix(w + ": ") {}
    amvpt_status bad(const std::string &what) const;           /* AMVPT_ERR_INVALID */
    amvpt_status unsupported(const std::string &what) const;   /* AMVPT_ERR_UNSUPPORTED */
    amvpt_status need_device() const;                          /* AMVPT_ERR_NO_DEVICE unless device_ok() */
};

amvpt_status check_channels(const Refusal &R, uint32_t channels);   /* 3 or 4 */
/* neither side 0 */
amvpt_status check_size(const Refusal &R, uint32_t w, uint32_t h);
/* check_size, and what a kernel over the image asks: pixel coordinates are ints, a tap reaches 2 * 128 pixels, and one
 * launch of 32 x 8 tiles covers the image */
amvpt_status check_size_tiles(const Refusal &R, uint32_t w, uint32_t h);
/* the launch geometry of w x h pixels: tx * ty tiles of 32 x 8 pixels */
void tile_grid(uint32_t w, uint32_t h, uint64_t &tx, uint64_t &ty);
/* tile_grid, refused at 2^31 tiles or more; `what` is what the message calls the pixels */
amvpt_status check_tiles(const Refusal &R, const char *what, uint32_t w, uint32_t h, uint64_t &tx, uint64_t &ty);

/* the layout of the quilt of *p (amvpt_temporal.h "Layout") and its refusals, `name` being the argument's; the
 * rectangle is the whole film */
amvpt_status check_layout(const Refusal &R, const char *name, const amvpt_params *p, TemporalLayout &L);
/* rect (null: the whole film) becomes L's rectangle: inside the film of check_layout and made of whole tiles */
amvpt_status check_rect(const Refusal &R, const uint32_t *rect, TemporalLayout &L);

/* a buffer of an entry under the name its refusals use; p may be null */
struct Span {
    const void *p;
    size_t bytes;
    const char *name;
};
/* no output overlaps an input or an earlier output: "A overlaps B" with A an output, and the later one of two */
amvpt_status check_disjoint(const Refusal &R, std::initializer_list<Span> outs, std::initializer_list<Span> ins);

} // namespace amvpt

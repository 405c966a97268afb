/*
 * amvpt_fixed.h -- the 32.32 fixed-point film of libamvpt_hip.so as a caller-owned object: renders accumulate
 * into it, partial films are summed as integers, and one resolve converts the sum to float.
 *
 * Integer sums are associative, so any partition of a frame -- ranks, film windows, lane ranges, chunk sizes,
 * streams, repeated calls -- sums to the same integers, and one amvpt_fixed_resolve of the sum gives the film of
 * amvpt_render_ex(AMVPT_OPT_DETERMINISTIC) of the whole frame bit for bit ("The fixed-point film").
 *
 * These are new entry points only: no struct of amvpt.h changes, AMVPT_ABI_VERSION stays as it is and this
 * header carries a version of its own.  Status codes and amvpt_last_error() are amvpt.h's.
 */
#ifndef AMVPT_FIXED_H
#define AMVPT_FIXED_H

#include "amvpt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AMVPT_FIXED_VERSION 1

/* amvpt_render_opts.flags: every put goes straight to the fixed-point film with global integer atomics instead of
 * through the integer LDS window (same integers; A/B runs and tests).  Also honoured under AMVPT_OPT_DETERMINISTIC. */
#define AMVPT_OPT_FIXED_DIRECT 1024u

/*
 * amvpt_film_window in integers.  `film` holds quilt pixels [x0, x0 + width) x [y0, y0 + height), height x width x
 * channels values of 32.32 two's complement (device memory).  Quilt cells outside it are appended to `overflow`
 * (device): a 16-byte header whose first u64 is the entry count, then 16-byte entries {u64 quilt float index,
 * i64 value}.  The list keeps the float list's rules: zero the header before the first render into it, renders
 * append, the count keeps counting past overflow_capacity and such a render fails with AMVPT_ERR_OOM.  A window
 * smaller than the quilt needs a list.
 */
typedef struct amvpt_fixed_window {
    int64_t *film;
    uint32_t x0, y0, width, height;
    uint64_t *overflow;
    uint64_t overflow_capacity;
} amvpt_fixed_window;

uint32_t amvpt_fixed_version(void);

/*
 * amvpt_render_ex into a fixed-point window.  Every footprint-cell add v goes into the window as
 * rint((double) v * 2^32); non-finite adds are dropped, finite adds of |v| >= 2^31 are dropped and counted in
 * counters->film_range_drops.  The window is accumulated into: it is neither cleared nor resolved, and no private
 * fixed-point film is reserved.  Any window is accepted; counters->film_overflow counts this render's list
 * entries.  Lane sets, adaptive renders (opts->exchange), records and debug mode behave as in amvpt_render_ex.
 */
amvpt_status amvpt_render_fixed(amvpt_scene *scene, const amvpt_view_desc *views, const amvpt_params *params,
                                const amvpt_lane_set *lanes, const amvpt_fixed_window *film, void *stream,
                                const amvpt_render_opts *opts, amvpt_counters *counters);

/*
 * quilt (quilt_height x quilt_width x channels, int64) += a window's rows, then += the overflow entries (the
 * 16-byte entries after a list's header; indices may repeat, an index past the quilt is ignored).  Two's
 * complement sums: wrap-around is the same however the adds are grouped.  Device pointers, ordered on `stream`.
 * AMVPT_ERR_INVALID, naming the argument: a null quilt, a null window with width and height set, null entries
 * with n_entries set, a window past the quilt, channels not 4 or 5.
 */
amvpt_status amvpt_fixed_accumulate(int64_t *quilt_device, uint32_t quilt_width, uint32_t quilt_height,
                                    uint32_t channels, const int64_t *window_device, uint32_t x0, uint32_t y0,
                                    uint32_t width, uint32_t height, const uint64_t *overflow_entries_device,
                                    uint64_t n_entries, void *stream);

/* film[i] = (add ? film[i] : 0) + (float) ((double) fixed[i] * 2^-32) for i < n_floats.  Device pointers. */
amvpt_status amvpt_fixed_resolve(const int64_t *fixed_device, float *film_device, uint64_t n_floats, int add,
                                 void *stream);

/* The same functions over host pointers, compiled for the host from the same per-element code: they need no
 * device and never return AMVPT_ERR_NO_DEVICE. */
amvpt_status amvpt_fixed_accumulate_host(int64_t *quilt, uint32_t quilt_width, uint32_t quilt_height,
                                         uint32_t channels, const int64_t *window, uint32_t x0, uint32_t y0,
                                         uint32_t width, uint32_t height, const uint64_t *overflow_entries,
                                         uint64_t n_entries);
amvpt_status amvpt_fixed_resolve_host(const int64_t *fixed, float *film, uint64_t n_floats, int add);

#ifdef __cplusplus
}
#endif

#endif /* AMVPT_FIXED_H */

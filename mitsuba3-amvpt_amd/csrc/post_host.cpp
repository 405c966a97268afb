/*
 * post_host.cpp -- the definitions of post_host.h: the one device test and the shared refusals of the post-process
 * entries.  The messages are part of the interface (tests/ pins each by its prefix and its words); change none in passing.
 */
#include <hip/hip_runtime.h>

#include <atomic>

#include "dtemporal.h"
#include "dtile.h"
#include "internal.h"
#include "post_host.h"

namespace amvpt {

bool device_ok() {
    static std::atomic<bool> seen{false};
    if (seen.load(std::memory_order_relaxed)) return true;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return false;
    seen.store(true, std::memory_order_relaxed);
    return true;
}

bool overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t a0 = (uintptr_t) a, b0 = (uintptr_t) b;
    return a0 < b0 + nb && b0 < a0 + na;
}

amvpt_status Refusal::bad(const std::string &what) const { set_error(prefix + what); return AMVPT_ERR_INVALID; }
amvpt_status Refusal::unsupported(const std::string &what) const { set_error(prefix + what); return AMVPT_ERR_UNSUPPORTED; }
amvpt_status Refusal::need_device() const {
    if (device_ok()) return AMVPT_OK;
    set_error(prefix + "no HIP device visible");
    return AMVPT_ERR_NO_DEVICE;
}

amvpt_status check_channels(const Refusal &R, uint32_t channels) {
    if (channels != 3u && channels != 4u) return R.bad("channels must be 3 or 4, not " + std::to_string(channels));
    return AMVPT_OK;
}

amvpt_status check_size(const Refusal &R, uint32_t w, uint32_t h) {
    if (w == 0) return R.bad("width is 0");
    if (h == 0) return R.bad("height is 0");
    return AMVPT_OK;
}

void tile_grid(uint32_t w, uint32_t h, uint64_t &tx, uint64_t &ty) {
    tx = (w + (uint32_t) kTileW - 1u) / (uint32_t) kTileW, ty = (h + (uint32_t) kTileH - 1u) / (uint32_t) kTileH;
}

amvpt_status check_tiles(const Refusal &R, const char *what, uint32_t w, uint32_t h, uint64_t &tx, uint64_t &ty) {
    tile_grid(w, h, tx, ty);
    if (tx * ty >= (1ull << 31)) return R.bad(std::string(what) + " above 2^31 tiles of 32 x 8 pixels");
    return AMVPT_OK;
}

amvpt_status check_size_tiles(const Refusal &R, uint32_t w, uint32_t h) {
    if (amvpt_status st = check_size(R, w, h)) return st;
    if (w > 0x7fffff00u || h > 0x7fffff00u) return R.bad("width or height above 2^31 - 256");
    uint64_t tx, ty;
    return check_tiles(R, "width x height", w, h, tx, ty);
}

amvpt_status check_layout(const Refusal &R, const char *name, const amvpt_params *p, TemporalLayout &L) {
    const Refusal N(R.prefix + name);
    if (p->film_width == 0) return N.bad("film_width is 0");
    if (p->film_height == 0) return N.bad("film_height is 0");
    /* pixel coordinates are formed as floats */
    if (p->film_width > (1u << 24) || p->film_height > (1u << 24)) return N.bad("film_width or film_height above 2^24");
    if (p->crop_offset_x || p->crop_offset_y) return N.unsupported("a crop window (crop_offset) is not supported");
    if ((p->full_width && p->full_width != p->film_width) || (p->full_height && p->full_height != p->film_height))
        return N.unsupported("a crop window (full_width / full_height differ from the film) is not supported");
    L.multisensor = p->multisensor ? 1u : 0u;
    L.batch = p->batch ? 1u : 0u;
    L.n_views = p->n_views, L.gx = p->grid_x, L.gy = p->grid_y;
    L.rev_x = p->reverse_x ? 1u : 0u, L.rev_y = p->reverse_y ? 1u : 0u;
    uint32_t tw = p->film_width, th = p->film_height;
    if (L.multisensor) {
        if (p->n_views == 0) return N.bad("n_views is 0");
        if (L.batch) {
            if (p->film_width % p->n_views) return N.unsupported("film_width is not a multiple of n_views");
            tw = p->film_width / p->n_views;
        } else {
            if (p->grid_x == 0 || p->grid_y == 0) return N.bad("grid_x or grid_y is 0");
            if ((uint64_t) p->grid_x * p->grid_y != p->n_views) return N.unsupported("n_views is not grid_x * grid_y");
            if (p->film_width % p->grid_x || p->film_height % p->grid_y)
                return N.unsupported("the film size is not a multiple of the grid");
            tw = p->film_width / p->grid_x, th = p->film_height / p->grid_y;
        }
    }
    L.tw = (int32_t) tw, L.th = (int32_t) th;
    L.rx0 = 0, L.ry0 = 0, L.rw = (int32_t) p->film_width, L.rh = (int32_t) p->film_height;
    return AMVPT_OK;
}

amvpt_status check_rect(const Refusal &R, const uint32_t *rect, TemporalLayout &L) {
    if (!rect) return AMVPT_OK;
    const uint32_t fw = (uint32_t) L.rw, fh = (uint32_t) L.rh, tw = (uint32_t) L.tw, th = (uint32_t) L.th;
    if (rect[2] == 0 || rect[3] == 0) return R.bad("rect: zero area");
    if (rect[0] >= fw || rect[2] > fw - rect[0] || rect[1] >= fh || rect[3] > fh - rect[1]) return R.bad("rect: outside the film");
    if (rect[0] % tw || rect[2] % tw || rect[1] % th || rect[3] % th) return R.bad("rect: not made of whole tiles");
    L.rx0 = (int32_t) rect[0], L.ry0 = (int32_t) rect[1], L.rw = (int32_t) rect[2], L.rh = (int32_t) rect[3];
    return AMVPT_OK;
}

amvpt_status check_disjoint(const Refusal &R, std::initializer_list<Span> outs, std::initializer_list<Span> ins) {
    for (const Span *o = outs.begin(); o != outs.end(); ++o) {
        if (!o->p) continue;
        for (const Span &i : ins)
            if (i.p && overlap(o->p, o->bytes, i.p, i.bytes)) return R.bad(std::string(o->name) + " overlaps " + i.name);
        for (const Span *e = outs.begin(); e != o; ++e)
            if (e->p && overlap(o->p, o->bytes, e->p, e->bytes)) return R.bad(std::string(o->name) + " overlaps " + e->name);
    }
    return AMVPT_OK;
}

} // namespace amvpt

/*
 * amvpt_capi.cpp -- C-ABI of libamvpt_hip.so (include/amvpt.h).
 *
 * Scene creation uploads the host image that scene_image.cpp builds from the descriptor (BVH, BVH-ordered
 * primitives, the small read-only tables), once.  The product path has no CPU fallback: without a GPU every
 * render entry point returns AMVPT_ERR_NO_DEVICE.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "scene_image.h"

namespace amvpt {

static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }
amvpt_status hip_fail(const char *what, int err) {
    g_err = std::string(what) + ": " + hipGetErrorString((hipError_t) err);
    return err == (int) hipErrorOutOfMemory ? AMVPT_ERR_OOM : AMVPT_ERR_HIP;
}

/* SAH shape of the scene build (amvpt_set_bvh_build; scene_image.cpp Builder) */
static uint32_t g_bvh_max_leaf = 4;
static float g_bvh_trav_cost = 0.f;

/* one upload of amvpt_scene_create: the host bytes and the DScene pointer member they fill */
struct Upload { const void *src; size_t bytes; void *slot; };
template <class T> static Upload row(const std::vector<T> &v, const T *&slot) { return {v.data(), v.size() * sizeof(T), &slot}; }

static bool device_ok() {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess && n > 0;
}

} // namespace amvpt

using namespace amvpt;

extern "C" {

const char *amvpt_last_error(void) { return g_err.c_str(); }
uint32_t amvpt_abi_version(void) { return AMVPT_ABI_VERSION; }

amvpt_status amvpt_device_count(int *count) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    if (count) *count = n;
    return AMVPT_OK;
}

amvpt_status amvpt_set_device(int device) {
    if (!device_ok()) { set_error("no HIP device visible"); return AMVPT_ERR_NO_DEVICE; }
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return hip_fail("hipSetDevice", (int) e);
    return AMVPT_OK;
}

uint32_t amvpt_film_channels(const amvpt_params *p) { return p && p->film_alpha ? 5u : 4u; }

amvpt_status amvpt_rfilter_eval(const amvpt_params *params, const float *x, uint32_t n, float *out, float *radius) {
    return rfilter_eval_impl(params, x, n, out, radius);
}

amvpt_status amvpt_set_chunk_lanes(uint64_t chunk_lanes) {
    g_chunk_lanes = chunk_lanes ? std::max<uint64_t>(256, chunk_lanes) : 0;   /* 0: automatic */
    return AMVPT_OK;
}

amvpt_status amvpt_set_traversal(uint32_t mode) {
    if (mode > 2) { set_error("amvpt_set_traversal: mode must be 0 (auto), 1 (wave-uniform) or 2 (per-lane)"); return AMVPT_ERR_INVALID; }
    g_traversal = mode;
    return AMVPT_OK;
}

amvpt_status amvpt_set_bvh_build(uint32_t max_leaf_prims, float traversal_cost) {
    if (max_leaf_prims < 1 || max_leaf_prims > kMaxLeafPrims || !(traversal_cost >= 0.f)) {
        set_error("amvpt_set_bvh_build: max_leaf_prims in [1, 15], traversal_cost >= 0");
        return AMVPT_ERR_INVALID;
    }
    g_bvh_max_leaf = max_leaf_prims;
    g_bvh_trav_cost = traversal_cost;
    return AMVPT_OK;
}

amvpt_status amvpt_set_adaptive_exchange(amvpt_exchange_fn fn, void *ctx) {
    g_exchange = fn;
    g_exchange_ctx = fn ? ctx : nullptr;
    return AMVPT_OK;
}

amvpt_status amvpt_plan(const amvpt_params *P, uint32_t *spp, uint32_t *spp_pp, uint32_t *n_passes,
                        uint64_t *lanes) {
    if (!P) { set_error("amvpt_plan: null params"); return AMVPT_ERR_INVALID; }
    uint32_t s = P->spp ? P->spp : 1, spl;
    uint32_t np;
    if (P->integrator == AMVPT_INTEGRATOR_MVPATH) {
        spl = P->spp_pass_lim ? std::min(P->spp_pass_lim, s) : s;
        np = s / spl;
        s = np * spl;
    } else {
        spl = s;
        np = 1;
    }
    uint64_t wf = (uint64_t) P->film_width * P->film_height * spl;
    if (wf > 0xffffffffull) {
        spl /= (uint32_t) ((wf + 0xffffffffull - 1) / 0xffffffffull);
        np = s / spl;
        wf = (uint64_t) P->film_width * P->film_height * spl;
    }
    if (spp) *spp = s;
    if (spp_pp) *spp_pp = spl;
    if (n_passes) *n_passes = np;
    if (lanes) *lanes = wf;
    return AMVPT_OK;
}

amvpt_status amvpt_scene_create(const amvpt_scene_desc *d, amvpt_scene **out) {
    if (!d || !out) { set_error("amvpt_scene_create: null argument"); return AMVPT_ERR_INVALID; }
    *out = nullptr;
    /* the whole descriptor is validated first, also without a device (scene_image.h) */
    amvpt_status st = validate_scene(d);
    if (st != AMVPT_OK) return st;
    if (!device_ok()) { set_error("amvpt_scene_create: no HIP device visible (the product path has no CPU fallback)"); return AMVPT_ERR_NO_DEVICE; }
    SceneImage img;
    if ((st = build_scene_image(d, g_bvh_max_leaf, g_bvh_trav_cost, img)) != AMVPT_OK) return st;

    amvpt_scene *sc = new amvpt_scene();
    static_cast<SceneFacts &>(*sc) = img.facts;
    (void) hipGetDevice(&sc->device);
    auto upload = [&](const void *src, size_t bytes, void **dst) -> amvpt_status {
        hipError_t e = hipMalloc(dst, bytes);
        if (e != hipSuccess) return hip_fail("hipMalloc(scene)", (int) e);
        sc->allocations.push_back(*dst);
        e = hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) return hip_fail("hipMemcpy(scene)", (int) e);
        return AMVPT_OK;
    };
    DScene &D = sc->dev = img.dev;
    const Upload table[] = {
        row(img.nodes, D.nodes), row(img.prims, D.prims), row(img.shapes, D.shapes), row(img.bsdfs, D.bsdfs),
        row(img.emitters, D.emitters), row(img.vpos, D.vpos), row(img.vnrm, D.vnrm), row(img.vuv, D.vuv),
        row(img.faces, D.faces), row(img.face_area, D.face_area), row(img.sph_prims, D.sph_prims),
        row(img.boxes, D.boxes), row(img.box_prims, D.box_prims), row(img.loose_prims, D.loose_prims),
        row(img.outer, D.outer), row(img.nodes2, D.nodes2), row(img.nodes2h, D.nodes2h), row(img.hrec, D.hrec)};
    for (const Upload &u : table) {
        void *p = nullptr;
        if ((st = upload(u.src, u.bytes, &p)) != AMVPT_OK) break;
        std::memcpy(u.slot, &p, sizeof(p));
    }
    /* the device copy of `dev`, now that its pointers are set */
    if (st == AMVPT_OK) st = upload(&D, sizeof(DScene), &sc->dev_scene_struct);
    if (st != AMVPT_OK) { amvpt_scene_destroy(sc); return st; }
    *out = sc;
    return AMVPT_OK;
}

amvpt_status amvpt_scene_desc_boxes(const amvpt_scene_desc *d, uint32_t *n_boxes) {
    if (!d || !n_boxes) { set_error("amvpt_scene_desc_boxes: null argument"); return AMVPT_ERR_INVALID; }
    const amvpt_status vs = validate_scene(d);
    if (vs != AMVPT_OK) return vs;
    *n_boxes = count_boxes(d);
    return AMVPT_OK;
}

amvpt_status amvpt_scene_destroy(amvpt_scene *scene) {
    if (!scene) return AMVPT_OK;
    for (void *p : scene->allocations) (void) hipFree(p);
    delete scene;
    return AMVPT_OK;
}

amvpt_status amvpt_scene_bvh2(const amvpt_scene *scene, uint32_t *n_nodes2, uint32_t *depth) {
    if (!scene || !n_nodes2 || !depth) { set_error("amvpt_scene_bvh2: null argument"); return AMVPT_ERR_INVALID; }
    *n_nodes2 = scene->n_nodes2;
    *depth = scene->bvh2_depth;
    return AMVPT_OK;
}

amvpt_status amvpt_scene_stats(const amvpt_scene *scene, uint32_t *n_nodes, uint32_t *n_prims) {
    if (!scene) { set_error("null scene"); return AMVPT_ERR_INVALID; }
    if (n_nodes) *n_nodes = scene->n_nodes;
    if (n_prims) *n_prims = scene->n_prims;
    return AMVPT_OK;
}

} // extern "C"

namespace {
/* amvpt_set_adaptive_exchange's one-count exchange as a run exchange: a contiguous lane set is
 * one run (or none, for an empty range) */
struct LegacyExchange { amvpt_exchange_fn fn; void *ctx; };
int legacy_run_exchange(void *ctx, uint32_t n_runs, const uint64_t *, const uint64_t *run_count, uint64_t *run_prefix,
                        uint64_t *total) {
    const LegacyExchange *x = static_cast<const LegacyExchange *>(ctx);
    if (n_runs > 1) return 1;
    uint64_t prefix = 0;
    const int rc = x->fn(x->ctx, n_runs ? run_count[0] : 0, &prefix, total);
    if (n_runs) run_prefix[0] = prefix;
    return rc;
}
/* amvpt_render / amvpt_render_records: contiguous lanes, whole-quilt film, process-global knobs */
amvpt_status render_legacy(amvpt_scene *scene, const amvpt_view_desc *views, const amvpt_params *params,
                           uint64_t lane_begin, uint64_t lane_end, float *film, void *stream, amvpt_counters *counters,
                           float *records, uint32_t pass) {
    if (!params) { set_error("amvpt_render: null argument"); return AMVPT_ERR_INVALID; }
    amvpt_lane_set lanes{};
    lanes.lane_begin = lane_begin;
    lanes.lane_end = lane_end;
    amvpt_film_window w{};
    w.film = film;
    w.width = params->film_width;
    w.height = params->film_height;
    LegacyExchange lx{g_exchange, g_exchange_ctx};
    amvpt_render_opts o{};
    o.chunk_lanes = g_chunk_lanes;
    o.traversal = g_traversal;
    if (g_exchange) { o.exchange = legacy_run_exchange; o.exchange_ctx = &lx; }
    return render_impl(scene, views, params, lanes, w, stream, o, counters, records, pass);
}
} // namespace

extern "C" {

amvpt_status amvpt_render(amvpt_scene *scene, const amvpt_view_desc *views, const amvpt_params *params,
                          uint64_t lane_begin, uint64_t lane_end, float *film_device, void *stream,
                          amvpt_counters *counters) {
    if (!device_ok()) { set_error("amvpt_render: no HIP device visible"); return AMVPT_ERR_NO_DEVICE; }
    return render_legacy(scene, views, params, lane_begin, lane_end, film_device, stream, counters, nullptr, 0);
}

amvpt_status amvpt_render_records(amvpt_scene *scene, const amvpt_view_desc *views, const amvpt_params *params,
                                  uint32_t pass, uint64_t lane_begin, uint64_t lane_end, float *film_device,
                                  float *records_device, void *stream) {
    if (!device_ok()) { set_error("amvpt_render_records: no HIP device visible"); return AMVPT_ERR_NO_DEVICE; }
    return render_legacy(scene, views, params, lane_begin, lane_end, film_device, stream, nullptr, records_device, pass);
}

amvpt_status amvpt_render_ex(amvpt_scene *scene, const amvpt_view_desc *views, const amvpt_params *params,
                             const amvpt_lane_set *lanes, const amvpt_film_window *film, void *stream,
                             const amvpt_render_opts *opts, amvpt_counters *counters) {
    if (!lanes || !film) { set_error("amvpt_render_ex: null lane set or film window"); return AMVPT_ERR_INVALID; }
    if (!device_ok()) { set_error("amvpt_render_ex: no HIP device visible"); return AMVPT_ERR_NO_DEVICE; }
    const amvpt_render_opts defaults{};
    const amvpt_render_opts &o = opts ? *opts : defaults;
    return render_impl(scene, views, params, *lanes, *film, stream, o, counters, o.records, o.record_pass);
}

amvpt_status amvpt_render_fixed(amvpt_scene *scene, const amvpt_view_desc *views, const amvpt_params *params,
                                const amvpt_lane_set *lanes, const amvpt_fixed_window *film, void *stream,
                                const amvpt_render_opts *opts, amvpt_counters *counters) {
    if (!lanes || !film) { set_error("amvpt_render_fixed: null lane set or fixed window"); return AMVPT_ERR_INVALID; }
    if (!device_ok()) { set_error("amvpt_render_fixed: no HIP device visible"); return AMVPT_ERR_NO_DEVICE; }
    const amvpt_render_opts defaults{};
    const amvpt_render_opts &o = opts ? *opts : defaults;
    /* the integer window and list travel in a film window's fields (render_impl's fixed_film) */
    amvpt_film_window w{};
    w.film = reinterpret_cast<float *>(film->film);
    w.x0 = film->x0; w.y0 = film->y0; w.width = film->width; w.height = film->height;
    w.overflow = reinterpret_cast<uint32_t *>(film->overflow);
    w.overflow_capacity = film->overflow_capacity;
    return render_impl(scene, views, params, *lanes, w, stream, o, counters, o.records, o.record_pass, true);
}

amvpt_status amvpt_fixed_accumulate(int64_t *quilt, uint32_t quilt_width, uint32_t quilt_height, uint32_t channels,
                                    const int64_t *window, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height,
                                    const uint64_t *overflow_entries, uint64_t n_entries, void *stream) {
    if (!device_ok()) { set_error("amvpt_fixed_accumulate: no HIP device visible"); return AMVPT_ERR_NO_DEVICE; }
    return fixed_accumulate_impl(quilt, quilt_width, quilt_height, channels, window, x0, y0, width, height,
                                 overflow_entries, n_entries, stream);
}

amvpt_status amvpt_fixed_resolve(const int64_t *fixed, float *film, uint64_t n_floats, int add, void *stream) {
    if (!device_ok()) { set_error("amvpt_fixed_resolve: no HIP device visible"); return AMVPT_ERR_NO_DEVICE; }
    return fixed_resolve_impl(fixed, film, n_floats, add, stream);
}

amvpt_status amvpt_film_accumulate(float *quilt, uint32_t quilt_width, uint32_t quilt_height, uint32_t channels,
                                   const float *window, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height,
                                   const uint32_t *overflow_entries, uint64_t n_entries, void *stream) {
    if (!device_ok()) { set_error("amvpt_film_accumulate: no HIP device visible"); return AMVPT_ERR_NO_DEVICE; }
    return accumulate_impl(quilt, quilt_width, quilt_height, channels, window, x0, y0, width, height, overflow_entries,
                           n_entries, stream);
}

amvpt_status amvpt_develop(const float *film_device, float *out_device, uint32_t width, uint32_t height,
                           uint32_t film_alpha, void *stream) {
    if (!device_ok()) { set_error("amvpt_develop: no HIP device visible"); return AMVPT_ERR_NO_DEVICE; }
    return develop_impl(film_device, out_device, width, height, film_alpha, stream);
}

amvpt_status amvpt_release_device_memory(int device) {
    if (!device_ok()) { set_error("amvpt_release_device_memory: no HIP device visible"); return AMVPT_ERR_NO_DEVICE; }
    return release_impl(device);
}

} // extern "C"

"""
amvpt -- Python front end of the MI355X-native AMVPT (`mvpath`) integrator.

A thin ctypes layer over the two in-tree native libraries:

* ``lib/libamvpt_hip.so``  -- the drop-in C-ABI of the hot path (include/amvpt.h),
  hand-written HIP kernels for gfx950;
* ``lib/libamvpt_host.so`` -- the Mitsuba-style host framework (XML scene subset,
  Properties, plugins, ``Integrator::render``) built on that C-ABI.

The surface mirrors the reference's Python API for the path
(``mi.load_file``, ``mi.load_string``, ``mi.render``, ``Bitmap.write``;
reference: src/python/python/__init__.py / src/render/python).  There is no
CPU fallback: rendering without a visible GPU raises ``RuntimeError``.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# AMVPT_LIB_DIR selects a variant build (Makefile LIB=...) for A/B measurements.
LIB_DIR = os.environ.get("AMVPT_LIB_DIR") or os.path.join(os.path.dirname(_HERE), "lib")
HIP_LIB_PATH = os.path.join(LIB_DIR, "libamvpt_hip.so")
HOST_LIB_PATH = os.path.join(LIB_DIR, "libamvpt_host.so")

u32, i32, u64, f32, f64 = ctypes.c_uint32, ctypes.c_int32, ctypes.c_uint64, ctypes.c_float, ctypes.c_double


class ShapeDesc(ctypes.Structure):
    _fields_ = [("type", u32), ("bsdf", i32), ("emitter", i32), ("flip_normals", u32),
                ("to_world", f32 * 16), ("to_object", f32 * 16),
                ("vertex_count", u32), ("face_count", u32),
                ("positions", ctypes.POINTER(f32)), ("normals", ctypes.POINTER(f32)),
                ("texcoords", ctypes.POINTER(f32)), ("faces", ctypes.POINTER(u32)),
                ("center", f32 * 3), ("radius", f32)]


class BsdfDesc(ctypes.Structure):
    _fields_ = [("type", u32), ("nested", i32 * 2), ("reflectance", f32 * 3), ("distribution", u32),
                ("sample_visible", u32), ("alpha_u", f32), ("alpha_v", f32), ("eta", f32 * 3),
                ("k", f32 * 3), ("has_specular_reflectance", u32), ("specular_reflectance", f32 * 3)]


class EmitterDesc(ctypes.Structure):
    _fields_ = [("type", u32), ("shape", i32), ("radiance", f32 * 3), ("sampling_weight", f32)]


class SceneDesc(ctypes.Structure):
    _fields_ = [("shapes", ctypes.POINTER(ShapeDesc)), ("shape_count", u32),
                ("bsdfs", ctypes.POINTER(BsdfDesc)), ("bsdf_count", u32),
                ("emitters", ctypes.POINTER(EmitterDesc)), ("emitter_count", u32),
                ("has_environment", u32)]


class ViewDesc(ctypes.Structure):
    _fields_ = [("type", u32), ("to_world", f32 * 16), ("to_world_inv", f32 * 16),
                ("sample_to_camera", f32 * 16), ("camera_to_sample", f32 * 16),
                ("near_clip", f32), ("far_clip", f32), ("normalization", f32),
                ("resolution", f32 * 2), ("pp_offset", f32 * 2),
                ("aperture_radius", f32), ("focus_distance", f32)]


class Params(ctypes.Structure):
    _fields_ = [(n, u32) for n in (
        "integrator", "max_depth", "rr_depth", "hide_emitters", "sa_reuse", "sa_mis", "fast_mis",
        "debug", "adaptive", "spp_pass_lim", "reuse_count", "spp", "seed", "base_seed", "n_views",
        "multisensor", "grid_x", "grid_y", "reverse_x", "reverse_y", "film_width", "film_height",
        "film_alpha", "rfilter")] + [("rfilter_stddev", f32), ("batch", u32), ("crop_offset_x", u32),
                                      ("crop_offset_y", u32), ("full_width", u32), ("full_height", u32),
                                      # ABI 12: tent radius / Lanczos lobes (0: default), Mitchell's B and C
                                      ("rfilter_radius", f32), ("rfilter_b", f32), ("rfilter_c", f32)]


class Counters(ctypes.Structure):
    _fields_ = [("lanes", u64), ("passes", u64), ("vertices", u64), ("reuse_lanes", u64),
                ("visibility_rays", u64), ("view_splats", u64), ("adaptive_lanes", u64),
                ("kernel_ms_primary", f64), ("kernel_ms_bounce", f64), ("kernel_ms_splat", f64),
                ("total_ms", f64), ("splat_fallback", u64),
                ("shadow_rays", u64), ("kernel_ms", f64 * 12), ("kernel_launches", u64 * 12),
                ("record_bytes", u64), ("nonfinite_samples", u64), ("negative_samples", u64),
                ("pushed_paths", u64), ("film_overflow", u64), ("film_range_drops", u64),
                ("chunk_lanes", u64), ("buffer_sets", u64), ("arena_bytes", u64),
                ("primary_record_bytes", u64), ("splat_record_bytes", u64)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        for k in ("kernel_ms", "kernel_launches"):
            d[k] = {name: d[k][i] for i, name in enumerate(KERNELS)}
        return d


class LaneSet(ctypes.Structure):
    """amvpt_lane_set: contiguous lanes [lane_begin, lane_end), or (rect_width > 0) the lanes of a
    pixel rectangle of the quilt (one run of rect_width * spp_per_pass lanes per pixel row)."""
    _fields_ = [("lane_begin", u64), ("lane_end", u64), ("rect_x0", u32), ("rect_y0", u32),
                ("rect_width", u32), ("rect_height", u32)]


class FilmWindow(ctypes.Structure):
    """amvpt_film_window: device film holding quilt pixels [x0, x0+width) x [y0, y0+height), plus the
    overflow list (device; 16-B header with the u64 cell count, then 16-B entries) for cells outside."""
    _fields_ = [("film", ctypes.c_void_p), ("x0", u32), ("y0", u32), ("width", u32), ("height", u32),
                ("overflow", ctypes.c_void_p), ("overflow_capacity", u64)]


class FixedWindow(ctypes.Structure):
    """amvpt_fixed_window (include/amvpt_fixed.h): FilmWindow in integers -- a device int64 film of 32.32
    fixed-point sums, plus the overflow list (16-B header with the u64 entry count, then 16-B entries
    {u64 quilt float index, i64 value}) for cells outside."""
    _fields_ = [("film", ctypes.c_void_p), ("x0", u32), ("y0", u32), ("width", u32), ("height", u32),
                ("overflow", ctypes.c_void_p), ("overflow_capacity", u64)]


class DenoiseParams(ctypes.Structure):
    """amvpt_denoise_params (include/amvpt_denoise.h).  Without arguments: amvpt_denoise_default_params' values,
    {3, 1.0, 0.01, 0.05, 5}; sigma_plane is in world units."""
    _fields_ = [("iterations", u32), ("sigma_color", f32), ("color_floor", f32), ("sigma_plane", f32),
                ("normal_squarings", u32)]

    def __init__(self, iterations=3, sigma_color=1.0, color_floor=0.01, sigma_plane=0.05, normal_squarings=5):
        super().__init__(iterations, sigma_color, color_floor, sigma_plane, normal_squarings)

    def values(self):
        return (self.iterations, self.sigma_color, self.color_floor, self.sigma_plane, self.normal_squarings)

    def __repr__(self):
        return ("DenoiseParams(iterations=%r, sigma_color=%r, color_floor=%r, sigma_plane=%r, normal_squarings=%r)"
                % self.values())


class TemporalParams(ctypes.Structure):
    """amvpt_temporal_params (include/amvpt_temporal.h).  Without arguments: amvpt_temporal_default_params' values,
    {32, 0.02, 0.9}; plane_tol is in world units."""
    _fields_ = [("max_history", u32), ("plane_tol", f32), ("normal_cos", f32)]

    def __init__(self, max_history=32, plane_tol=0.02, normal_cos=0.9):
        super().__init__(max_history, plane_tol, normal_cos)

    def values(self):
        return (self.max_history, self.plane_tol, self.normal_cos)

    def __repr__(self):
        return "TemporalParams(max_history=%r, plane_tol=%r, normal_cos=%r)" % self.values()


class VarianceParams(ctypes.Structure):
    """amvpt_variance_params (include/amvpt_variance.h).  Without arguments: amvpt_variance_default_params' values,
    {4, 2.0, 1e-8, 0.05, 5, 4}; sigma_plane is in world units."""
    _fields_ = [("iterations", u32), ("sigma_lum", f32), ("var_floor", f32), ("sigma_plane", f32),
                ("normal_squarings", u32), ("min_history", u32)]

    def __init__(self, iterations=4, sigma_lum=2.0, var_floor=1e-8, sigma_plane=0.05, normal_squarings=5, min_history=4):
        super().__init__(iterations, sigma_lum, var_floor, sigma_plane, normal_squarings, min_history)

    def values(self):
        return (self.iterations, self.sigma_lum, self.var_floor, self.sigma_plane, self.normal_squarings, self.min_history)

    def __repr__(self):
        return ("VarianceParams(iterations=%r, sigma_lum=%r, var_floor=%r, sigma_plane=%r, normal_squarings=%r, "
                "min_history=%r)" % self.values())


class SynthParams(ctypes.Structure):
    """amvpt_synth_params (include/amvpt_synth.h).  Without arguments: amvpt_synth_default_params' values,
    {0.02, 0.9, 1e5, 4}; plane_tol is in world units."""
    _fields_ = [("plane_tol", f32), ("normal_cos", f32), ("view_falloff", f32), ("fill_iterations", u32)]

    def __init__(self, plane_tol=0.02, normal_cos=0.9, view_falloff=1e5, fill_iterations=4):
        super().__init__(plane_tol, normal_cos, view_falloff, fill_iterations)

    def values(self):
        return (self.plane_tol, self.normal_cos, self.view_falloff, self.fill_iterations)

    def __repr__(self):
        return "SynthParams(plane_tol=%r, normal_cos=%r, view_falloff=%r, fill_iterations=%r)" % self.values()


TONEMAP_LINEAR, TONEMAP_REINHARD, TONEMAP_ACES = range(3)
TONEMAP_OPS = {"linear": TONEMAP_LINEAR, "reinhard": TONEMAP_REINHARD, "aces": TONEMAP_ACES}


class TonemapParams(ctypes.Structure):
    """amvpt_tonemap_params (include/amvpt_tonemap.h).  Without arguments: amvpt_tonemap_default_params' values,
    the identity (LINEAR, no metering, ev 0, key 0.18).  `op` is a TONEMAP_* value or its lower-case name."""
    _fields_ = [("op", u32), ("auto_exposure", u32), ("ev", f32), ("key", f32), ("lo", f32), ("hi", f32), ("adapt", f32),
                ("white", f32), ("min_ev", f32), ("max_ev", f32)]

    def __init__(self, op=TONEMAP_LINEAR, auto_exposure=False, ev=0.0, key=0.18, lo=0.10, hi=0.95, adapt=1.0, white=4.0,
                 min_ev=-16.0, max_ev=16.0):
        super().__init__(TONEMAP_OPS[op] if isinstance(op, str) else op, int(auto_exposure), ev, key, lo, hi, adapt, white,
                         min_ev, max_ev)

    def values(self):
        return (self.op, self.auto_exposure, self.ev, self.key, self.lo, self.hi, self.adapt, self.white, self.min_ev,
                self.max_ev)

    def __repr__(self):
        return ("TonemapParams(op=%r, auto_exposure=%r, ev=%r, key=%r, lo=%r, hi=%r, adapt=%r, white=%r, min_ev=%r, "
                "max_ev=%r)" % self.values())


class TonemapState(ctypes.Structure):
    """amvpt_tonemap_state (include/amvpt_tonemap.h): the histogram of the last metered frame and the exposure it left.
    A zero-filled one (TonemapState()) is fresh."""
    _fields_ = [("hist", u32 * 512), ("counted", u32), ("skipped", u32), ("frames", u32), ("exposure", f32),
                ("log2_exposure", f64)]

    def histogram(self):
        return np.frombuffer(self, dtype=np.uint32, count=512).copy()


# amvpt_run_exchange_fn: (ctx, n_runs, *run_lane_begin, *run_count, *run_prefix, *total) -> 0 on success
RunExchangeFn = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, u32, ctypes.POINTER(u64), ctypes.POINTER(u64),
                                 ctypes.POINTER(u64), ctypes.POINTER(u64))


class RenderOpts(ctypes.Structure):
    """amvpt_render_opts: per-call chunk size, traversal, path-selection flags, run exchange, records, and
    (ABI 10) the device-memory budget in MiB (0: automatic)."""
    _fields_ = [("chunk_lanes", u64), ("traversal", u32), ("flags", u32), ("exchange", RunExchangeFn),
                ("exchange_ctx", ctypes.c_void_p), ("records", ctypes.c_void_p), ("record_pass", u32),
                ("budget_mib", u32)]


# amvpt_render_opts.flags (results are identical; kernel-path selection for tests / A/B)
OPT_GENERIC_KERNELS, OPT_WAVEFRONT_SUFFIX, OPT_SPLIT_NEE, OPT_ONE_STREAM, OPT_DETERMINISTIC = 1, 2, 4, 8, 16
OPT_NO_BINNING = 32
OPT_NO_BOX_SCREEN = 64
OPT_THREADED_BVH = 128
OPT_SPLIT_PRIMARY = 256
OPT_BLOCK_SPLAT = 512   # ABI 12: the per-lane block-window splat even where the row-reduced one is eligible
OPT_GENERIC_FLUSH = 2048  # the row splat's wave windows with run-time geometry and the generic flush loop everywhere
OPT_FIXED_DIRECT = 1024  # amvpt_fixed.h: direct puts into the fixed-point film instead of the integer LDS window

# amvpt_params.rfilter
RFILTER_BOX, RFILTER_GAUSSIAN, RFILTER_TENT, RFILTER_MITCHELL, RFILTER_CATMULLROM, RFILTER_LANCZOS = range(6)


def wrap_run_exchange(fn):
    """ctypes callback around `fn(run_lane_begin: list, run_count: list) -> (run_prefix: list, total)`
    (exceptions -> status 1)."""
    def cb(_ctx, n, begins, counts, prefix, total):
        try:
            pre, tot = fn([int(begins[i]) for i in range(n)], [int(counts[i]) for i in range(n)])
            for i in range(n):
                prefix[i] = int(pre[i])
            total[0] = int(tot)
            return 0
        except Exception:   # noqa: BLE001 -- reported to the C side as a failed exchange
            return 1
    return RunExchangeFn(cb)


# amvpt_kernel_id (include/amvpt.h): index -> name of Counters.kernel_ms / kernel_launches
KERNELS = ("k_prim_hit", "k_prim_req", "k_vis", "k_mv_primary", "k_raygen", "k_extend", "k_bounce", "k_shadow",
           "k_splat", "k_suffix", "k_select", "k_bin")


INTEGRATOR_MVPATH, INTEGRATOR_PATH = 0, 1
EMITTER_AREA, EMITTER_CONSTANT = 0, 1
_hip = None
_host = None


def hip_lib():
    """Load libamvpt_hip.so (the C-ABI of the hot path); raises if it was not built."""
    global _hip
    if _hip is None:
        if not os.path.exists(HIP_LIB_PATH):
            raise RuntimeError("libamvpt_hip.so missing: run `make -C mitsuba3-amvpt_amd` "
                               "(__graft_entry__.build()); the product path has no fallback")
        L = ctypes.CDLL(HIP_LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        L.amvpt_last_error.restype = ctypes.c_char_p
        L.amvpt_abi_version.restype = u32
        L.amvpt_film_channels.restype = u32
        for fn in ("amvpt_device_count", "amvpt_set_device", "amvpt_scene_create", "amvpt_scene_destroy",
                   "amvpt_scene_stats", "amvpt_render", "amvpt_render_records", "amvpt_plan",
                   "amvpt_develop", "amvpt_set_chunk_lanes", "amvpt_set_traversal",
                   "amvpt_set_adaptive_exchange", "amvpt_set_bvh_build", "amvpt_render_ex", "amvpt_scene_desc_boxes",
                   "amvpt_release_device_memory"):
            if hasattr(L, fn):   # older variant builds (AMVPT_LIB_DIR A/B runs) may lack the newest knobs
                getattr(L, fn).restype = ctypes.c_int
        L.amvpt_render.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(Params), u64, u64,
                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(Counters)]
        if hasattr(L, "amvpt_render_ex"):
            L.amvpt_render_ex.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(Params),
                                          ctypes.POINTER(LaneSet), ctypes.POINTER(FilmWindow), ctypes.c_void_p,
                                          ctypes.POINTER(RenderOpts), ctypes.POINTER(Counters)]
        L.amvpt_render_records.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(Params), u32, u64,
                                           u64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.amvpt_scene_create.argtypes = [ctypes.POINTER(SceneDesc), ctypes.POINTER(ctypes.c_void_p)]
        L.amvpt_scene_destroy.argtypes = [ctypes.c_void_p]
        L.amvpt_scene_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(u32), ctypes.POINTER(u32)]
        L.amvpt_plan.argtypes = [ctypes.POINTER(Params), ctypes.POINTER(u32), ctypes.POINTER(u32),
                                 ctypes.POINTER(u32), ctypes.POINTER(u64)]
        L.amvpt_develop.argtypes = [ctypes.c_void_p, ctypes.c_void_p, u32, u32, u32, ctypes.c_void_p]
        L.amvpt_set_chunk_lanes.argtypes = [u64]
        if hasattr(L, "amvpt_set_bvh_build"):
            L.amvpt_set_bvh_build.argtypes = [u32, ctypes.c_float]
        if hasattr(L, "amvpt_set_adaptive_exchange"):
            L.amvpt_set_adaptive_exchange.argtypes = [ExchangeFn, ctypes.c_void_p]
        L.amvpt_set_device.argtypes = [ctypes.c_int]
        if hasattr(L, "amvpt_release_device_memory"):
            L.amvpt_release_device_memory.argtypes = [ctypes.c_int]
        L.amvpt_device_count.argtypes = [ctypes.POINTER(ctypes.c_int)]
        if hasattr(L, "amvpt_rfilter_eval"):
            L.amvpt_rfilter_eval.restype = ctypes.c_int
            L.amvpt_rfilter_eval.argtypes = [ctypes.POINTER(Params), ctypes.c_void_p, u32, ctypes.c_void_p,
                                             ctypes.POINTER(f32)]
        if hasattr(L, "amvpt_fixed_version"):   # include/amvpt_fixed.h
            L.amvpt_fixed_version.restype = u32
            for fn in ("amvpt_render_fixed", "amvpt_fixed_accumulate", "amvpt_fixed_resolve",
                       "amvpt_fixed_accumulate_host", "amvpt_fixed_resolve_host"):
                getattr(L, fn).restype = ctypes.c_int
            L.amvpt_render_fixed.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(Params),
                                             ctypes.POINTER(LaneSet), ctypes.POINTER(FixedWindow), ctypes.c_void_p,
                                             ctypes.POINTER(RenderOpts), ctypes.POINTER(Counters)]
            acc = [ctypes.c_void_p, u32, u32, u32, ctypes.c_void_p, u32, u32, u32, u32, ctypes.c_void_p, u64]
            L.amvpt_fixed_accumulate.argtypes = acc + [ctypes.c_void_p]
            L.amvpt_fixed_accumulate_host.argtypes = acc
            L.amvpt_fixed_resolve.argtypes = [ctypes.c_void_p, ctypes.c_void_p, u64, ctypes.c_int, ctypes.c_void_p]
            L.amvpt_fixed_resolve_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, u64, ctypes.c_int]
        if hasattr(L, "amvpt_guides_version"):   # include/amvpt_guides.h
            vp = ctypes.c_void_p
            L.amvpt_guides_version.restype = u32
            for fn, args in (("amvpt_guides", [vp, vp, ctypes.POINTER(Params), ctypes.POINTER(u32 * 4), vp, vp]),
                             ("amvpt_guide_depth", [vp, vp, u32, u64, vp, vp]),
                             ("amvpt_guide_depth_host", [vp, vp, u32, u64, vp]),
                             ("amvpt_guide_depth_range", [vp, u64, ctypes.POINTER(f32 * 2), vp]),
                             ("amvpt_guide_depth_range_host", [vp, u64, ctypes.POINTER(f32 * 2)]),
                             ("amvpt_depth8", [vp, u32, u32, f32, f32, vp, vp]),
                             ("amvpt_depth8_host", [vp, u32, u32, f32, f32, vp])):
                getattr(L, fn).restype = ctypes.c_int
                getattr(L, fn).argtypes = args
        if hasattr(L, "amvpt_denoise_version"):   # include/amvpt_denoise.h
            vp = ctypes.c_void_p
            L.amvpt_denoise_version.restype = u32
            L.amvpt_denoise_default_params.restype = DenoiseParams
            L.amvpt_denoise_default_params.argtypes = []
            L.amvpt_denoise.restype = L.amvpt_denoise_host.restype = ctypes.c_int
            L.amvpt_denoise.argtypes = [vp, u32, u32, u32, vp, ctypes.POINTER(DenoiseParams), vp, vp, vp]
            L.amvpt_denoise_host.argtypes = [vp, u32, u32, u32, vp, ctypes.POINTER(DenoiseParams), vp, vp]
        if hasattr(L, "amvpt_temporal_version"):   # include/amvpt_temporal.h
            vp = ctypes.c_void_p
            L.amvpt_temporal_version.restype = u32
            L.amvpt_temporal_default_params.restype = TemporalParams
            L.amvpt_temporal_default_params.argtypes = []
            L.amvpt_temporal.restype = L.amvpt_temporal_host.restype = ctypes.c_int
            planes = [vp, u32, vp, vp, vp, vp, vp, ctypes.POINTER(Params), ctypes.POINTER(u32 * 4),
                      ctypes.POINTER(TemporalParams), vp, vp]
            L.amvpt_temporal.argtypes = planes + [vp]
            L.amvpt_temporal_host.argtypes = planes
        if hasattr(L, "amvpt_variance_version"):   # include/amvpt_variance.h
            vp = ctypes.c_void_p
            vq = ctypes.POINTER(VarianceParams)
            L.amvpt_variance_version.restype = u32
            L.amvpt_variance_default_params.restype = VarianceParams
            L.amvpt_variance_default_params.argtypes = []
            planes = [vp, u32, vp, vp, vp, vp, vp, vp, ctypes.POINTER(Params), ctypes.POINTER(u32 * 4),
                      ctypes.POINTER(TemporalParams), vp, vp, vp]
            for fn, args in (("amvpt_temporal_moments", planes + [vp]), ("amvpt_temporal_moments_host", planes),
                             ("amvpt_variance", [vp, vp, vp, u32, u32, vq, vp, vp]),
                             ("amvpt_variance_host", [vp, vp, vp, u32, u32, vq, vp]),
                             ("amvpt_denoise_variance", [vp, u32, u32, u32, vp, vp, vq, vp, vp, vp, vp, vp]),
                             ("amvpt_denoise_variance_host", [vp, u32, u32, u32, vp, vp, vq, vp, vp, vp, vp])):
                getattr(L, fn).restype = ctypes.c_int
                getattr(L, fn).argtypes = args
        if hasattr(L, "amvpt_synth_version"):   # include/amvpt_synth.h
            vp = ctypes.c_void_p
            sq = ctypes.POINTER(SynthParams)
            L.amvpt_synth_version.restype = u32
            L.amvpt_synth_default_params.restype = SynthParams
            L.amvpt_synth_default_params.argtypes = []
            planes = [vp, u32, vp, vp, ctypes.POINTER(Params), vp, vp, ctypes.POINTER(Params), ctypes.POINTER(u32 * 4), sq, vp, vp]
            fill = [vp, u32, u32, u32, vp, vp, sq, vp, vp, vp, vp]
            for fn, args in (("amvpt_synth", planes + [vp]), ("amvpt_synth_host", planes),
                             ("amvpt_synth_fill", fill + [vp]), ("amvpt_synth_fill_host", fill)):
                getattr(L, fn).restype = ctypes.c_int
                getattr(L, fn).argtypes = args
        if hasattr(L, "amvpt_tonemap_version"):   # include/amvpt_tonemap.h
            vp = ctypes.c_void_p
            tq, rc = ctypes.POINTER(TonemapParams), ctypes.POINTER(u32 * 4)
            L.amvpt_tonemap_version.restype = u32
            L.amvpt_tonemap_default_params.restype = TonemapParams
            L.amvpt_tonemap_default_params.argtypes = []
            L.amvpt_tonemap_exp2_host.restype = f64
            L.amvpt_tonemap_exp2_host.argtypes = [f64]
            for fn, args in (("amvpt_tonemap_meter", [vp, u32, u32, u32, rc, tq, vp, vp]),
                             ("amvpt_tonemap_meter_host", [vp, u32, u32, u32, rc, tq, vp]),
                             ("amvpt_tonemap_apply", [vp, u32, u32, u32, tq, vp, vp, vp]),
                             ("amvpt_tonemap_apply_host", [vp, u32, u32, u32, tq, vp, vp]),
                             ("amvpt_tonemap_srgb8", [vp, u32, u32, u32, tq, vp, vp, vp]),
                             ("amvpt_tonemap_srgb8_host", [vp, u32, u32, u32, tq, vp, vp])):
                getattr(L, fn).restype = ctypes.c_int
                getattr(L, fn).argtypes = args
        _hip = L
    return _hip


def denoise_version():
    """AMVPT_DENOISE_VERSION of the loaded library (include/amvpt_denoise.h)."""
    return hip_lib().amvpt_denoise_version()


def denoise_default_params():
    """amvpt_denoise_default_params of the loaded library."""
    c = hip_lib().amvpt_denoise_default_params()
    return DenoiseParams(*c.values())


def denoise_device(image_ptr, channels, width, height, guides_ptr, out_ptr, scratch_ptr=None, params=None, stream=None):
    """amvpt_denoise over device pointers, ordered on `stream`: the height x width x channels float32 image and its
    height x width x 8 guide records -> out_ptr; scratch_ptr (the image's size) may be None when iterations is 1."""
    L = hip_lib()
    q = params if params is not None else denoise_default_params()
    _check(L.amvpt_denoise(ctypes.c_void_p(image_ptr), channels, width, height, ctypes.c_void_p(guides_ptr),
                           ctypes.byref(q), ctypes.c_void_p(out_ptr), ctypes.c_void_p(scratch_ptr or 0),
                           ctypes.c_void_p(stream or 0)), L)


def denoise_host(image, guides, params=None):
    """amvpt_denoise_host over numpy: (H, W, 3 or 4) float32 image and (H, W, 8) guide records -> the filtered image.
    Bit-identical to the device entry; needs no device."""
    L = hip_lib()
    img = np.ascontiguousarray(image, dtype=np.float32)
    g = np.ascontiguousarray(guides, dtype=np.float32)
    if img.ndim != 3 or g.shape != img.shape[:2] + (8,):
        raise ValueError("denoise_host: an (H, W, C) image and (H, W, 8) guide records of its size are needed")
    q = params if params is not None else denoise_default_params()
    h, w, c = img.shape
    out = np.empty_like(img)
    scratch = np.empty_like(img) if q.iterations > 1 else None
    _check(L.amvpt_denoise_host(img.ctypes.data, c, w, h, g.ctypes.data, ctypes.byref(q), out.ctypes.data,
                                scratch.ctypes.data if scratch is not None else None), L)
    return out


def denoise_sigma_plane(guides):
    """The default sigma_plane of `denoise` for these guide records: 1/40 of the largest side of the bounding box
    of their hit points, as a float32 (0.05 for the Cornell box; the C default when nothing is hit)."""
    g = np.asarray(guides, dtype=np.float32).reshape(-1, 8)
    pts = g[g[:, 0] >= 0][:, 4:7]
    side = np.float32((pts.max(axis=0) - pts.min(axis=0)).max()) if len(pts) else np.float32(0)
    return float(side / np.float32(40)) if side > 0 else 0.05


def temporal_version():
    """AMVPT_TEMPORAL_VERSION of the loaded library (include/amvpt_temporal.h)."""
    return hip_lib().amvpt_temporal_version()


def temporal_default_params():
    """amvpt_temporal_default_params of the loaded library."""
    c = hip_lib().amvpt_temporal_default_params()
    return TemporalParams(*c.values())


def _views_ptr(views):
    return ctypes.cast(views, ctypes.c_void_p) if views is not None else None


def _rect_ref(rect):
    return ctypes.byref((u32 * 4)(*[int(v) for v in rect])) if rect is not None else None


def temporal_device(image_ptr, channels, guides_ptr, hist_image_ptr, hist_guides_ptr, hist_count_ptr, prev_views, params,
                    out_image_ptr, out_count_ptr, tp=None, rect=None, stream=None):
    """amvpt_temporal over device pointers, ordered on `stream`: the current developed image and guide records, the
    previous call's outputs (image, guide records, count) and the host ViewDesc table the history was rendered with
    -> out_image_ptr, out_count_ptr.  `params` gives the quilt layout; `rect` = (x0, y0, w, h), whole tiles of the
    quilt that every plane holds alone (None: all of it)."""
    L = hip_lib()
    q = tp if tp is not None else temporal_default_params()
    _check(L.amvpt_temporal(ctypes.c_void_p(image_ptr), channels, ctypes.c_void_p(guides_ptr),
                            ctypes.c_void_p(hist_image_ptr), ctypes.c_void_p(hist_guides_ptr),
                            ctypes.c_void_p(hist_count_ptr), _views_ptr(prev_views), ctypes.byref(params), _rect_ref(rect),
                            ctypes.byref(q), ctypes.c_void_p(out_image_ptr), ctypes.c_void_p(out_count_ptr),
                            ctypes.c_void_p(stream or 0)), L)


def temporal_host(image, guides, hist_image, hist_guides, hist_count, prev_views, params, tp=None, rect=None):
    """amvpt_temporal_host over numpy: (H, W, 3 or 4) float32 image, (H, W, 8) guide records, the history planes of
    the same size ((H, W, C), (H, W, 8), (H, W)) and the host ViewDesc table of the history -> (image, count).
    Bit-identical to the device entry; needs no device."""
    L = hip_lib()
    img = np.ascontiguousarray(image, dtype=np.float32)
    g = np.ascontiguousarray(guides, dtype=np.float32)
    hi = np.ascontiguousarray(hist_image, dtype=np.float32)
    hg = np.ascontiguousarray(hist_guides, dtype=np.float32)
    hc = np.ascontiguousarray(hist_count, dtype=np.float32)
    if img.ndim != 3 or g.shape != img.shape[:2] + (8,):
        raise ValueError("temporal_host: an (H, W, C) image and (H, W, 8) guide records of its size are needed")
    if hi.shape != img.shape or hg.shape != g.shape or hc.size != g.shape[0] * g.shape[1]:
        raise ValueError("temporal_host: the history planes must have the sizes of the image, the guides and (H, W)")
    q = tp if tp is not None else temporal_default_params()
    out, cnt = np.empty_like(img), np.empty(img.shape[:2], dtype=np.float32)
    _check(L.amvpt_temporal_host(img.ctypes.data, img.shape[2], g.ctypes.data, hi.ctypes.data, hg.ctypes.data,
                                 hc.ctypes.data, _views_ptr(prev_views), ctypes.byref(params), _rect_ref(rect),
                                 ctypes.byref(q), out.ctypes.data, cnt.ctypes.data), L)
    return out, cnt


def variance_version():
    """AMVPT_VARIANCE_VERSION of the loaded library (include/amvpt_variance.h)."""
    return hip_lib().amvpt_variance_version()


def variance_default_params():
    """amvpt_variance_default_params of the loaded library."""
    c = hip_lib().amvpt_variance_default_params()
    return VarianceParams(*c.values())


def temporal_moments_device(image_ptr, channels, guides_ptr, hist_image_ptr, hist_guides_ptr, hist_count_ptr, hist_moments_ptr,
                            prev_views, params, out_image_ptr, out_count_ptr, out_moments_ptr, tp=None, rect=None, stream=None):
    """amvpt_temporal_moments over device pointers: temporal_device with the (H, W, 2) planes of the luminance moments,
    hist_moments_ptr in and out_moments_ptr out."""
    L = hip_lib()
    q = tp if tp is not None else temporal_default_params()
    _check(L.amvpt_temporal_moments(ctypes.c_void_p(image_ptr), channels, ctypes.c_void_p(guides_ptr),
                                    ctypes.c_void_p(hist_image_ptr), ctypes.c_void_p(hist_guides_ptr),
                                    ctypes.c_void_p(hist_count_ptr), ctypes.c_void_p(hist_moments_ptr), _views_ptr(prev_views),
                                    ctypes.byref(params), _rect_ref(rect), ctypes.byref(q), ctypes.c_void_p(out_image_ptr),
                                    ctypes.c_void_p(out_count_ptr), ctypes.c_void_p(out_moments_ptr),
                                    ctypes.c_void_p(stream or 0)), L)


def temporal_moments_host(image, guides, hist_image, hist_guides, hist_count, hist_moments, prev_views, params, tp=None,
                          rect=None):
    """amvpt_temporal_moments_host over numpy: temporal_host with the (H, W, 2) history of the luminance moments ->
    (image, count, moments).  Image and count are temporal_host's, bit for bit."""
    L = hip_lib()
    img = np.ascontiguousarray(image, dtype=np.float32)
    g = np.ascontiguousarray(guides, dtype=np.float32)
    hi = np.ascontiguousarray(hist_image, dtype=np.float32)
    hg = np.ascontiguousarray(hist_guides, dtype=np.float32)
    hc = np.ascontiguousarray(hist_count, dtype=np.float32)
    hm = np.ascontiguousarray(hist_moments, dtype=np.float32)
    if img.ndim != 3 or g.shape != img.shape[:2] + (8,):
        raise ValueError("temporal_moments_host: an (H, W, C) image and (H, W, 8) guide records of its size are needed")
    if hi.shape != img.shape or hg.shape != g.shape or hc.size != g.shape[0] * g.shape[1] or hm.shape != g.shape[:2] + (2,):
        raise ValueError("temporal_moments_host: the history planes must have the sizes of the image, the guides, (H, W) "
                         "and (H, W, 2)")
    q = tp if tp is not None else temporal_default_params()
    out, cnt, mom = np.empty_like(img), np.empty(img.shape[:2], dtype=np.float32), np.empty_like(hm)
    _check(L.amvpt_temporal_moments_host(img.ctypes.data, img.shape[2], g.ctypes.data, hi.ctypes.data, hg.ctypes.data,
                                         hc.ctypes.data, hm.ctypes.data, _views_ptr(prev_views), ctypes.byref(params),
                                         _rect_ref(rect), ctypes.byref(q), out.ctypes.data, cnt.ctypes.data, mom.ctypes.data), L)
    return out, cnt, mom


def variance_device(moments_ptr, count_ptr, guides_ptr, width, height, out_ptr, params=None, stream=None):
    """amvpt_variance over device pointers, ordered on `stream`: (H, W, 2) moments, (H, W) count and (H, W, 8) guide
    records -> the (H, W) variance of the accumulated luminance at out_ptr."""
    L = hip_lib()
    q = params if params is not None else variance_default_params()
    _check(L.amvpt_variance(ctypes.c_void_p(moments_ptr), ctypes.c_void_p(count_ptr), ctypes.c_void_p(guides_ptr), width,
                            height, ctypes.byref(q), ctypes.c_void_p(out_ptr), ctypes.c_void_p(stream or 0)), L)


def variance_host(moments, count, guides, params=None):
    """amvpt_variance_host over numpy: (H, W, 2) moments, (H, W) count, (H, W, 8) guide records -> (H, W) variance.
    Bit-identical to the device entry; needs no device."""
    L = hip_lib()
    m = np.ascontiguousarray(moments, dtype=np.float32)
    g = np.ascontiguousarray(guides, dtype=np.float32)
    c = np.ascontiguousarray(count, dtype=np.float32)
    if g.ndim != 3 or g.shape[2] != 8 or m.shape != g.shape[:2] + (2,) or c.shape != g.shape[:2]:
        raise ValueError("variance_host: (H, W, 2) moments, an (H, W) count and (H, W, 8) guide records are needed")
    q = params if params is not None else variance_default_params()
    out = np.empty(g.shape[:2], dtype=np.float32)
    _check(L.amvpt_variance_host(m.ctypes.data, c.ctypes.data, g.ctypes.data, g.shape[1], g.shape[0], ctypes.byref(q),
                                 out.ctypes.data), L)
    return out


def denoise_variance_device(image_ptr, channels, width, height, variance_ptr, guides_ptr, out_ptr, scratch_ptr=None,
                            var_out_ptr=None, var_scratch_ptr=None, params=None, stream=None):
    """amvpt_denoise_variance over device pointers, ordered on `stream`: image, (H, W) variance and guide records ->
    out_ptr and, where given, the filtered variance at var_out_ptr.  scratch_ptr and var_scratch_ptr may be None when
    iterations is 1, var_out_ptr when it is at most 2."""
    L = hip_lib()
    q = params if params is not None else variance_default_params()
    _check(L.amvpt_denoise_variance(ctypes.c_void_p(image_ptr), channels, width, height, ctypes.c_void_p(variance_ptr),
                                    ctypes.c_void_p(guides_ptr), ctypes.byref(q), ctypes.c_void_p(out_ptr),
                                    ctypes.c_void_p(scratch_ptr or 0), ctypes.c_void_p(var_out_ptr or 0),
                                    ctypes.c_void_p(var_scratch_ptr or 0), ctypes.c_void_p(stream or 0)), L)


def denoise_variance_host(image, variance, guides, params=None):
    """amvpt_denoise_variance_host over numpy: (H, W, 3 or 4) image, (H, W) variance, (H, W, 8) guide records ->
    (filtered image, filtered variance).  Bit-identical to the device entry; needs no device."""
    L = hip_lib()
    img = np.ascontiguousarray(image, dtype=np.float32)
    g = np.ascontiguousarray(guides, dtype=np.float32)
    v = np.ascontiguousarray(variance, dtype=np.float32)
    if img.ndim != 3 or g.shape != img.shape[:2] + (8,) or v.shape != img.shape[:2]:
        raise ValueError("denoise_variance_host: an (H, W, C) image, an (H, W) variance and (H, W, 8) guide records of its "
                         "size are needed")
    q = params if params is not None else variance_default_params()
    h, w, c = img.shape
    out, vout = np.empty_like(img), np.empty_like(v)
    scratch, vscratch = (np.empty_like(img), np.empty_like(v)) if q.iterations > 1 else (None, None)
    _check(L.amvpt_denoise_variance_host(img.ctypes.data, c, w, h, v.ctypes.data, g.ctypes.data, ctypes.byref(q),
                                         out.ctypes.data, scratch.ctypes.data if scratch is not None else None,
                                         vout.ctypes.data, vscratch.ctypes.data if vscratch is not None else None), L)
    return out, vout


def synth_version():
    """AMVPT_SYNTH_VERSION of the loaded library (include/amvpt_synth.h)."""
    return hip_lib().amvpt_synth_version()


def synth_default_params():
    """amvpt_synth_default_params of the loaded library."""
    c = hip_lib().amvpt_synth_default_params()
    return SynthParams(*c.values())


def synth_device(src_image_ptr, channels, src_guides_ptr, src_views, src_params, dst_guides_ptr, dst_views, dst_params,
                 dst_image_ptr, dst_cover_ptr, sp=None, rect=None, stream=None):
    """amvpt_synth over device pointers, ordered on `stream`: the source quilt (image, guide records, the host ViewDesc
    table and the Params of its layout) and the target quilt's guide records, views and Params -> dst_image_ptr,
    dst_cover_ptr.  `rect` = (x0, y0, w, h), whole tiles of the target quilt that the target planes hold alone (None: all
    of it)."""
    L = hip_lib()
    q = sp if sp is not None else synth_default_params()
    _check(L.amvpt_synth(ctypes.c_void_p(src_image_ptr), channels, ctypes.c_void_p(src_guides_ptr), _views_ptr(src_views),
                         ctypes.byref(src_params), ctypes.c_void_p(dst_guides_ptr), _views_ptr(dst_views),
                         ctypes.byref(dst_params), _rect_ref(rect), ctypes.byref(q), ctypes.c_void_p(dst_image_ptr),
                         ctypes.c_void_p(dst_cover_ptr), ctypes.c_void_p(stream or 0)), L)


def synth_host(src_image, src_guides, src_views, src_params, dst_guides, dst_views, dst_params, sp=None, rect=None):
    """amvpt_synth_host over numpy: the (Hs, Ws, 3 or 4) float32 source image, its (Hs, Ws, 8) guide records, views and
    Params, and the target's (h, w, 8) guide records, views and Params -> (image (h, w, C), cover (h, w)).
    Bit-identical to the device entry; needs no device."""
    L = hip_lib()
    img = np.ascontiguousarray(src_image, dtype=np.float32)
    sg = np.ascontiguousarray(src_guides, dtype=np.float32)
    dg = np.ascontiguousarray(dst_guides, dtype=np.float32)
    if img.ndim != 3 or sg.shape != img.shape[:2] + (8,):
        raise ValueError("synth_host: an (Hs, Ws, C) source image and (Hs, Ws, 8) guide records of its size are needed")
    if img.shape[:2] != (int(src_params.film_height), int(src_params.film_width)):
        raise ValueError("synth_host: the source planes must hold the whole film of src_params")
    want = (int(rect[3]), int(rect[2])) if rect is not None else (int(dst_params.film_height), int(dst_params.film_width))
    if dg.ndim != 3 or dg.shape != want + (8,):
        raise ValueError("synth_host: (h, w, 8) target guide records of the rectangle (or of dst_params' film) are needed")
    q = sp if sp is not None else synth_default_params()
    out, cover = np.empty(dg.shape[:2] + (img.shape[2],), dtype=np.float32), np.empty(dg.shape[:2], dtype=np.float32)
    _check(L.amvpt_synth_host(img.ctypes.data, img.shape[2], sg.ctypes.data, _views_ptr(src_views), ctypes.byref(src_params),
                              dg.ctypes.data, _views_ptr(dst_views), ctypes.byref(dst_params), _rect_ref(rect),
                              ctypes.byref(q), out.ctypes.data, cover.ctypes.data), L)
    return out, cover


def synth_fill_device(image_ptr, channels, width, height, cover_ptr, guides_ptr, out_ptr, cover_out_ptr, scratch_ptr=None,
                      cover_scratch_ptr=None, sp=None, stream=None):
    """amvpt_synth_fill over device pointers, ordered on `stream`: sp.fill_iterations iterations of the hole fill ->
    out_ptr, cover_out_ptr.  scratch_ptr and cover_scratch_ptr may be None when fill_iterations is at most 1."""
    L = hip_lib()
    q = sp if sp is not None else synth_default_params()
    _check(L.amvpt_synth_fill(ctypes.c_void_p(image_ptr), channels, width, height, ctypes.c_void_p(cover_ptr),
                              ctypes.c_void_p(guides_ptr), ctypes.byref(q), ctypes.c_void_p(out_ptr),
                              ctypes.c_void_p(scratch_ptr or 0), ctypes.c_void_p(cover_out_ptr),
                              ctypes.c_void_p(cover_scratch_ptr or 0), ctypes.c_void_p(stream or 0)), L)


def synth_fill_host(image, cover, guides, sp=None):
    """amvpt_synth_fill_host over numpy: (H, W, 3 or 4) image, (H, W) cover, (H, W, 8) guide records -> (image, cover)
    after sp.fill_iterations iterations.  Bit-identical to the device entry; needs no device."""
    L = hip_lib()
    img = np.ascontiguousarray(image, dtype=np.float32)
    g = np.ascontiguousarray(guides, dtype=np.float32)
    c = np.ascontiguousarray(cover, dtype=np.float32)
    if img.ndim != 3 or g.shape != img.shape[:2] + (8,) or c.shape != img.shape[:2]:
        raise ValueError("synth_fill_host: an (H, W, C) image, an (H, W) cover and (H, W, 8) guide records of its size are needed")
    q = sp if sp is not None else synth_default_params()
    h, w, ch = img.shape
    out, cout = np.empty_like(img), np.empty_like(c)
    scratch, cscratch = (np.empty_like(img), np.empty_like(c)) if q.fill_iterations > 1 else (None, None)
    _check(L.amvpt_synth_fill_host(img.ctypes.data, ch, w, h, c.ctypes.data, g.ctypes.data, ctypes.byref(q), out.ctypes.data,
                                   scratch.ctypes.data if scratch is not None else None, cout.ctypes.data,
                                   cscratch.ctypes.data if cscratch is not None else None), L)
    return out, cout


def tonemap_version():
    """AMVPT_TONEMAP_VERSION of the loaded library (include/amvpt_tonemap.h)."""
    return hip_lib().amvpt_tonemap_version()


def tonemap_default_params():
    """amvpt_tonemap_default_params of the loaded library."""
    c = hip_lib().amvpt_tonemap_default_params()
    return TonemapParams(*c.values())


def tonemap_exp2_host(x):
    """exp2_pm of include/amvpt_tonemap.h at the float64 x (amvpt_tonemap_exp2_host)."""
    return hip_lib().amvpt_tonemap_exp2_host(float(x))


def _tonemap_image(who, image):
    img = np.ascontiguousarray(image, dtype=np.float32)
    if img.ndim != 3:
        raise ValueError("%s: an (H, W, C) image is needed" % who)
    return img


def tonemap_meter_device(image_ptr, channels, width, height, state_ptr, params=None, rect=None, stream=None):
    """amvpt_tonemap_meter over device pointers, ordered on `stream`: the histogram of the image (`rect` = (x0, y0, w,
    h) in pixels; None: all of it) and the exposure it gives, into the amvpt_tonemap_state at state_ptr."""
    L = hip_lib()
    q = params if params is not None else tonemap_default_params()
    _check(L.amvpt_tonemap_meter(ctypes.c_void_p(image_ptr), channels, width, height, _rect_ref(rect), ctypes.byref(q),
                                 ctypes.c_void_p(state_ptr), ctypes.c_void_p(stream or 0)), L)


def tonemap_device(image_ptr, channels, width, height, out_ptr, params=None, state_ptr=None, stream=None):
    """amvpt_tonemap_apply over device pointers, ordered on `stream`: height x width x channels float32 at out_ptr, which
    may be image_ptr itself.  state_ptr may be None unless params.auto_exposure is set."""
    L = hip_lib()
    q = params if params is not None else tonemap_default_params()
    _check(L.amvpt_tonemap_apply(ctypes.c_void_p(image_ptr), channels, width, height, ctypes.byref(q),
                                 ctypes.c_void_p(state_ptr or 0), ctypes.c_void_p(out_ptr), ctypes.c_void_p(stream or 0)), L)


def tonemap_srgb8_device(image_ptr, channels, width, height, out_ptr, params=None, state_ptr=None, stream=None):
    """amvpt_tonemap_srgb8 over device pointers, ordered on `stream`: height x width x 3 uint8 at out_ptr."""
    L = hip_lib()
    q = params if params is not None else tonemap_default_params()
    _check(L.amvpt_tonemap_srgb8(ctypes.c_void_p(image_ptr), channels, width, height, ctypes.byref(q),
                                 ctypes.c_void_p(state_ptr or 0), ctypes.c_void_p(out_ptr), ctypes.c_void_p(stream or 0)), L)


def tonemap_meter_host(image, params=None, state=None, rect=None):
    """amvpt_tonemap_meter_host over numpy: meters the (H, W, 3 or 4) float32 image into `state` (a TonemapState, updated
    in place; None: a fresh one) and returns it.  Bit-identical to the device entry; needs no device."""
    L = hip_lib()
    img = _tonemap_image("tonemap_meter_host", image)
    q = params if params is not None else tonemap_default_params()
    s = state if state is not None else TonemapState()
    h, w, c = img.shape
    _check(L.amvpt_tonemap_meter_host(img.ctypes.data, c, w, h, _rect_ref(rect), ctypes.byref(q), ctypes.addressof(s)), L)
    return s


def tonemap_host(image, params=None, state=None, in_place=False):
    """amvpt_tonemap_apply_host over numpy: (H, W, 3 or 4) float32 -> the mapped floats, alpha passed through.
    in_place=True maps a contiguous float32 `image` onto itself and returns it."""
    L = hip_lib()
    img = _tonemap_image("tonemap_host", image)
    if in_place and img is not image:
        raise ValueError("tonemap_host: in_place needs a contiguous float32 array")
    q = params if params is not None else tonemap_default_params()
    out = img if in_place else np.empty_like(img)
    h, w, c = img.shape
    _check(L.amvpt_tonemap_apply_host(img.ctypes.data, c, w, h, ctypes.byref(q),
                                      ctypes.addressof(state) if state is not None else None, out.ctypes.data), L)
    return out


def tonemap_srgb8_host(image, params=None, state=None):
    """amvpt_tonemap_srgb8_host over numpy: (H, W, 3 or 4) float32 -> (H, W, 3) uint8 sRGB of the mapped colours."""
    L = hip_lib()
    img = _tonemap_image("tonemap_srgb8_host", image)
    q = params if params is not None else tonemap_default_params()
    h, w, c = img.shape
    out = np.empty((h, w, 3), dtype=np.uint8)
    _check(L.amvpt_tonemap_srgb8_host(img.ctypes.data, c, w, h, ctypes.byref(q),
                                      ctypes.addressof(state) if state is not None else None, out.ctypes.data), L)
    return out


def guides_version():
    """AMVPT_GUIDES_VERSION of the loaded library (include/amvpt_guides.h)."""
    return hip_lib().amvpt_guides_version()


def guide_depth(guides_ptr, views, n_views, n_pixels, depth_ptr, stream=None):
    """amvpt_guide_depth over device pointers: guide records -> planar depth (+inf on a miss), ordered on `stream`.
    `views` is the host ViewDesc table."""
    L = hip_lib()
    _check(L.amvpt_guide_depth(ctypes.c_void_p(guides_ptr), views, n_views, n_pixels,
                               ctypes.c_void_p(depth_ptr), ctypes.c_void_p(stream or 0)), L)


def guide_depth_host(guides, views, n_views):
    """amvpt_guide_depth_host over numpy: (..., 8) float32 guide records -> (...) float32 planar depth."""
    L = hip_lib()
    g = np.ascontiguousarray(guides, dtype=np.float32)
    if g.ndim < 1 or g.shape[-1] != 8:
        raise ValueError("guide_depth_host: (..., 8) guide records are needed")
    out = np.empty(g.shape[:-1], dtype=np.float32)
    _check(L.amvpt_guide_depth_host(g.ctypes.data, views, n_views, out.size, out.ctypes.data), L)
    return out


def guide_depth_range(depth_ptr, n, stream=None):
    """amvpt_guide_depth_range: (min, max) over the finite values of the device depth plane; (0, 0) when there is
    none.  Synchronises `stream`."""
    L = hip_lib()
    nf = (f32 * 2)()
    _check(L.amvpt_guide_depth_range(ctypes.c_void_p(depth_ptr), n, ctypes.byref(nf), ctypes.c_void_p(stream or 0)), L)
    return np.float32(nf[0]), np.float32(nf[1])


def guide_depth_range_host(depth):
    """amvpt_guide_depth_range_host over a numpy depth plane."""
    L = hip_lib()
    d = np.ascontiguousarray(depth, dtype=np.float32)
    nf = (f32 * 2)()
    _check(L.amvpt_guide_depth_range_host(d.ctypes.data if d.size else None, d.size, ctypes.byref(nf)), L)
    return np.float32(nf[0]), np.float32(nf[1])


def depth8(depth_ptr, width, height, near, far, out_ptr, stream=None):
    """amvpt_depth8 over device pointers: depth plane -> height x width x 3 uint8, nearer brighter, a miss 0."""
    L = hip_lib()
    _check(L.amvpt_depth8(ctypes.c_void_p(depth_ptr), width, height, float(near), float(far), ctypes.c_void_p(out_ptr),
                          ctypes.c_void_p(stream or 0)), L)


def depth8_host(depth, near, far):
    """amvpt_depth8_host over numpy: (H, W) float32 depth -> (H, W, 3) uint8."""
    L = hip_lib()
    d = np.ascontiguousarray(depth, dtype=np.float32)
    if d.ndim != 2:
        raise ValueError("depth8_host: an (H, W) depth plane is needed")
    h, w = d.shape
    out = np.empty((h, w, 3), dtype=np.uint8)
    _check(L.amvpt_depth8_host(d.ctypes.data if d.size else None, w, h, float(near), float(far), out.ctypes.data), L)
    return out


def fixed_version():
    """AMVPT_FIXED_VERSION of the loaded library (include/amvpt_fixed.h)."""
    return hip_lib().amvpt_fixed_version()


def fixed_accumulate(quilt_ptr, quilt_width, quilt_height, channels, window_ptr, window, entries_ptr=None,
                     n_entries=0, stream=None):
    """amvpt_fixed_accumulate: the int64 quilt (device) += the int64 window (x0, y0, width, height) and the
    `n_entries` 16-byte overflow entries at `entries_ptr` (the entries after a list's header)."""
    L = hip_lib()
    x0, y0, w, h = window
    _check(L.amvpt_fixed_accumulate(ctypes.c_void_p(quilt_ptr), quilt_width, quilt_height, channels,
                                    ctypes.c_void_p(window_ptr or 0), x0, y0, w, h,
                                    ctypes.c_void_p(entries_ptr or 0), n_entries, ctypes.c_void_p(stream)), L)


def fixed_accumulate_host(quilt, window_film, window, entries=None):
    """amvpt_fixed_accumulate_host over numpy arrays: `quilt` (H, W, C) int64, C-contiguous, updated in place;
    `window_film` (h, w, C) int64 or None; `window` (x0, y0, w, h); `entries` (n, 2) int64 (index, value) or None."""
    L = hip_lib()
    if quilt.dtype != np.int64 or not quilt.flags.c_contiguous or quilt.ndim != 3:
        raise ValueError("fixed_accumulate_host: quilt must be a C-contiguous (H, W, C) int64 array")
    x0, y0, w, h = window
    win = None if window_film is None else np.ascontiguousarray(window_film, dtype=np.int64)
    if win is not None and win.shape != (h, w, quilt.shape[2]):
        raise ValueError("fixed_accumulate_host: window_film is not (h, w, C) of `window`")
    ent = None if entries is None else np.ascontiguousarray(entries, dtype=np.int64).reshape(-1, 2)
    _check(L.amvpt_fixed_accumulate_host(quilt.ctypes.data, quilt.shape[1], quilt.shape[0], quilt.shape[2],
                                         win.ctypes.data if win is not None else None, x0, y0, w, h,
                                         ent.ctypes.data if ent is not None and len(ent) else None,
                                         len(ent) if ent is not None else 0), L)
    return quilt


def fixed_resolve(fixed_ptr, film_ptr, n_floats, add=False, stream=None):
    """amvpt_fixed_resolve: film[i] (float32, device) = or += (float) ((double) fixed[i] * 2^-32)."""
    L = hip_lib()
    _check(L.amvpt_fixed_resolve(ctypes.c_void_p(fixed_ptr), ctypes.c_void_p(film_ptr), n_floats, int(bool(add)),
                                 ctypes.c_void_p(stream)), L)


def fixed_resolve_host(fixed, film=None, add=False):
    """amvpt_fixed_resolve_host over numpy arrays: the float32 film of the int64 array `fixed` (same shape);
    with `add`, `film` (float32, C-contiguous) is added to in place."""
    L = hip_lib()
    fx = np.ascontiguousarray(fixed, dtype=np.int64)
    if film is None:
        if add:
            raise ValueError("fixed_resolve_host: add needs a film")
        film = np.empty(fx.shape, dtype=np.float32)
    if film.dtype != np.float32 or not film.flags.c_contiguous or film.size != fx.size:
        raise ValueError("fixed_resolve_host: film must be a C-contiguous float32 array of fixed's size")
    _check(L.amvpt_fixed_resolve_host(fx.ctypes.data, film.ctypes.data, fx.size, int(bool(add))), L)
    return film


def host_lib():
    global _host
    if _host is None:
        hip_lib()
        if not os.path.exists(HOST_LIB_PATH):
            raise RuntimeError("libamvpt_host.so missing: run `make -C mitsuba3-amvpt_amd`")
        L = ctypes.CDLL(HOST_LIB_PATH)
        L.amvpt_host_last_error.restype = ctypes.c_char_p
        L.amvpt_host_load_file.restype = ctypes.c_void_p
        L.amvpt_host_load_string.restype = ctypes.c_void_p
        L.amvpt_host_load_file.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        L.amvpt_host_load_string.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        L.amvpt_host_scene_free.argtypes = [ctypes.c_void_p]
        L.amvpt_host_sensor_count.argtypes = [ctypes.c_void_p]
        L.amvpt_host_sensor_count.restype = u32
        L.amvpt_host_film_info.argtypes = [ctypes.c_void_p, u32] + [ctypes.POINTER(u32)] * 4
        L.amvpt_host_render.argtypes = [ctypes.c_void_p, u32, u32, u32, ctypes.c_int, ctypes.c_void_p,
                                        ctypes.POINTER(Counters)]
        L.amvpt_host_render_stream.argtypes = [ctypes.c_void_p, u32, u32, u32, ctypes.c_int, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.POINTER(Counters)]
        L.amvpt_host_render_stats.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(u64)] * 3
        L.amvpt_host_render_multi.argtypes = [ctypes.c_void_p, u32, u32, u32, ctypes.c_int,
                                              ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_void_p,
                                              ctypes.POINTER(Counters)]
        L.amvpt_host_lane_shard.argtypes = [u64, u32, u32, ctypes.POINTER(u64), ctypes.POINTER(u64)]
        L.amvpt_host_lane_shard.restype = None
        L.amvpt_host_view_group_partition.argtypes = [ctypes.POINTER(Params), u32, u32, ctypes.POINTER(u32),
                                                      ctypes.POINTER(u32)]
        L.amvpt_host_multi_stats.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(u64)] * 3
        L.amvpt_host_describe.argtypes = [ctypes.c_void_p, u32, u32, u32, ctypes.POINTER(ctypes.POINTER(SceneDesc)),
                                          ctypes.POINTER(ctypes.POINTER(ViewDesc)), ctypes.POINTER(Params)]
        L.amvpt_host_integrator_string.argtypes = [ctypes.c_void_p]
        L.amvpt_host_integrator_string.restype = ctypes.c_char_p
        L.amvpt_host_write_exr.argtypes = [ctypes.c_char_p, ctypes.c_void_p, u32, u32, u32]
        L.amvpt_host_read_exr.argtypes = [ctypes.c_char_p, ctypes.c_void_p, u32, u32, u32]
        if hasattr(L, "amvpt_host_guides"):   # older variant builds (AMVPT_LIB_DIR A/B runs) lack the guide buffers
            L.amvpt_host_guides.argtypes = [ctypes.c_void_p, u32, ctypes.c_void_p, ctypes.c_void_p]
            names = ctypes.POINTER(ctypes.c_char_p)
            L.amvpt_host_write_exr_channels.argtypes = [ctypes.c_char_p, ctypes.c_void_p, u32, u32, u32, names]
            L.amvpt_host_read_exr_channels.argtypes = [ctypes.c_char_p, ctypes.c_void_p, u32, u32, u32, names]
        if hasattr(L, "amvpt_host_denoise_stream"):
            L.amvpt_host_denoise_stream.argtypes = [ctypes.c_void_p, u32, ctypes.POINTER(DenoiseParams), ctypes.c_void_p,
                                                    ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        L.amvpt_host_parse_fov.argtypes = [f64, ctypes.c_char_p, ctypes.c_char_p, f64]
        L.amvpt_host_parse_fov.restype = f64
        L.amvpt_host_perspective_projection.argtypes = [ctypes.POINTER(ctypes.c_int)] * 3 + [f32, f32, f32,
                                                                                              ctypes.POINTER(f32)]
        _host = L
    return _host


def _defines(kw):
    keys = [k.encode() for k in kw]
    vals = [str(v).encode() for v in kw.values()]
    K = (ctypes.c_char_p * max(1, len(keys)))(*keys)
    V = (ctypes.c_char_p * max(1, len(vals)))(*vals)
    return K, V, len(keys)


def _check(rc, lib):
    if rc != 0:
        raise RuntimeError((lib.amvpt_host_last_error() if lib is _host else lib.amvpt_last_error()).decode())


class Scene:
    """A loaded scene (Scene + its sensors/integrator), as `mi.load_file` returns."""

    def __init__(self, handle):
        self._h = handle
        self._lib = host_lib()

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.amvpt_host_scene_free(self._h)
            self._h = None

    def sensor_count(self):
        return self._lib.amvpt_host_sensor_count(self._h)

    def film_info(self, sensor=0):
        w, h, c, s = u32(), u32(), u32(), u32()
        _check(self._lib.amvpt_host_film_info(self._h, sensor, w, h, c, s), self._lib)
        return w.value, h.value, c.value, s.value

    def integrator_string(self):
        return self._lib.amvpt_host_integrator_string(self._h).decode()

    def describe(self, sensor=0, seed=0, spp=0):
        """(SceneDesc*, ViewDesc*, Params) exactly as render() passes them to the C-ABI."""
        sd = ctypes.POINTER(SceneDesc)()
        vd = ctypes.POINTER(ViewDesc)()
        p = Params()
        _check(self._lib.amvpt_host_describe(self._h, sensor, seed, spp, ctypes.byref(sd), ctypes.byref(vd),
                                             ctypes.byref(p)), self._lib)
        return sd, vd, p


def rfilter_eval(params, xs):
    """(values, radius) of the reconstruction filter of `params` at the float32 arguments `xs`: the function the
    splat kernels evaluate, compiled for the host (amvpt_rfilter_eval; needs no device)."""
    import numpy as np
    L = hip_lib()
    x = np.ascontiguousarray(xs, dtype=np.float32).ravel()
    out = np.empty_like(x)
    radius = f32()
    rc = L.amvpt_rfilter_eval(ctypes.byref(params), x.ctypes.data, x.size, out.ctypes.data, ctypes.byref(radius))
    if rc != 0:
        raise RuntimeError(L.amvpt_last_error().decode())
    return out.reshape(np.shape(xs)), radius.value


def load_file(path, **defines):
    L = host_lib()
    K, V, n = _defines(defines)
    h = L.amvpt_host_load_file(path.encode(), K, V, n)
    if not h:
        raise RuntimeError(L.amvpt_host_last_error().decode())
    return Scene(h)


def load_string(xml, **defines):
    L = host_lib()
    K, V, n = _defines(defines)
    h = L.amvpt_host_load_string(xml.encode(), K, V, n)
    if not h:
        raise RuntimeError(L.amvpt_host_last_error().decode())
    return Scene(h)


def render(scene, sensor=0, seed=0, spp=0, raw=False, counters=None, stream=None):
    """Integrator::render(scene, sensor, seed, spp, develop=not raw) -> numpy (H, W, C), on the current
    device and `stream` (a hipStream_t handle; None: the default stream).  The device scene and the film
    are cached on the scene (render_stats)."""
    w, h, c, _ = scene.film_info(sensor)
    _, _, p = scene.describe(sensor, seed, spp)
    ch = (5 if p.film_alpha else 4) if raw else c
    out = np.zeros((h, w, ch), dtype=np.float32)
    cnt = counters if counters is not None else Counters()
    _check(scene._lib.amvpt_host_render_stream(scene._h, sensor, seed, spp, 1 if raw else 0,
                                               out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(stream or 0),
                                               ctypes.byref(cnt)), scene._lib)
    return out


def render_stats(scene):
    """render's cache counters on this scene: device-scene creations, film buffer allocations, renders."""
    a, b, c = u64(), u64(), u64()
    _check(scene._lib.amvpt_host_render_stats(scene._h, a, b, c), scene._lib)
    return {"scene_creates": a.value, "buffer_allocs": b.value, "renders": c.value}


def render_multi(scene, devices, sensor=0, seed=0, spp=0, raw=False, counters=None):
    """Integrator::render over several GPUs of this node (C++ threads, lane shards, one RCCL reduce of
    the RGBW ImageBlocks onto devices[0]; amvpt_host_render_multi) -> numpy (H, W, C)."""
    w, h, c, _ = scene.film_info(sensor)
    _, _, p = scene.describe(sensor, seed, spp)
    ch = (5 if p.film_alpha else 4) if raw else c
    out = np.zeros((h, w, ch), dtype=np.float32)
    cnt = counters if counters is not None else Counters()
    devs = (ctypes.c_int * len(devices))(*devices)
    _check(scene._lib.amvpt_host_render_multi(scene._h, sensor, seed, spp, 1 if raw else 0, devs, len(devices),
                                              out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(cnt)), scene._lib)
    return out


def host_lane_shard(n_lanes, rank, world):
    """The C++ host's lane partition (amvpt_host_lane_shard), for checks against dist.lane_shard."""
    b, e = u64(), u64()
    host_lib().amvpt_host_lane_shard(n_lanes, rank, world, ctypes.byref(b), ctypes.byref(e))
    return b.value, e.value


def host_view_group_partition(params, rank, world):
    """The C++ host's view-group partition (amvpt_host_view_group_partition): (rect, window) or None."""
    r, w = (u32 * 4)(), (u32 * 4)()
    ok = host_lib().amvpt_host_view_group_partition(ctypes.byref(params), rank, world, r, w)
    return (tuple(r), tuple(w)) if ok else None


def multi_stats(scene):
    """render_multi's cache counters on this scene: scene creations, communicator inits, renders."""
    a, b, c = u64(), u64(), u64()
    _check(scene._lib.amvpt_host_multi_stats(scene._h, a, b, c), scene._lib)
    return {"scene_creates": a.value, "comm_inits": b.value, "renders": c.value}


def plan(params):
    L = hip_lib()
    spp, spl, npass, lanes = u32(), u32(), u32(), u64()
    _check(L.amvpt_plan(ctypes.byref(params), spp, spl, npass, lanes), L)
    return spp.value, spl.value, npass.value, lanes.value


# process-wide defaults of the legacy setters, also the defaults of render_ex's per-call options
_DEFAULTS = {"chunk_lanes": 0, "traversal": 0}


def set_traversal(mode):
    """BVH walk: 0 auto (brute force for tiny scenes), 1 wave-uniform, 2 per-lane (amvpt_set_traversal)."""
    L = hip_lib()
    _check(L.amvpt_set_traversal(u32(mode)), L)
    _DEFAULTS["traversal"] = int(mode)


def set_bvh_build(max_leaf_prims=4, traversal_cost=0.0):
    """SAH shape of later DeviceScene builds (amvpt_set_bvh_build)."""
    L = hip_lib()
    _check(L.amvpt_set_bvh_build(u32(max_leaf_prims), ctypes.c_float(traversal_cost)), L)


def set_chunk_lanes(n):
    L = hip_lib()
    _check(L.amvpt_set_chunk_lanes(u64(n)), L)
    _DEFAULTS["chunk_lanes"] = int(n)


# amvpt_exchange_fn: (ctx, local_count, *prefix, *total) -> 0 on success
ExchangeFn = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, u64, ctypes.POINTER(u64), ctypes.POINTER(u64))
_exchange_cb = None


def wrap_exchange(fn):
    """ctypes callback around `fn(local_count) -> (prefix, total)` (exceptions -> status 1)."""
    def cb(_ctx, local, prefix, total):
        try:
            pre, tot = fn(int(local))
            prefix[0], total[0] = int(pre), int(tot)
            return 0
        except Exception:   # noqa: BLE001 -- reported to the C side as a failed exchange
            return 1
    return ExchangeFn(cb)


def set_adaptive_exchange(fn):
    """Count exchange for adaptive renders over lane ranges (amvpt_set_adaptive_exchange).

    `fn(local_count) -> (prefix, total)`: flagged lanes in lower ranges and in the
    whole pass (see amvpt.dist.count_exchange); None clears it."""
    global _exchange_cb
    L = hip_lib()
    _exchange_cb = wrap_exchange(fn) if fn is not None else None
    _check(L.amvpt_set_adaptive_exchange(_exchange_cb if _exchange_cb else ExchangeFn(), None), L)


def scene_box_count(scene, sensor=0):
    """Box meshes amvpt_scene_create screens in the brute-force walks of `scene` (amvpt_scene_desc_boxes)."""
    L = hip_lib()
    sd, _, _ = scene.describe(sensor, 0, 0)
    L.amvpt_scene_desc_boxes.argtypes = [ctypes.c_void_p, ctypes.POINTER(u32)]
    n = u32()
    _check(L.amvpt_scene_desc_boxes(ctypes.cast(sd, ctypes.c_void_p), ctypes.byref(n)), L)
    return n.value


def release_device_memory(device=0):
    """Free the lane arena renders keep on `device` between frames (amvpt_release_device_memory, ABI 10)."""
    L = hip_lib()
    _check(L.amvpt_release_device_memory(int(device)), L)


def device_count():
    n = ctypes.c_int(0)
    hip_lib().amvpt_device_count(ctypes.byref(n))
    return n.value


def write_exr(path, img):
    img = np.ascontiguousarray(img, dtype=np.float32)
    h, w, c = img.shape
    L = host_lib()
    _check(L.amvpt_host_write_exr(path.encode(), img.ctypes.data_as(ctypes.c_void_p), w, h, c), L)


def read_exr(path, width, height, channels):
    out = np.zeros((height, width, channels), dtype=np.float32)
    L = host_lib()
    _check(L.amvpt_host_read_exr(path.encode(), out.ctypes.data_as(ctypes.c_void_p), width, height, channels), L)
    return out


def _name_array(names):
    enc = [str(n).encode() for n in names]
    return (ctypes.c_char_p * max(1, len(enc)))(*enc), len(enc)


def write_exr_channels(path, data, names):
    """(H, W, C) float32 -> an OpenEXR file with one float32 channel per name (amvpt_host_write_exr_channels).
    Names are 1 to 31 bytes and unique; the file stores the channels in the byte order of their names."""
    img = np.ascontiguousarray(data, dtype=np.float32)
    if img.ndim != 3:
        raise ValueError("write_exr_channels: an (H, W, C) array is needed")
    h, w, c = img.shape
    arr, n = _name_array(names)
    if n != c:
        raise ValueError("write_exr_channels: %d names for %d channels" % (n, c))
    L = host_lib()
    _check(L.amvpt_host_write_exr_channels(str(path).encode(), img.ctypes.data_as(ctypes.c_void_p), w, h, c, arr), L)


def read_exr_channels(path, width, height, names):
    """The named float32 channels of a file write_exr_channels wrote -> (height, width, len(names)), in the order
    of `names` (amvpt_host_read_exr_channels)."""
    arr, n = _name_array(names)
    out = np.zeros((height, width, n), dtype=np.float32)
    L = host_lib()
    _check(L.amvpt_host_read_exr_channels(str(path).encode(), out.ctypes.data_as(ctypes.c_void_p), width, height, n,
                                          arr), L)
    return out


def _host_guides(scene, sensor, want_guides, want_depth):
    w, h, _, _ = scene.film_info(sensor)
    g = np.zeros((h, w, 8), dtype=np.float32) if want_guides else None
    z = np.zeros((h, w), dtype=np.float32) if want_depth else None
    _check(scene._lib.amvpt_host_guides(scene._h, sensor, g.ctypes.data if g is not None else None,
                                        z.ctypes.data if z is not None else None), scene._lib)
    return g, z


def guides(scene, sensor=0):
    """Guide records of every quilt pixel -> (H, W, 8) float32: shape index (-1: miss), geometric normal, hit
    point, view index, through the pixel centre (amvpt_host_guides; on the device scene render() caches)."""
    return _host_guides(scene, sensor, True, False)[0]


def depth(scene, sensor=0):
    """Planar depth of every quilt pixel -> (H, W) float32: the camera-space z of the primary hit in the pixel's
    own view, +inf on a miss (amvpt_host_guides)."""
    return _host_guides(scene, sensor, False, True)[1]


def denoise_params_for(scene, sensor=0, params=None, **fields):
    """The DenoiseParams `denoise` uses: `params` as given, or the defaults with the given fields replaced and, where
    sigma_plane is not among them, denoise_sigma_plane of the scene's guide records."""
    if params is not None:
        if fields:
            raise ValueError("denoise: give either params or single fields, not both")
        return params
    q = DenoiseParams(**fields)
    if "sigma_plane" not in fields:
        q.sigma_plane = denoise_sigma_plane(guides(scene, sensor))
    return q


def host_denoise(scene, params, image=None, sensor=0, replace=False, download=True, stream=None):
    """amvpt_host_denoise_stream: amvpt_denoise on the device over `image` (None: the developed frame the last render
    or display of this sensor cached there) and the guide records of the cached device scene -> the filtered image
    (None with download=False).  replace=True makes it the cached frame, which display(rerender=False) then shows."""
    w, h, c, _ = scene.film_info(sensor)
    img = None
    if image is not None:
        img = np.ascontiguousarray(image, dtype=np.float32)
        if img.shape != (h, w, c):
            raise ValueError("denoise: the image must be (%d, %d, %d), the sensor's developed frame" % (h, w, c))
    out = np.zeros((h, w, c), dtype=np.float32) if download else None
    _check(scene._lib.amvpt_host_denoise_stream(scene._h, sensor, ctypes.byref(params),
                                                img.ctypes.data if img is not None else None, int(bool(replace)),
                                                out.ctypes.data if out is not None else None,
                                                ctypes.c_void_p(stream or 0)), scene._lib)
    return out


def denoise(scene, image=None, sensor=0, seed=0, spp=0, params=None, stream=None, **fields):
    """The a-trous denoiser (include/amvpt_denoise.h) on the device: `image` (None: a fresh render of `sensor` with
    `seed` and `spp`, developed) filtered with the scene's guide records -> (H, W, C) float32.  `params` is a
    DenoiseParams; otherwise its fields are keywords (iterations, sigma_color, color_floor, sigma_plane,
    normal_squarings) over the defaults, with sigma_plane from denoise_sigma_plane of the scene."""
    q = denoise_params_for(scene, sensor, params, **fields)
    if image is None:
        render(scene, sensor=sensor, seed=seed, spp=spp, stream=stream)
    return host_denoise(scene, q, image=image, sensor=sensor, stream=stream)


GUIDE_CHANNELS = ("Z", "N.X", "N.Y", "N.Z", "P.X", "P.Y", "P.Z", "id", "view")


def write_guides_exr(path, image, guides, depth):
    """One OpenEXR file with the developed image (H, W, 3 or 4) and its guide buffers: channels R, G, B[, A], Z,
    N.X, N.Y, N.Z, P.X, P.Y, P.Z, id, view.  id = shape index + 1 with 0 the background, the convention of the
    reference's `shape_index` AOV (aov.cpp:231-235)."""
    img = np.asarray(image, dtype=np.float32)
    g = np.asarray(guides, dtype=np.float32)
    z = np.asarray(depth, dtype=np.float32)
    if img.ndim != 3 or img.shape[2] not in (3, 4):
        raise ValueError("write_guides_exr: an (H, W, 3 or 4) image is needed")
    if g.shape != img.shape[:2] + (8,) or z.shape != img.shape[:2]:
        raise ValueError("write_guides_exr: guides must be (H, W, 8) and depth (H, W) of the image's size")
    planes = np.concatenate([img, z[..., None], g[..., 1:7], g[..., 0:1] + np.float32(1.0), g[..., 7:8]], axis=2)
    write_exr_channels(path, planes, ("R", "G", "B", "A")[:img.shape[2]] + GUIDE_CHANNELS)


def parse_fov(fov=0.0, fov_axis=None, focal_length=None, aspect=1.0):
    L = host_lib()
    r = L.amvpt_host_parse_fov(float(fov), fov_axis.encode() if fov_axis else None,
                               focal_length.encode() if focal_length else None, float(aspect))
    if r < 0:
        raise RuntimeError(L.amvpt_host_last_error().decode())
    return r


def perspective_projection(film_size, crop_size, crop_offset, fov_x, near_clip, far_clip):
    L = host_lib()
    I3 = ctypes.c_int * 2
    m = (f32 * 16)()
    L.amvpt_host_perspective_projection(I3(*film_size), I3(*crop_size), I3(*crop_offset), fov_x, near_clip,
                                        far_clip, m)
    return np.array(m[:], dtype=np.float32).reshape(4, 4)


class DeviceScene:
    """Direct handle on the C-ABI: amvpt_scene_create over host descriptors (bench / tests)."""

    def __init__(self, scene_desc_ptr):
        self._lib = hip_lib()
        h = ctypes.c_void_p()
        _check(self._lib.amvpt_scene_create(scene_desc_ptr, ctypes.byref(h)), self._lib)
        self.h = h

    def stats(self):
        n, p = u32(), u32()
        _check(self._lib.amvpt_scene_stats(self.h, n, p), self._lib)
        return n.value, p.value

    def bvh2(self):
        """(two-box BVH nodes, tree depth in inner nodes) -- amvpt_scene_bvh2 (0 nodes: threaded walks)"""
        n, d = u32(), u32()
        self._lib.amvpt_scene_bvh2.argtypes = [ctypes.c_void_p, ctypes.POINTER(u32), ctypes.POINTER(u32)]
        _check(self._lib.amvpt_scene_bvh2(self.h, n, d), self._lib)
        return n.value, d.value

    def render(self, views_ptr, params, film_ptr, lane_begin=0, lane_end=2 ** 64 - 1, stream=None,
               counters=None):
        """amvpt_render over lanes [lane_begin, lane_end).  Without `counters` the render is not
        instrumented (no per-kernel event timing, no host synchronisation); with an amvpt.Counters
        it is filled (per-kernel HIP-event times, lane statistics) and returned."""
        _check(self._lib.amvpt_render(self.h, views_ptr, ctypes.byref(params), lane_begin, lane_end,
                                      ctypes.c_void_p(film_ptr), ctypes.c_void_p(stream),
                                      ctypes.byref(counters) if counters is not None else None),
               self._lib)
        return counters

    def render_ex(self, views_ptr, params, film_ptr, lanes=None, window=None, overflow_ptr=None,
                  overflow_capacity=0, stream=None, counters=None, chunk_lanes=None, traversal=None, flags=0,
                  exchange=None, records_ptr=None, record_pass=0, budget_mib=0):
        """amvpt_render_ex: `lanes` a LaneSet (None: the whole pass), `window` (x0, y0, width, height)
        of the quilt the film holds (None: the whole quilt), per-call options; `exchange` is
        `fn(run_lane_begin, run_count) -> (run_prefix, total)` (see amvpt.dist.run_exchange)."""
        if lanes is None:
            lanes = LaneSet(0, 2 ** 64 - 1, 0, 0, 0, 0)
        chunk_lanes = _DEFAULTS["chunk_lanes"] if chunk_lanes is None else chunk_lanes
        traversal = _DEFAULTS["traversal"] if traversal is None else traversal
        x0, y0, w, h = window if window is not None else (0, 0, params.film_width, params.film_height)
        fw = FilmWindow(ctypes.c_void_p(film_ptr), x0, y0, w, h, ctypes.c_void_p(overflow_ptr or 0),
                        overflow_capacity)
        cb = wrap_run_exchange(exchange) if exchange is not None else RunExchangeFn()
        o = RenderOpts(chunk_lanes, traversal, flags, cb, None, ctypes.c_void_p(records_ptr or 0), record_pass,
                       int(budget_mib))
        _check(self._lib.amvpt_render_ex(self.h, views_ptr, ctypes.byref(params), ctypes.byref(lanes),
                                         ctypes.byref(fw), ctypes.c_void_p(stream), ctypes.byref(o),
                                         ctypes.byref(counters) if counters is not None else None), self._lib)
        return counters

    def render_fixed(self, views_ptr, params, fixed_ptr, lanes=None, window=None, overflow_ptr=None,
                     overflow_capacity=0, stream=None, counters=None, chunk_lanes=None, traversal=None, flags=0,
                     exchange=None, records_ptr=None, record_pass=0, budget_mib=0):
        """amvpt_render_fixed: render_ex into the caller's int64 fixed-point window at `fixed_ptr` (accumulated
        into: neither cleared nor resolved) with an int64 overflow list (2 header words, 2 words per entry)."""
        if lanes is None:
            lanes = LaneSet(0, 2 ** 64 - 1, 0, 0, 0, 0)
        chunk_lanes = _DEFAULTS["chunk_lanes"] if chunk_lanes is None else chunk_lanes
        traversal = _DEFAULTS["traversal"] if traversal is None else traversal
        x0, y0, w, h = window if window is not None else (0, 0, params.film_width, params.film_height)
        fw = FixedWindow(ctypes.c_void_p(fixed_ptr), x0, y0, w, h, ctypes.c_void_p(overflow_ptr or 0),
                         overflow_capacity)
        cb = wrap_run_exchange(exchange) if exchange is not None else RunExchangeFn()
        o = RenderOpts(chunk_lanes, traversal, flags, cb, None, ctypes.c_void_p(records_ptr or 0), record_pass,
                       int(budget_mib))
        _check(self._lib.amvpt_render_fixed(self.h, views_ptr, ctypes.byref(params), ctypes.byref(lanes),
                                            ctypes.byref(fw), ctypes.c_void_p(stream), ctypes.byref(o),
                                            ctypes.byref(counters) if counters is not None else None), self._lib)
        return counters

    def render_records(self, views_ptr, params, film_ptr, records_ptr, pass_index=0, lane_begin=0,
                       lane_end=2 ** 64 - 1, stream=None):
        _check(self._lib.amvpt_render_records(self.h, views_ptr, ctypes.byref(params), pass_index, lane_begin,
                                              lane_end, ctypes.c_void_p(film_ptr), ctypes.c_void_p(records_ptr),
                                              ctypes.c_void_p(stream)), self._lib)

    def guides(self, views_ptr, params, out_ptr, rect=None, stream=None):
        """amvpt_guides: the guide record (shape index or -1, geometric normal, hit point, view index; 8 float32)
        of every pixel of `rect` = (x0, y0, w, h) of the quilt crop (None: all of it) into the device buffer at
        `out_ptr` (h * w * 8 floats, 16-byte aligned), ordered on `stream`."""
        r = ctypes.byref((u32 * 4)(*[int(v) for v in rect])) if rect is not None else None
        _check(self._lib.amvpt_guides(self.h, views_ptr, ctypes.byref(params), r, ctypes.c_void_p(out_ptr or 0),
                                      ctypes.c_void_p(stream or 0)), self._lib)

    def __del__(self):
        if getattr(self, "h", None):
            self._lib.amvpt_scene_destroy(self.h)
            self.h = None


class TemporalAccumulator:
    """Temporal accumulation over a sequence of frames (include/amvpt_temporal.h).  It owns two sets of the three
    planes (accumulated image, guide records, history count) as torch device tensors and the views of the last frame;
    `push` takes the current developed frame, runs amvpt_guides and amvpt_temporal on the device and swaps the sets.
    A change of film size, channel count or n_views starts over, as `reset` does.
    moments=True keeps a fourth plane, the two luminance moments of include/amvpt_variance.h, and accumulates through
    amvpt_temporal_moments (image and count are the same bits either way); `variance` and `denoise` then run the
    other two stages of that header over the accumulator's own tensors."""

    def __init__(self, params=None, moments=False):
        self.params = params if params is not None else temporal_default_params()
        self.with_moments = bool(moments)
        self._scene = None   # (Scene, DeviceScene) of device_scene_for
        self.reset()

    def device_scene_for(self, scene, scene_desc):
        """The DeviceScene this accumulator keeps for the loaded `scene` (amvpt.display.display(..., temporal=)):
        created from `scene_desc` at the first call; another scene replaces it and forgets the history.  reset()
        keeps it: the geometry does not change with the history."""
        if self._scene is None or self._scene[0] is not scene:
            self._scene = (scene, DeviceScene(scene_desc))
            self.reset()
        return self._scene[1]

    def reset(self):
        """Forget the history: the next push returns its frame unchanged, with count 1."""
        self._key = None
        self._sets = None
        self._cur = 0
        self.prev_views = None
        self.frames = 0

    @property
    def image(self):
        """The accumulated image of the last push, (H, W, C) on the device (None before the first)."""
        return self._sets[self._cur][0] if self._sets and self.frames else None

    @property
    def guides(self):
        """The guide records of the last push, (H, W, 8) on the device."""
        return self._sets[self._cur][1] if self._sets and self.frames else None

    @property
    def count(self):
        """The history count of the last push, (H, W) on the device."""
        return self._sets[self._cur][2] if self._sets and self.frames else None

    @property
    def moments(self):
        """The luminance moments of the last push, (H, W, 2) on the device (None without moments=True)."""
        return self._sets[self._cur][3] if self._sets and self.frames and self.with_moments else None

    def _stream(self, stream):
        import torch
        return torch.cuda.current_stream() if not stream else torch.cuda.ExternalStream(int(stream))

    def variance(self, params=None, stream=None):
        """amvpt_variance over the planes of the last push -> the (H, W) variance of the accumulated luminance, a new
        device tensor.  `params` is a VarianceParams (None: the defaults)."""
        if self.moments is None:
            raise ValueError("TemporalAccumulator.variance: needs moments=True and a pushed frame")
        import torch
        h, w = self.count.shape
        st = self._stream(stream)
        with torch.cuda.stream(st):
            var = torch.empty((h, w), dtype=torch.float32, device="cuda")
            variance_device(self.moments.data_ptr(), self.count.data_ptr(), self.guides.data_ptr(), w, h, var.data_ptr(),
                            params=params, stream=st.cuda_stream)
        return var

    def denoise(self, params=None, stream=None):
        """amvpt_variance and amvpt_denoise_variance over the planes of the last push -> (filtered image, filtered
        variance), new device tensors; the history is not touched."""
        import torch
        q = params if params is not None else variance_default_params()
        var = self.variance(q, stream=stream)
        img = self.image
        h, w, c = img.shape
        st = self._stream(stream)
        with torch.cuda.stream(st):
            out, scratch = torch.empty_like(img), torch.empty_like(img)
            vout, vscratch = torch.empty_like(var), torch.empty_like(var)
            denoise_variance_device(img.data_ptr(), c, w, h, var.data_ptr(), self.guides.data_ptr(), out.data_ptr(),
                                    scratch.data_ptr(), vout.data_ptr(), vscratch.data_ptr(), params=q, stream=st.cuda_stream)
        return out, vout

    def push(self, device_scene, views, params, image, stream=None):
        """Accumulate one frame: `image` is the developed frame of `params`' film on the device, a torch tensor
        (H, W, 3 or 4) or a device pointer (then 4 channels with film_alpha, else 3); `views` the host ViewDesc table
        it was rendered with.  Work is ordered on `stream` (a hipStream_t handle; None: torch's current stream).
        Returns the accumulated image, a tensor this accumulator owns: it is the history of the next push and is
        overwritten by the one after."""
        import torch
        h, w = int(params.film_height), int(params.film_width)
        if hasattr(image, "data_ptr"):
            if image.dtype != torch.float32 or not image.is_contiguous() or tuple(image.shape[:2]) != (h, w) or image.dim() != 3:
                raise ValueError("TemporalAccumulator.push: a contiguous float32 (%d, %d, C) tensor is needed" % (h, w))
            c, ptr = int(image.shape[2]), image.data_ptr()
        else:
            c, ptr = (4 if params.film_alpha else 3), int(image)
        n_views = max(1, int(params.n_views)) if params.multisensor else 1
        st = torch.cuda.current_stream() if not stream else torch.cuda.ExternalStream(int(stream))
        with torch.cuda.stream(st):
            key = (h, w, c, n_views)
            if key != self._key:
                self.reset()
                self._key = key
                self._sets = [(torch.zeros((h, w, c), dtype=torch.float32, device="cuda"),
                               torch.zeros((h, w, 8), dtype=torch.float32, device="cuda"),
                               torch.zeros((h, w), dtype=torch.float32, device="cuda")) +
                              ((torch.zeros((h, w, 2), dtype=torch.float32, device="cuda"),) if self.with_moments else ())
                              for _ in range(2)]
            hist = self._sets[self._cur]
            cur = self._sets[1 - self._cur]
            if self.prev_views is None:   # no history: its count is zero, any valid view table serves
                hist[2].zero_()
                prev = views
            else:
                prev = self.prev_views
            device_scene.guides(views, params, cur[1].data_ptr(), stream=st.cuda_stream)
            if self.with_moments:
                temporal_moments_device(ptr, c, cur[1].data_ptr(), hist[0].data_ptr(), hist[1].data_ptr(), hist[2].data_ptr(),
                                        hist[3].data_ptr(), prev, params, cur[0].data_ptr(), cur[2].data_ptr(),
                                        cur[3].data_ptr(), tp=self.params, stream=st.cuda_stream)
            else:
                temporal_device(ptr, c, cur[1].data_ptr(), hist[0].data_ptr(), hist[1].data_ptr(), hist[2].data_ptr(), prev,
                                params, cur[0].data_ptr(), cur[2].data_ptr(), tp=self.params, stream=st.cuda_stream)
        keep = (ViewDesc * n_views)()
        ctypes.memmove(keep, views, ctypes.sizeof(keep))
        self.prev_views = keep
        self._cur = 1 - self._cur
        self.frames += 1
        return cur[0]


class ViewSynthesizer:
    """View synthesis into the dense quilt of `dst_scene` (include/amvpt_synth.h): a host Scene of the same XML as the
    rendered one, loaded with the dense grid.  It keeps the target views, the target Params and, as a torch device
    tensor, the target guide records, computed with DeviceScene.guides at the first `run` and again only when the bytes
    of the target views change (`guide_runs` counts).  `holes` is the number of pixels whose cover is 0 after the last
    run, whose planes stay reachable as `source_image`, `source_guides`, `image` and `cover`."""

    def __init__(self, dst_scene, params=None, sensor=0):
        self.params = params if params is not None else synth_default_params()
        self.scene, self.sensor = dst_scene, sensor
        self.guides = None
        self.guide_runs = 0
        self._guides_key = None
        self.holes = None
        self.source_image = self.source_guides = self.image = self.cover = None   # the planes of the last run
        self._device = None   # (Scene, DeviceScene) of device_scene_for
        self.set_views(*dst_scene.describe(sensor, 0, 0)[1:])

    def set_views(self, views, params):
        """The target views (a host ViewDesc table) and the Params of the target quilt; copies are kept."""
        self.dst_params = Params.from_buffer_copy(params)
        n = max(1, int(params.n_views)) if params.multisensor else 1
        keep = (ViewDesc * n)()
        ctypes.memmove(keep, views, ctypes.sizeof(keep))
        self.dst_views = keep

    def device_scene_for(self, scene, scene_desc):
        """The DeviceScene this synthesizer keeps for the loaded `scene` (amvpt.display.display(..., synth=) without an
        accumulator): created from `scene_desc` at the first call, replaced by another scene's."""
        if self._device is None or self._device[0] is not scene:
            self._device = (scene, DeviceScene(scene_desc))
        return self._device[1]

    def run(self, device_scene, src_views, src_params, src_image, src_guides=None, stream=None):
        """Synthesize the target quilt from the developed source quilt `src_image`, a contiguous float32 (Hs, Ws, 3 or
        4) torch device tensor rendered with `src_views` / `src_params`; `src_guides` its (Hs, Ws, 8) guide records
        (None: computed here with device_scene.guides).  Stage 1, then params.fill_iterations of stage 2, ordered on
        `stream` (a hipStream_t handle; None: torch's current stream) -> (image (h, w, C), cover (h, w)), new tensors."""
        import torch
        hs, ws = int(src_params.film_height), int(src_params.film_width)
        if (not hasattr(src_image, "data_ptr") or src_image.dtype != torch.float32 or not src_image.is_contiguous()
                or src_image.dim() != 3 or tuple(src_image.shape[:2]) != (hs, ws)):
            raise ValueError("ViewSynthesizer.run: a contiguous float32 (%d, %d, C) tensor is needed" % (hs, ws))
        c = int(src_image.shape[2])
        p = self.dst_params
        h, w = int(p.film_height), int(p.film_width)
        st = torch.cuda.current_stream() if not stream else torch.cuda.ExternalStream(int(stream))
        with torch.cuda.stream(st):
            key = bytes(self.dst_views) + bytes(p)
            if self.guides is None or key != self._guides_key:
                self.guides = torch.empty((h, w, 8), dtype=torch.float32, device="cuda")
                device_scene.guides(self.dst_views, p, self.guides.data_ptr(), stream=st.cuda_stream)
                self._guides_key = key
                self.guide_runs += 1
            if src_guides is None:
                src_guides = torch.empty((hs, ws, 8), dtype=torch.float32, device="cuda")
                device_scene.guides(src_views, src_params, src_guides.data_ptr(), stream=st.cuda_stream)
            elif tuple(src_guides.shape) != (hs, ws, 8) or src_guides.dtype != torch.float32 or not src_guides.is_contiguous():
                raise ValueError("ViewSynthesizer.run: src_guides must be a contiguous float32 (%d, %d, 8) tensor" % (hs, ws))
            img = torch.empty((h, w, c), dtype=torch.float32, device="cuda")
            cover = torch.empty((h, w), dtype=torch.float32, device="cuda")
            synth_device(src_image.data_ptr(), c, src_guides.data_ptr(), src_views, src_params, self.guides.data_ptr(),
                         self.dst_views, p, img.data_ptr(), cover.data_ptr(), sp=self.params, stream=st.cuda_stream)
            if self.params.fill_iterations:
                out, cout = torch.empty_like(img), torch.empty_like(cover)
                many = self.params.fill_iterations > 1
                scratch, cscratch = (torch.empty_like(img), torch.empty_like(cover)) if many else (None, None)
                synth_fill_device(img.data_ptr(), c, w, h, cover.data_ptr(), self.guides.data_ptr(), out.data_ptr(),
                                  cout.data_ptr(), scratch.data_ptr() if many else None, cscratch.data_ptr() if many else None,
                                  sp=self.params, stream=st.cuda_stream)
                img, cover = out, cout
            self.holes = int((cover == 0).sum().item())
        self.source_image, self.source_guides, self.image, self.cover = src_image, src_guides, img, cover
        return img, cover


class ToneMapper:
    """The tone-mapping stage over torch device tensors (include/amvpt_tonemap.h).  It owns the amvpt_tonemap_state in
    device memory; with params.auto_exposure set, `run` and `run_float` meter the frame into it first, and the exposure
    adapts from call to call.  Nothing returns to the host between metering and tone mapping.  The input of the last
    run stays reachable as `frame`."""

    def __init__(self, params=None):
        self.params = params if params is not None else tonemap_default_params()
        self._state = None
        self.frame = None     # the input of the last run, which stays reachable
        self._device = None   # (Scene, DeviceScene) of device_scene_for

    def device_scene_for(self, scene, scene_desc):
        """The DeviceScene this tone mapper keeps for the loaded `scene` (amvpt.display.display(..., tonemap=) with
        neither an accumulator nor a synthesizer): created from `scene_desc` at the first call."""
        if self._device is None or self._device[0] is not scene:
            self._device = (scene, DeviceScene(scene_desc))
        return self._device[1]

    def _state_tensor(self):
        import torch
        if self._state is None:
            self._state = torch.zeros(ctypes.sizeof(TonemapState), dtype=torch.uint8, device="cuda")
        return self._state

    def reset(self):
        """Return the state to a fresh one: the next metered frame sets the exposure without adaptation."""
        if self._state is not None:
            self._state.zero_()

    def state(self):
        """The state struct, downloaded (synchronises with the work issued so far)."""
        return TonemapState.from_buffer_copy(self._state_tensor().cpu().numpy().tobytes())

    def _frame(self, who, frame):
        import torch
        if (not hasattr(frame, "data_ptr") or frame.dtype != torch.float32 or not frame.is_contiguous() or frame.dim() != 3):
            raise ValueError("ToneMapper.%s: a contiguous float32 (H, W, C) device tensor is needed" % who)
        return int(frame.shape[0]), int(frame.shape[1]), int(frame.shape[2])

    def _run(self, who, frame, stream, rect, out_of, entry):
        import torch
        h, w, c = self._frame(who, frame)
        st = torch.cuda.current_stream() if not stream else torch.cuda.ExternalStream(int(stream))
        with torch.cuda.stream(st):
            state = self._state_tensor().data_ptr() if self.params.auto_exposure else None
            if state is not None:
                tonemap_meter_device(frame.data_ptr(), c, w, h, state, self.params, rect=rect, stream=st.cuda_stream)
            out = out_of(h, w, c)
            entry(frame.data_ptr(), c, w, h, out.data_ptr(), self.params, state_ptr=state, stream=st.cuda_stream)
        self.frame = frame
        return out

    def run(self, frame, stream=None, rect=None):
        """Meter `frame` (with auto_exposure; `rect` = (x0, y0, w, h) restricts the metering) and map it to 8-bit sRGB
        (amvpt_tonemap_srgb8), ordered on `stream` (a hipStream_t handle; None: torch's current stream) -> a new
        (H, W, 3) uint8 device tensor."""
        import torch
        return self._run("run", frame, stream, rect,
                         lambda h, w, c: torch.empty((h, w, 3), dtype=torch.uint8, device="cuda"), tonemap_srgb8_device)

    def run_float(self, frame, stream=None, rect=None):
        """`run` with float output (amvpt_tonemap_apply) -> a new (H, W, C) float32 device tensor."""
        import torch
        return self._run("run_float", frame, stream, rect, lambda h, w, c: torch.empty_like(frame), tonemap_device)

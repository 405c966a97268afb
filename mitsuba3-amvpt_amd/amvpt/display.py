"""
amvpt.display -- the display stage: the developed quilt as 8-bit sRGB and the quilt interlaced into the
native image of a lenticular light-field display (include/amvpt_display.h; the reference's front end,
src/mitsuba/program.cpp:199-276 with the presets of src/mitsuba/preset.h).

`srgb8`, `interlace` and `views` run the host entries over numpy arrays and need no device;
`srgb8_device` / `interlace_device` launch the kernels over device pointers; `display` renders a scene and
runs the whole stage on the device, downloading the display image once (with `tonemap=` an amvpt.ToneMapper,
include/amvpt_tonemap.h, stands where the sRGB conversion does).  `depth_quilt` is the 8-bit depth
quilt of a scene (include/amvpt_guides.h), the RGB-D companion of the sRGB quilt.
"""
import ctypes

import numpy as np

import amvpt
from amvpt import Counters, f32, i32, u32

ERR_INVALID = 1


class Preset(ctypes.Structure):
    """amvpt_display_preset: a lenticular display's calibration (Preset, preset.h:12-17)."""
    _fields_ = [("center", f32), ("focus", f32), ("pitch", f32), ("tilt", f32), ("subp", f32),
                ("view", f32 * 2), ("grid", i32 * 2), ("flip_rgb", u32)]

    def __init__(self, center=-0.5, focus=-0.05, pitch=354.548, tilt=-0.114, subp=0.00013, view=(1.0, 1.0),
                 grid=(4, 8), flip_rgb=False, name="LKG4x8"):
        super().__init__(center, focus, pitch, tilt, subp, (f32 * 2)(*view), (i32 * 2)(*grid), 1 if flip_rgb else 0)
        self.name = name

    def values(self):
        """The fields as a tuple of Python numbers (floats as the float32 values the library sees)."""
        return (self.center, self.focus, self.pitch, self.tilt, self.subp, tuple(self.view), tuple(self.grid),
                bool(self.flip_rgb))

    def __eq__(self, other):
        return isinstance(other, Preset) and self.values() == other.values() and self.name == other.name

    def __repr__(self):
        return "Preset(name=%r, center=%r, focus=%r, pitch=%r, tilt=%r, subp=%r, view=%r, grid=%r, flip_rgb=%r)" % (
            (self.name,) + self.values())

    @classmethod
    def _from_c(cls, c, name="LKG4x8"):
        return cls(c.center, c.focus, c.pitch, c.tilt, c.subp, tuple(c.view), tuple(c.grid), bool(c.flip_rgb), name)


class _NamedPreset(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 64), ("preset", Preset)]


_bound = False


def _libs():
    global _bound
    L, H = amvpt.hip_lib(), amvpt.host_lib()
    if not _bound:
        vp, cp = ctypes.c_void_p, ctypes.c_int
        pp = ctypes.POINTER(Preset)
        L.amvpt_display_version.restype = u32
        L.amvpt_display_default_preset.restype = Preset
        L.amvpt_display_default_preset.argtypes = []
        for fn, args in (("amvpt_srgb8", [vp, u32, u32, u32, vp, vp]),
                         ("amvpt_srgb8_host", [vp, u32, u32, u32, vp]),
                         ("amvpt_interlace", [vp, u32, u32, u32, pp, cp, cp, vp, u32, u32, vp]),
                         ("amvpt_interlace_host", [vp, u32, u32, u32, pp, cp, cp, vp, u32, u32]),
                         ("amvpt_interlace_views_host", [pp, vp, u32, u32])):
            getattr(L, fn).restype = cp
            getattr(L, fn).argtypes = args
        H.amvpt_host_display.argtypes = [vp, u32, u32, u32, pp, cp, cp, u32, u32, vp, ctypes.POINTER(Counters)]
        H.amvpt_host_display_stream.argtypes = [vp, u32, u32, u32, pp, cp, cp, u32, u32, vp, vp,
                                                ctypes.POINTER(Counters)]
        H.amvpt_host_redisplay_stream.argtypes = [vp, u32, pp, cp, cp, u32, u32, vp, vp]
        H.amvpt_host_preset_for_scene.argtypes = [vp, u32, pp]
        H.amvpt_host_read_presets.argtypes = [ctypes.c_char_p, vp, u32, ctypes.POINTER(u32)]
        H.amvpt_host_write_presets.argtypes = [ctypes.c_char_p, vp, u32]
        H.amvpt_host_write_png.argtypes = [ctypes.c_char_p, vp, u32, u32]
        _bound = True
    return L, H


def _check_hip(rc, L):
    if rc != 0:
        raise RuntimeError(L.amvpt_last_error().decode())


def version():
    return _libs()[0].amvpt_display_version()


def default_preset():
    """The reference's LKG4x8 (amvpt_display_default_preset)."""
    return Preset._from_c(_libs()[0].amvpt_display_default_preset())


def srgb8(image):
    """Developed float32 image (H, W, 3 or 4) -> (H, W, 3) uint8 sRGB; alpha is dropped (amvpt_srgb8_host)."""
    L, _ = _libs()
    img = np.ascontiguousarray(image, dtype=np.float32)
    if img.ndim != 3:
        raise ValueError("srgb8: an (H, W, C) image is needed")
    h, w, c = img.shape
    out = np.empty((h, w, 3), dtype=np.uint8)
    _check_hip(L.amvpt_srgb8_host(img.ctypes.data, c, w, h, out.ctypes.data), L)
    return out


def _src_u8(src):
    s = np.ascontiguousarray(src)
    if s.dtype != np.uint8 or s.ndim != 3:
        raise ValueError("interlace: an (H, W, C) uint8 quilt is needed")
    return s


def interlace(src, preset=None, size=(1280, 720), quilt=False, nearest=False):
    """8-bit quilt (H, W, 3 or 4) -> the (size[1], size[0], 3) uint8 lenticular image of `preset`
    (amvpt_interlace_host); quilt=True resamples the whole quilt instead."""
    L, _ = _libs()
    s = _src_u8(src)
    p = preset if preset is not None else default_preset()
    w, h = int(size[0]), int(size[1])
    out = np.empty((max(h, 0), max(w, 0), 3), dtype=np.uint8)
    _check_hip(L.amvpt_interlace_host(s.ctypes.data, s.shape[1], s.shape[0], s.shape[2], ctypes.byref(p),
                                      int(bool(quilt)), int(bool(nearest)), out.ctypes.data, w, h), L)
    return out


def views(preset=None, size=(1280, 720)):
    """The view index every subpixel picks: (size[1], size[0], 3) int32 (amvpt_interlace_views_host)."""
    L, _ = _libs()
    p = preset if preset is not None else default_preset()
    w, h = int(size[0]), int(size[1])
    out = np.empty((max(h, 0), max(w, 0), 3), dtype=np.int32)
    _check_hip(L.amvpt_interlace_views_host(ctypes.byref(p), out.ctypes.data, w, h), L)
    return out


def srgb8_device(image_ptr, channels, width, height, out_ptr, stream=None):
    """amvpt_srgb8 over device pointers, ordered on `stream` (a hipStream_t handle; None: the default stream)."""
    L, _ = _libs()
    _check_hip(L.amvpt_srgb8(ctypes.c_void_p(image_ptr), channels, width, height, ctypes.c_void_p(out_ptr),
                             ctypes.c_void_p(stream or 0)), L)


def interlace_device(src_ptr, src_w, src_h, src_channels, dst_ptr, size, preset=None, quilt=False, nearest=False,
                     stream=None):
    """amvpt_interlace over device pointers: the src_h x src_w x src_channels uint8 quilt at src_ptr -> the
    size[1] x size[0] x 3 uint8 image at dst_ptr, ordered on `stream`."""
    L, _ = _libs()
    p = preset if preset is not None else default_preset()
    _check_hip(L.amvpt_interlace(ctypes.c_void_p(src_ptr), src_w, src_h, src_channels, ctypes.byref(p),
                                 int(bool(quilt)), int(bool(nearest)), ctypes.c_void_p(dst_ptr), int(size[0]),
                                 int(size[1]), ctypes.c_void_p(stream or 0)), L)


def preset_for_scene(scene, sensor=0):
    """The default preset with `grid` from the sensor's view grid (a batch sensor gives n x 1)."""
    _, H = _libs()
    p = Preset()
    amvpt._check(H.amvpt_host_preset_for_scene(scene._h, sensor, ctypes.byref(p)), H)
    return p


def display(scene, preset=None, size=(1280, 720), quilt=False, nearest=False, sensor=0, seed=0, spp=0,
            counters=None, stream=None, rerender=True, denoise=None, tonemap=None, temporal=None, synth=None):
    """Render `scene` and run the display stage on the device (amvpt_host_display): render -> develop -> sRGB
    quilt -> lenticular image, one download -> (size[1], size[0], 3) uint8.  preset None: preset_for_scene.
    rerender=False runs the stage alone on the developed frame the last render / display of this sensor left on
    the device (amvpt_host_redisplay_stream): another preset, size or mode for the same frame.
    denoise None: the frame as rendered.  An amvpt.DenoiseParams, or True for amvpt.denoise's defaults, filters the
    developed frame on the device between develop and the sRGB quilt (amvpt_host_denoise_stream); the filtered frame
    is the cached one afterwards, so with rerender=False a frame already filtered is filtered again.
    temporal None: every frame stands alone, and the call and its bytes are what they are without the keyword.  An
    amvpt.TemporalAccumulator is applied between develop and the denoiser (_display_temporal): the frame is rendered,
    accumulated, filtered and shown through the C-ABI's device entries, and the accumulator keeps the history.
    With an accumulator built with moments=True, denoise may be an amvpt.VarianceParams: the variance-guided filter of
    include/amvpt_variance.h (temporal with moments -> amvpt_variance -> amvpt_denoise_variance) in the denoiser's
    place.
    synth None: the rendered quilt is the one shown, and the call and its bytes are what they are without the keyword.
    An amvpt.ViewSynthesizer makes the dense quilt of its own scene from the rendered one (include/amvpt_synth.h) after
    the accumulator and the denoiser (_display_synth): render -> develop -> (temporal) -> (denoise) -> synthesis -> sRGB
    quilt -> lenticular image, and preset None is preset_for_scene of the synthesizer's scene.
    tonemap None: the sRGB quilt clips at 1, and the call and its bytes are what they are without the keyword.  An
    amvpt.ToneMapper takes the place of the sRGB conversion at the end of the chain (include/amvpt_tonemap.h): the frame
    is metered where its parameters ask for it, scaled by one exposure for the whole quilt, mapped by the operator and
    written as sRGB bytes in one pass, after the accumulator, the denoiser and the synthesis where they are given, and
    over torch device tensors without them (_display_tonemap).  It needs a fresh frame, as the accumulator does."""
    if isinstance(denoise, amvpt.VarianceParams) and (temporal is None or not temporal.with_moments):
        raise ValueError("display: a VarianceParams denoiser needs temporal=TemporalAccumulator(moments=True)")
    if tonemap is not None and not rerender:
        raise ValueError("display: tone mapping needs a fresh frame (rerender=True)")
    if synth is not None:
        return _display_synth(scene, synth, temporal, preset, size, quilt, nearest, sensor, seed, spp, counters, stream,
                              rerender, denoise, tonemap)
    if temporal is not None:
        return _display_temporal(scene, temporal, preset, size, quilt, nearest, sensor, seed, spp, counters, stream,
                                 rerender, denoise, tonemap)
    if tonemap is not None:
        return _display_tonemap(scene, tonemap, preset, size, quilt, nearest, sensor, seed, spp, counters, stream, denoise)
    _, H = _libs()
    if denoise is not None and denoise is not False:
        if rerender:
            amvpt.render(scene, sensor=sensor, seed=seed, spp=spp, counters=counters, stream=stream)
        q = amvpt.denoise_params_for(scene, sensor, denoise if isinstance(denoise, amvpt.DenoiseParams) else None)
        amvpt.host_denoise(scene, q, sensor=sensor, replace=True, download=False, stream=stream)
        rerender = False
    w, h = int(size[0]), int(size[1])
    out = np.zeros((max(h, 0), max(w, 0), 3), dtype=np.uint8)
    if not rerender:
        amvpt._check(H.amvpt_host_redisplay_stream(scene._h, sensor,
                                                   ctypes.byref(preset) if preset is not None else None,
                                                   int(bool(quilt)), int(bool(nearest)), w, h,
                                                   ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(stream or 0)), H)
        return out
    cnt = counters if counters is not None else Counters()
    amvpt._check(H.amvpt_host_display_stream(scene._h, sensor, seed, spp,
                                             ctypes.byref(preset) if preset is not None else None,
                                             int(bool(quilt)), int(bool(nearest)), w, h,
                                             ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(stream or 0),
                                             ctypes.byref(cnt)), H)
    return out


def _quilt8(frame, c, w, h, tonemap, stream):
    """The 8-bit sRGB quilt of the float frame (a torch device tensor), the step the torch chains share: srgb8_device, or
    the tone mapper's metered and fused form in its place."""
    import torch
    if tonemap is not None:
        return tonemap.run(frame, stream=stream)
    q8 = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    srgb8_device(frame.data_ptr(), c, w, h, q8.data_ptr(), stream=stream)
    return q8


def _display_tonemap(scene, tonemap, preset, size, quilt, nearest, sensor, seed, spp, counters, stream, denoise):
    """display with a ToneMapper and neither an accumulator nor a synthesizer: render -> develop -> (denoiser) -> meter,
    tone map and sRGB -> lenticular image over torch device tensors, downloaded once.  The device scene is one the tone
    mapper keeps; the frame the host library caches for rerender=False is not touched."""
    import torch
    L, _ = _libs()
    sd, vd, p = scene.describe(sensor, seed, spp)
    dev = tonemap.device_scene_for(scene, sd)
    h, w = int(p.film_height), int(p.film_width)
    c = 4 if p.film_alpha else 3
    st = torch.cuda.current_stream() if not stream else torch.cuda.ExternalStream(int(stream))
    with torch.cuda.stream(st):
        film = torch.zeros((h, w, c + 1), dtype=torch.float32, device="cuda")
        frame = torch.empty((h, w, c), dtype=torch.float32, device="cuda")
        dev.render(vd, p, film.data_ptr(), stream=st.cuda_stream, counters=counters)
        _check_hip(L.amvpt_develop(ctypes.c_void_p(film.data_ptr()), ctypes.c_void_p(frame.data_ptr()), w, h, p.film_alpha,
                                   ctypes.c_void_p(st.cuda_stream)), L)
        if denoise is not None and denoise is not False:
            guides = torch.empty((h, w, 8), dtype=torch.float32, device="cuda")
            dev.guides(vd, p, guides.data_ptr(), stream=st.cuda_stream)
            q = denoise if isinstance(denoise, amvpt.DenoiseParams) else amvpt.DenoiseParams(
                sigma_plane=amvpt.denoise_sigma_plane(guides.cpu().numpy()))
            out, scratch = torch.empty_like(frame), torch.empty_like(frame)
            amvpt.denoise_device(frame.data_ptr(), c, w, h, guides.data_ptr(), out.data_ptr(), scratch.data_ptr(), q,
                                 stream=st.cuda_stream)
            frame = out
        q8 = _quilt8(frame, c, w, h, tonemap, st.cuda_stream)
        dw, dh = int(size[0]), int(size[1])
        shown = torch.empty((max(dh, 0), max(dw, 0), 3), dtype=torch.uint8, device="cuda")
        interlace_device(q8.data_ptr(), w, h, 3, shown.data_ptr(), (dw, dh), preset if preset is not None else
                         preset_for_scene(scene, sensor), quilt=quilt, nearest=nearest, stream=st.cuda_stream)
        st.synchronize()
        return shown.cpu().numpy()


def _display_temporal(scene, acc, preset, size, quilt, nearest, sensor, seed, spp, counters, stream, rerender, denoise,
                      tonemap=None):
    """display with a TemporalAccumulator: render -> develop -> temporal accumulation -> (denoiser) -> sRGB quilt ->
    lenticular image over torch device tensors; the display image is downloaded once (denoise=True also downloads
    the guide records, for denoise_sigma_plane; a DenoiseParams does not; a VarianceParams runs the accumulator's own
    variance and variance-guided filter instead, TemporalAccumulator.denoise).  The device scene is a second one beside
    the host library's, created once per scene and kept on the accumulator (TemporalAccumulator.device_scene_for);
    the frame the host library caches for rerender=False is not touched."""
    import torch
    if not rerender:
        raise ValueError("display: temporal accumulation needs a fresh frame (rerender=True)")
    L, _ = _libs()
    sd, vd, p = scene.describe(sensor, seed, spp)
    dev = acc.device_scene_for(scene, sd)
    h, w = int(p.film_height), int(p.film_width)
    c = 4 if p.film_alpha else 3
    st = torch.cuda.current_stream() if not stream else torch.cuda.ExternalStream(int(stream))
    with torch.cuda.stream(st):
        film = torch.zeros((h, w, c + 1), dtype=torch.float32, device="cuda")
        img = torch.empty((h, w, c), dtype=torch.float32, device="cuda")
        dev.render(vd, p, film.data_ptr(), stream=st.cuda_stream, counters=counters)
        _check_hip(L.amvpt_develop(ctypes.c_void_p(film.data_ptr()), ctypes.c_void_p(img.data_ptr()), w, h, p.film_alpha,
                                   ctypes.c_void_p(st.cuda_stream)), L)
        frame = acc.push(dev, vd, p, img, stream=st.cuda_stream)
        if isinstance(denoise, amvpt.VarianceParams):
            frame, _ = acc.denoise(denoise, stream=st.cuda_stream)
        elif denoise is not None and denoise is not False:
            q = denoise if isinstance(denoise, amvpt.DenoiseParams) else amvpt.DenoiseParams(
                sigma_plane=amvpt.denoise_sigma_plane(acc.guides.cpu().numpy()))
            out, scratch = torch.empty_like(frame), torch.empty_like(frame)
            amvpt.denoise_device(frame.data_ptr(), c, w, h, acc.guides.data_ptr(), out.data_ptr(), scratch.data_ptr(), q,
                                 stream=st.cuda_stream)
            frame = out
        q8 = _quilt8(frame, c, w, h, tonemap, st.cuda_stream)
        dw, dh = int(size[0]), int(size[1])
        shown = torch.empty((max(dh, 0), max(dw, 0), 3), dtype=torch.uint8, device="cuda")
        interlace_device(q8.data_ptr(), w, h, 3, shown.data_ptr(), (dw, dh), preset if preset is not None else
                         preset_for_scene(scene, sensor), quilt=quilt, nearest=nearest, stream=st.cuda_stream)
        st.synchronize()
        return shown.cpu().numpy()


def _display_synth(scene, synth, acc, preset, size, quilt, nearest, sensor, seed, spp, counters, stream, rerender, denoise,
                   tonemap=None):
    """display with a ViewSynthesizer, with or without a TemporalAccumulator: _display_temporal's chain over torch
    device tensors with the synthesis between the denoiser and the sRGB quilt; what is shown is the synthesizer's dense
    quilt.  The device scene is the accumulator's where there is one, else one the synthesizer keeps."""
    import torch
    if not rerender:
        raise ValueError("display: view synthesis needs a fresh frame (rerender=True)")
    L, _ = _libs()
    sd, vd, p = scene.describe(sensor, seed, spp)
    dev = acc.device_scene_for(scene, sd) if acc is not None else synth.device_scene_for(scene, sd)
    h, w = int(p.film_height), int(p.film_width)
    c = 4 if p.film_alpha else 3
    st = torch.cuda.current_stream() if not stream else torch.cuda.ExternalStream(int(stream))
    with torch.cuda.stream(st):
        film = torch.zeros((h, w, c + 1), dtype=torch.float32, device="cuda")
        img = torch.empty((h, w, c), dtype=torch.float32, device="cuda")
        dev.render(vd, p, film.data_ptr(), stream=st.cuda_stream, counters=counters)
        _check_hip(L.amvpt_develop(ctypes.c_void_p(film.data_ptr()), ctypes.c_void_p(img.data_ptr()), w, h, p.film_alpha,
                                   ctypes.c_void_p(st.cuda_stream)), L)
        if acc is not None:
            frame, guides = acc.push(dev, vd, p, img, stream=st.cuda_stream), acc.guides
        else:
            frame, guides = img, torch.empty((h, w, 8), dtype=torch.float32, device="cuda")
            dev.guides(vd, p, guides.data_ptr(), stream=st.cuda_stream)
        if isinstance(denoise, amvpt.VarianceParams):
            frame, _ = acc.denoise(denoise, stream=st.cuda_stream)
        elif denoise is not None and denoise is not False:
            q = denoise if isinstance(denoise, amvpt.DenoiseParams) else amvpt.DenoiseParams(
                sigma_plane=amvpt.denoise_sigma_plane(guides.cpu().numpy()))
            out, scratch = torch.empty_like(frame), torch.empty_like(frame)
            amvpt.denoise_device(frame.data_ptr(), c, w, h, guides.data_ptr(), out.data_ptr(), scratch.data_ptr(), q,
                                 stream=st.cuda_stream)
            frame = out
        dense, _ = synth.run(dev, vd, p, frame, guides, stream=st.cuda_stream)
        qh, qw = int(dense.shape[0]), int(dense.shape[1])
        q8 = _quilt8(dense, c, qw, qh, tonemap, st.cuda_stream)
        dw, dh = int(size[0]), int(size[1])
        shown = torch.empty((max(dh, 0), max(dw, 0), 3), dtype=torch.uint8, device="cuda")
        interlace_device(q8.data_ptr(), qw, qh, 3, shown.data_ptr(), (dw, dh), preset if preset is not None else
                         preset_for_scene(synth.scene, synth.sensor), quilt=quilt, nearest=nearest, stream=st.cuda_stream)
        st.synchronize()
        return shown.cpu().numpy()


def depth_quilt(scene, sensor=0, near=None, far=None):
    """The depth quilt of `scene` for an RGB-D display -> (H, W, 3) uint8, nearer brighter, a miss 0: the planar
    depth of every quilt pixel (amvpt.depth: k_guides and k_guide_depth on the device scene render() caches)
    coded by amvpt.depth8_host.  A bound left None comes from the frame itself (amvpt.guide_depth_range_host:
    the nearest hit 255, the farthest 0).  The host forms are bit-identical to the device entries."""
    z = amvpt.depth(scene, sensor)
    if near is None or far is None:
        lo, hi = amvpt.guide_depth_range_host(z)
        near = lo if near is None else near
        far = hi if far is None else far
    return amvpt.depth8_host(z, near, far)


def read_presets(path):
    """The presets of a presets.csv (name;center;focus;pitch;tilt;subp;view0;view1;grid0;grid1;flip_rgb)."""
    _, H = _libs()
    n = u32()
    amvpt._check(H.amvpt_host_read_presets(str(path).encode(), None, 0, ctypes.byref(n)), H)
    buf = (_NamedPreset * max(1, n.value))()
    amvpt._check(H.amvpt_host_read_presets(str(path).encode(), ctypes.addressof(buf), n.value, ctypes.byref(n)), H)
    return [Preset._from_c(buf[i].preset, buf[i].name.decode()) for i in range(min(n.value, len(buf)))]


def write_presets(path, presets):
    _, H = _libs()
    buf = (_NamedPreset * max(1, len(presets)))()
    for i, p in enumerate(presets):
        buf[i].name = p.name.encode()[:63]
        ctypes.memmove(ctypes.addressof(buf[i].preset), ctypes.addressof(p), ctypes.sizeof(Preset))
    amvpt._check(H.amvpt_host_write_presets(str(path).encode(), ctypes.addressof(buf), len(presets)), H)


def write_png(path, image):
    """(H, W, 3) uint8 -> an 8-bit RGB PNG (amvpt_host_write_png)."""
    _, H = _libs()
    img = np.ascontiguousarray(image)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("write_png: an (H, W, 3) uint8 image is needed")
    amvpt._check(H.amvpt_host_write_png(str(path).encode(), img.ctypes.data, img.shape[1], img.shape[0]), H)
